"""K17, the `.ovl` codec on the device (ndgpu_ovl_decode_batch, ndgpu_ovl_encode_batch, ndgpu_ovl_sort_images, ndgpu_admit_piles_image).
Expected values come from the reference's files and the pinned host routines only: the golden `.ovl` bytes, ovl.decode_ovl_numpy,
ndgpu_ovl_decode and ndgpu_ovl_encode (held to the compiled reference by test_stage_cli.py) -- never from the device path.
tests/test_simt_codec.py runs the same bodies under the interpreter.

Sizes the kernels change path at (csrc/ovlsort_kernels.hip): a lane reads 16 bytes, a wavefront 1,024 per iteration, a decode tile is
4,096 bytes; the per-record kernels run 256 lanes a block; an encode wavefront stages 64 records."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_ovlsort as GS  # noqa: E402
import test_zz_gpu_admit as GA  # noqa: E402

pytestmark = pytest.mark.gpu
STAGE = GS.STAGE
LANE, ITER, TILE, BLOCK = 16, 1024, 4096, 256
FIELDS = ("qname", "rev", "qs", "qe", "tname", "ts", "te", "match")   # decode_ovl's order


# ---------------------------------------------------------------- the pinned host routines
def _host_decode(blob):
    """ndgpu_ovl_decode over a byte string -> (uint32[n, 8] in decode_ovl's order, consumed)."""
    from nextdenovo_amd import ovl
    lib = ovl._native()
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)
    cap = buf.size // 8 + 1
    out = np.zeros((cap, 8), dtype=np.uint32)
    prev = np.zeros(2, dtype=np.uint32)
    used = C.c_uint64(0)
    n = lib.ndgpu_ovl_decode(buf.ctypes.data if buf.size else None, buf.size, prev.ctypes.data, out.ctypes.data, cap, C.byref(used))
    return out[:n].copy(), int(used.value)


def _host_encode(rows, prev=(0, 0)):
    """ndgpu_ovl_encode over rows in decode_ovl's order -> (bytes, prev afterwards)."""
    from nextdenovo_amd import overlap
    p = np.asarray(prev, dtype=np.uint32).copy()
    recs = overlap.from_decoded(np.asarray(rows, dtype=np.uint32).reshape(-1, 8))
    return overlap.encode(recs, p), p


def _decoded(recs):
    """A record array -> uint32[n, 8] in decode_ovl's order."""
    return np.stack([recs[c] for c in FIELDS], axis=1) if recs.size else np.zeros((0, 8), dtype=np.uint32)


def _varint_lengths(blob):
    """The byte length of every complete value of a byte string, and the bytes behind the last one."""
    b = np.frombuffer(bytes(blob), dtype=np.uint8)
    ends = np.flatnonzero(b < 128)
    return np.diff(np.r_[-1, ends]).tolist(), int(b.size - (ends[-1] + 1 if ends.size else 0))


def _check_decode(blobs, alone=True):
    """decode_images over the byte strings in one call == ndgpu_ovl_decode of each: records, counts, consumed; and each alone."""
    from nextdenovo_amd import overlap
    want = [_host_decode(b) for b in blobs]
    recs, per_file, used, st = overlap.decode_images(blobs)
    assert per_file.tolist() == [w[0].shape[0] for w in want]
    assert used.tolist() == [w[1] for w in want]
    at = 0
    for k, (w, _) in enumerate(want):
        assert np.array_equal(_decoded(recs[at:at + w.shape[0]]), w), k
        at += w.shape[0]
    assert at == recs.size == st["records"] and st["bytes_in"] == sum(len(b) for b in blobs)
    if sum(len(b) for b in blobs):
        assert st["host_decodes"] == 0 and st["bytes_uploaded"] == st["bytes_in"]
    if alone and len(blobs) > 1:
        for k, b in enumerate(blobs):
            r1, p1, u1, _ = overlap.decode_images([b])
            assert np.array_equal(_decoded(r1), want[k][0]) and p1.tolist() == [want[k][0].shape[0]] and u1.tolist() == [want[k][1]], k
    return want


def _random_rows(rng, n, big=False):
    """n records in decode_ovl's order, names walking up and down, both span orders."""
    hi = 2 ** 32 if big else 70000
    q = rng.integers(0, hi, n, dtype=np.uint64)
    t = rng.integers(0, hi, n, dtype=np.uint64)
    qs = rng.integers(0, 30000, n, dtype=np.uint64)
    ts = rng.integers(0, 30000, n, dtype=np.uint64)
    ql = rng.integers(0, 40000, n, dtype=np.uint64)
    tl = rng.integers(0, 40000, n, dtype=np.uint64)
    return np.stack([q, rng.integers(0, 2, n, dtype=np.uint64), qs, qs + ql, t, ts, ts + tl, rng.integers(0, 50000, n, dtype=np.uint64)],
                    axis=1).astype(np.uint32)


# ---------------------------------------------------------------- 1. the golden files
def _golden_files():
    g = os.path.join(HERE, "golden")
    return sorted(glob.glob(os.path.join(g, "overlap", "*.ovl"))) + sorted(glob.glob(os.path.join(g, "cigar", "*.ovl"))) \
        + [os.path.join(STAGE, "input.seed.001.sorted.ovl")]


_GOLD = {}


def _golden():
    """(path, bytes, the numpy decoder's records), read and decoded once."""
    if not _GOLD:
        from nextdenovo_amd import ovl
        _GOLD["v"] = [(p, open(p, "rb").read(), ovl.decode_ovl_numpy(p)) for p in _golden_files()]
    return _GOLD["v"]


def test_golden_files_decode_to_the_numpy_decoder_and_encode_back():
    from nextdenovo_amd import overlap
    gold = _golden()
    assert len(gold) == 33
    for p, blob, want in gold:
        recs, per_file, used, _ = overlap.decode_images([blob])
        assert np.array_equal(_decoded(recs), want), p
        assert per_file.tolist() == [want.shape[0]] and used.tolist() == [len(blob)], p
        prev = np.zeros(2, dtype=np.uint32)
        assert overlap.encode_device(recs, prev) == blob, p
        assert prev.tolist() == [int(want[-1, 0]), int(want[-1, 4])], p


def test_golden_files_in_one_call_equal_each_alone():
    from nextdenovo_amd import overlap
    gold = _golden()
    recs, per_file, used, st = overlap.decode_images([g[1] for g in gold])
    assert per_file.tolist() == [g[2].shape[0] for g in gold] and used.tolist() == [len(g[1]) for g in gold]
    at = 0
    for p, _blob, want in gold:
        assert np.array_equal(_decoded(recs[at:at + want.shape[0]]), want), p
        at += want.shape[0]
    assert st["records"] == at and st["host_decodes"] == 0 and st["bytes_downloaded"] == 32 * at


# ---------------------------------------------------------------- 2. directed decode streams
def _padded_value(v, nbytes):
    """v as a varint of exactly nbytes bytes (continuation bytes of zero in front where it is shorter)."""
    groups = [(v >> (7 * g)) & 127 for g in range(nbytes - 1, -1, -1)]
    assert sum(g << (7 * (nbytes - 1 - i)) for i, g in enumerate(groups)) == v & ((1 << 7 * nbytes) - 1)
    return bytes([g | 128 for g in groups[:-1]] + [groups[-1]])


def test_values_of_one_to_five_bytes_in_every_field():
    """Field k of record (5 k + L - 1) is L bytes long; the flag field takes its longer forms as over-long values (the encoder never
    writes them, the loop reads them)."""
    natural = {1: 100, 2: 9000, 3: 2000000, 4: 200000000, 5: 0xfedcba98}
    blob = b""
    for k in range(8):
        for ln in range(1, 6):
            vals = [3, 0, 7, 11, 2, 5, 1, 9]
            parts = [_padded_value(v, 1) for v in vals]
            parts[k] = _padded_value(natural[ln] if k != 1 else (1 + 2 * ln) & 15, ln)   # (the flags: 3, 5, 7, 9, 11)
            blob += b"".join(parts)
    lens, tail = _varint_lengths(blob)
    assert tail == 0 and len(lens) == 8 * 40
    for k in range(8):
        for ln in range(1, 6):
            assert lens[8 * (5 * k + ln - 1) + k] == ln
    want = _check_decode([blob])
    assert want[0][0].shape[0] == 40
    # five bytes: the fifth from last keeps its low 4 bits (0xfedcba98 came back whole; 0x7f on top of it does not)
    b5 = bytes([0xff, 0xff, 0xff, 0xff, 0x7f]) + bytes(7)
    (w, used), = _check_decode([b5])
    assert w[0, 0] == 0xffffffff and used == 12
    # six and more continuation bytes in front: shifted out
    b9 = bytes([0x81] * 9 + [0x02]) + bytes(7)
    (w, used), = _check_decode([b9])
    assert w[0, 0] == ((0x01 << 28) | (0x01 << 21) | (0x01 << 14) | (0x01 << 7) | 2) & 0xffffffff and used == 17


@pytest.mark.parametrize("boundary", [LANE, ITER, TILE, 2 * TILE], ids=["lane", "iteration", "tile", "second-tile"])
@pytest.mark.parametrize("nbytes", [2, 3, 4, 5])
def test_a_value_straddling_a_boundary(boundary, nbytes):
    """A value of `nbytes` bytes whose terminator is the first byte behind the boundary, all its other bytes in front of it."""
    rng = np.random.default_rng(boundary + nbytes)
    rows = _random_rows(rng, 700)
    rows[:, 7] = {2: 9000, 3: 2000000, 4: 200000000, 5: 0}[nbytes] + np.arange(700)   # `match`: a value of nbytes bytes in every record
    if nbytes == 5:
        rows[:, 7] = 0xf0000000 + np.arange(700)
    body, _ = _host_encode(rows)
    lens, _ = _varint_lengths(body)
    ends = np.cumsum(lens) - 1
    e = next(int(e) for e, ln, j in zip(ends, lens, range(len(lens))) if j % 8 == 7 and j > 8 and ln == nbytes)
    room = boundary - (nbytes - 1)        # bytes in front of the value: values of the stream as far as they fit, then one-byte zeros
    starts = np.r_[0, ends + 1]
    m = int(starts[starts <= room].max())
    blob = body[:m] + bytes(room - m) + body[e - nbytes + 1:]   # (the field phase moves: the host loop says what comes out)
    b = np.frombuffer(blob, dtype=np.uint8)
    assert b[boundary] < 128 and all(b[boundary - k] >= 128 for k in range(1, nbytes)) and b[boundary - nbytes] < 128
    assert len(blob) > boundary + 100
    _check_decode([blob])


def test_flags_set_and_clear_next_to_each_other():
    """Names going up and down from record to record, tspan above and below qspan: flags 2, 4 and 8 in every combination."""
    rows = []
    for i in range(200):
        q = 5000 + (-1) ** i * 37 * (i % 5) + (i // 3) * 11 * (-1) ** (i // 7)
        t = 90000 + (-1) ** (i // 2) * 1000 * (i % 3)
        qs, ts = 10 * i, 7 * i
        ql, tl = 800 + 13 * (i % 9), 800 + 13 * ((i + 4) % 9)
        rows.append([q, i & 1, qs, qs + ql, t, ts, ts + tl, 500 + i])
    blob, _ = _host_encode(rows)
    (w, used), = _check_decode([blob])
    assert np.array_equal(w, np.asarray(rows, dtype=np.uint32)) and used == len(blob)
    flags = _raw_fields(blob)[:, 1]
    assert {int(f) & 14 for f in flags} == {0, 2, 4, 6, 8, 10, 12, 14}


def _raw_fields(blob):
    """The eight values of every whole record, as written (no deltas applied)."""
    from nextdenovo_amd import ovl
    v = ovl.decode_varints(np.frombuffer(bytes(blob), dtype=np.uint8))
    return np.asarray(v[: v.size // 8 * 8]).reshape(-1, 8)


def test_empty_short_and_partial_files():
    rng = np.random.default_rng(5)
    body, _ = _host_encode(_random_rows(rng, 90))
    lens, _ = _varint_lengths(body)
    ends = np.cumsum(lens)
    whole = int(ends[8 * 50 - 1])                      # 50 records
    seven = body[:int(ends[8 * 50 + 7 - 1])]           # ... and 7 values of the next
    j = next(k for k in range(8 * 50, len(lens)) if lens[k] >= 2)
    on_cont = body[:int(ends[j]) - 1]                  # ... and a tail that ends on a continuation byte
    assert len(_varint_lengths(seven)[0]) == 8 * 50 + 7 and _varint_lengths(seven)[1] == 0
    assert on_cont[-1] >= 128 and _varint_lengths(on_cont)[1] >= 1
    few = bytes([1, 2, 0x81, 3, 4, 5, 6, 7])           # 7 terminators
    assert sum(1 for c in few if c < 128) == 7
    only_cont = bytes([0x80] * 40)
    want = _check_decode([b"", few, seven, on_cont, only_cont, body[:whole], b""])
    assert [w[0].shape[0] for w in want] == [0, 0, 50, 50, 0, 50, 0]
    assert [w[1] for w in want] == [0, 0, whole, whole, 0, whole, 0]
    # nothing at all
    from nextdenovo_amd import overlap
    recs, per_file, used, st = overlap.decode_images([])
    assert recs.size == 0 and per_file.size == 0 and used.size == 0 and all(v == 0 for v in st.values())
    recs, per_file, used, st = overlap.decode_images([b"", b""])
    assert recs.size == 0 and per_file.tolist() == [0, 0] and used.tolist() == [0, 0] and all(v == 0 for v in st.values())


def test_three_files_the_middle_one_with_a_partial_tail():
    """The next file's field phase and its names start afresh."""
    rng = np.random.default_rng(6)
    a, _ = _host_encode(_random_rows(rng, 300))
    b, _ = _host_encode(_random_rows(rng, 500))
    c_rows = _random_rows(rng, 400)
    c, _ = _host_encode(c_rows)
    lens, _ = _varint_lengths(b)
    cut = int(np.cumsum(lens)[8 * 333 + 3 - 1])        # 333 records and 3 values
    want = _check_decode([a, b[:cut], c])
    assert [w[0].shape[0] for w in want] == [300, 333, 400] and want[1][1] < cut
    assert np.array_equal(want[2][0], c_rows)
    assert len(a) > TILE and cut > TILE                 # more than one tile each


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_record_counts_around_the_wavefront_and_the_block(n):
    rng = np.random.default_rng(n)
    rows = _random_rows(rng, n, big=True)
    blob, _ = _host_encode(rows)
    (w, used), = _check_decode([blob])
    assert np.array_equal(w, rows) and used == len(blob)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_byte_counts_around_the_tile(delta):
    """Files that end one byte in front of, at and one byte behind a tile boundary, and a second file behind them."""
    rng = np.random.default_rng(40 + delta)
    body, _ = _host_encode(_random_rows(rng, 900))
    assert len(body) > 2 * TILE
    blob = body[:2 * TILE + delta]
    tail, _ = _host_encode(_random_rows(rng, 70))
    _check_decode([blob, tail, body[:TILE + delta]])


# ---------------------------------------------------------------- 3. random bytes: no input declines
def _random_blobs():
    rng = np.random.default_rng(17)
    out = []
    for k in range(200):
        n = int(rng.integers(0, 5001)) if k > 3 else (0, 1, 7, 5000)[k]
        p = float(rng.choice([0.1, 0.35, 0.6, 0.85, 0.97]))
        b = rng.integers(0, 128, n, dtype=np.uint8) | (rng.random(n) < p).astype(np.uint8) << 7
        out.append(b.tobytes())
    return out


def test_random_byte_strings_equal_the_host_loop():
    blobs = _random_blobs()
    longest = 0
    for b in blobs:
        a = np.frombuffer(b, dtype=np.uint8) >= 128
        run = 0
        for x in a[:600]:
            run = run + 1 if x else 0
            longest = max(longest, run)
    assert longest > 5                                   # runs of more than 5 continuation bytes are in there
    for at in range(0, 200, 25):
        _check_decode(blobs[at:at + 25], alone=at == 0)


# ---------------------------------------------------------------- 4. directed encode
_EDGE_VALUES = [0, 1, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 28 - 1, 2 ** 28, 2 ** 28 + 1, 2 ** 32 - 1]


def _edge_rows():
    """Every edge value in every encoded field: as a name delta up and down, flags, start, span, span difference either way, match."""
    rows = []
    for v in _EDGE_VALUES:
        m = 2 ** 32
        rows.append([v, 0, v, v, (m - v) % m, v, v, v])                      # deltas from (0 or the last) up / down, spans of 0
        rows.append([0, 1, 5, (5 + v) % m, v, 9, 9, 0])                      # qspan = v, tspan = 0: difference v, flag 8 clear
        rows.append([v, 0x80, 5, 5, 0, 9, (9 + v) % m, (m - 1 - v) % m])     # tspan = v above qspan = 0: flag 8; a flag byte of 2 bytes
    return np.asarray(rows, dtype=np.uint32)


def _check_encode(rows, prev=(0, 0)):
    from nextdenovo_amd import overlap
    want, want_prev = _host_encode(rows, prev)
    p = np.asarray(prev, dtype=np.uint32).copy()
    recs = overlap.from_decoded(np.asarray(rows, dtype=np.uint32).reshape(-1, 8))
    got, st = overlap.encode_device(recs, p, want_stats=True)
    assert got == want and p.tolist() == want_prev.tolist()
    assert st["bytes_out"] == len(want) and st["records"] == recs.size
    if recs.size:
        assert st["bytes_uploaded"] == 32 * recs.size and st["bytes_downloaded"] == len(want)
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
@pytest.mark.parametrize("prev", [(0, 0), (70000, 3)], ids=["fresh", "carried"])
def test_encode_record_counts(n, prev):
    rng = np.random.default_rng(100 + n)
    _check_encode(_random_rows(rng, n), prev)
    _check_encode(_random_rows(rng, n, big=True), prev)


def test_encode_field_edges():
    rows = _edge_rows()
    blob = _check_encode(rows)
    lens, _ = _varint_lengths(blob)
    assert set(lens) == {1, 2, 3, 4, 5}
    _check_encode(rows, (2 ** 32 - 1, 128))
    _check_encode(rows[::-1].copy(), (127, 2 ** 28))
    # the longest record the encoder writes (seven values of 5 bytes and two flag bytes: 37) next to shorter ones, 64 times over
    wide = [[2 ** 31 + 5, 0x81, 2 ** 30, 2 ** 30 + 2 ** 29, 2 ** 31 + 7, 2 ** 30, 2 ** 30 + 2 ** 31, 2 ** 32 - 1], [5, 0x81, 2 ** 30, 2 ** 30 + 2 ** 29, 2, 2 ** 30, 2 ** 31, 2 ** 32 - 1]]
    blob = _check_encode(np.asarray(wide * 64, dtype=np.uint32))
    assert max(np.add.reduceat(_varint_lengths(blob)[0], np.arange(0, 8 * 128, 8))) == 37
    _check_encode(np.zeros((130, 8), dtype=np.uint32))   # 8 bytes each


def test_two_encode_calls_chained_through_prev_equal_one():
    from nextdenovo_amd import overlap
    rng = np.random.default_rng(9)
    rows = _random_rows(rng, 333, big=True)
    want, want_prev = _host_encode(rows)
    recs = overlap.from_decoded(rows)
    for cut in (1, 64, 100, 332):
        p = np.zeros(2, dtype=np.uint32)
        got = overlap.encode_device(recs[:cut], p) + overlap.encode_device(recs[cut:], p)
        assert got == want and p.tolist() == want_prev.tolist(), cut


# ---------------------------------------------------------------- 5. the fused calls
def _stage_images():
    """The input set of test_gpu_ovlsort as `.ovl` images (the host encoder's), with the seed table."""
    files, sl, mn = GA._stage_raw()
    return [_host_encode(_decoded(f))[0] for f in files], files, sl, mn


def _bl_text(bl):
    return "".join("%d %s\n" % x for x in bl).encode()


@pytest.mark.parametrize("hq", [False, True], ids=["plain", "H"])
def test_sort_images_equals_decode_sort_encode(hq, monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.delenv("NDGPU_OVLSORT_PIECE_RECORDS", raising=False)
    monkeypatch.delenv("NDGPU_OVLSORT_RANGE_CANDIDATES", raising=False)
    images, _files, sl, mn = _stage_images()
    decoded = [overlap.from_decoded(_host_decode(b)[0]) for b in images]
    srt, bl, _ = overlap.sort_overlaps(decoded, sl, mn, 40, 300, hq=hq)
    want = overlap.encode(srt, np.zeros(2, dtype=np.uint32))
    if not hq:
        assert want == GS._golden("input.seed.001.sorted.ovl") and _bl_text(bl) == GS._golden("input.seed.001.sorted.ovl.bl")
    # in core: bytes up, bytes down
    img, got_bl, st = overlap.sort_images(images, sl, mn, 40, 300, hq=hq)
    assert img.tobytes() == want and got_bl == bl
    cs = st["codec"]
    assert st["sort"]["ranges"] == 1 and st["sort"]["kept"] == srt.size and cs["host_decodes"] == 0
    assert cs["bytes_uploaded"] == sum(len(b) for b in images) == cs["bytes_in"]
    assert cs["bytes_downloaded"] == len(want) == cs["bytes_out"]
    assert cs["records"] == sum(d.size for d in decoded) and cs["decode_ms"] > 0 and cs["encode_ms"] > 0
    # the host legs around the same sort
    img, got_bl, st = overlap.sort_images(images, sl, mn, 40, 300, hq=hq, flags=1)
    assert img.tobytes() == want and got_bl == bl and st["codec"]["decode_ms"] == 0 and st["codec"]["encode_ms"] == 0
    # forced out of core: host decode, every range encoded on the device, prev carried
    monkeypatch.setenv("NDGPU_OVLSORT_PIECE_RECORDS", "257")
    monkeypatch.setenv("NDGPU_OVLSORT_RANGE_CANDIDATES", "900")
    img, got_bl, st = overlap.sort_images(images, sl, mn, 40, 300, hq=hq)
    assert img.tobytes() == want and got_bl == bl
    assert st["sort"]["ranges"] >= 3 and st["codec"]["host_decodes"] == len(images) and st["codec"]["encode_ms"] > 0
    assert st["codec"]["bytes_uploaded"] == 0 and st["codec"]["bytes_downloaded"] == len(want)
    # (prev carried: equality with `want` above is the check; this says it bites -- a range that restarted from prev = {0, 0} at a seed
    # boundary would write other bytes)
    cut = int(np.flatnonzero(np.diff(srt["qname"]))[srt.size // 100]) + 1
    restarted = overlap.encode(srt[cut:], np.zeros(2, dtype=np.uint32))
    assert restarted != want[len(want) - len(restarted):]


def test_sort_images_decides_its_form_once(monkeypatch):
    """NDGPU_OVLSORT_AVAIL_BYTES stands in for the device's free memory.  Between the bound from the image size (a record is 40 bytes
    at most) and the real record count the images are counted on the device, found too many and decoded by the host loop for the
    sort in seed ranges; a figure that lets the count fit keeps the call in core whatever the memory looks like afterwards."""
    from nextdenovo_amd import overlap
    monkeypatch.delenv("NDGPU_OVLSORT_PIECE_RECORDS", raising=False)
    monkeypatch.delenv("NDGPU_OVLSORT_RANGE_CANDIDATES", raising=False)
    images, _files, sl, mn = _stage_images()
    want = GS._golden("input.seed.001.sorted.ovl")
    n_bytes = sum(len(b) for b in images)
    n_rec = sum(_host_decode(b)[0].shape[0] for b in images)
    assert n_bytes // 40 < n_rec
    # the image bound fits, the count does not
    monkeypatch.setenv("NDGPU_OVLSORT_AVAIL_BYTES", str(360 * ((n_bytes // 40 + n_rec) // 2)))
    img, bl, st = overlap.sort_images(images, sl, mn, 40, 300)
    assert img.tobytes() == want and _bl_text(bl) == GS._golden("input.seed.001.sorted.ovl.bl")
    assert st["codec"]["host_decodes"] == len(images) and st["codec"]["bytes_uploaded"] == 0 and st["codec"]["records"] == n_rec
    # not even the image bound fits: no device count at all
    monkeypatch.setenv("NDGPU_OVLSORT_AVAIL_BYTES", str(360 * (n_bytes // 40) - 1))
    img, bl, st = overlap.sort_images(images, sl, mn, 40, 300)
    assert img.tobytes() == want and st["codec"]["host_decodes"] == len(images) and st["codec"]["decode_ms"] == 0
    # the count fits exactly: in core, decoded on the device
    monkeypatch.setenv("NDGPU_OVLSORT_AVAIL_BYTES", str(360 * n_rec))
    img, bl, st = overlap.sort_images(images, sl, mn, 40, 300)
    assert img.tobytes() == want and st["codec"]["host_decodes"] == 0 and st["codec"]["bytes_uploaded"] == n_bytes and st["sort"]["ranges"] == 1
    # one byte less: in seed ranges
    monkeypatch.setenv("NDGPU_OVLSORT_AVAIL_BYTES", str(360 * n_rec - 1))
    img, bl, st = overlap.sort_images(images, sl, mn, 40, 300)
    assert img.tobytes() == want and st["codec"]["host_decodes"] == len(images)


_TH3 = ((1250, 500, 130, 10), (3000, 900, 4, 2), (0, 500, 1, 1))
_SKIP3 = ((), (3, 5, 40), ())


@pytest.mark.parametrize("k", [0, 1, 2])
def test_admit_piles_image_on_the_stage_fixture(k):
    from nextdenovo_amd import overlap, ovl
    path = os.path.join(STAGE, "input.seed.001.sorted.ovl")
    blob = open(path, "rb").read()
    recs = overlap.from_decoded(ovl.decode_ovl(path))
    n_ids = int(max(recs["qname"].max(), recs["tname"].max())) + 1
    want = overlap.assemble_piles(recs, n_ids, *_TH3[k], sorted(_SKIP3[k]))
    two = overlap.admit_piles(recs, n_ids, *_TH3[k], sorted(_SKIP3[k]))
    got = overlap.admit_piles_image(blob, n_ids, *_TH3[k], sorted(_SKIP3[k]))
    GA._same(got[:3], want)
    GA._same(got[:3], two[:3])
    st = got[3]
    assert st["admit"]["groups_declined"] == 0 and st["admit"]["groups"] == 143 and st["admit"]["sorted_records"] == recs.size
    assert st["codec"]["bytes_uploaded"] == len(blob) and st["codec"]["host_decodes"] == 0 and st["codec"]["records"] == recs.size
    host = overlap.admit_piles_image(blob, n_ids, *_TH3[k], sorted(_SKIP3[k]), flags=1)
    GA._same(host[:3], want)
    assert host[3]["codec"]["decode_ms"] == 0 and host[3]["admit"]["k16_ms"] == 0 and host[3]["codec"]["host_decodes"] == 1


def test_admit_piles_image_on_a_stream_that_declines():
    from nextdenovo_amd import overlap
    _name, rows, th = GA._DECLINE[0]
    recs = GA._rows(rows)
    blob, _ = _host_encode(np.asarray(rows, dtype=np.uint32))
    want = overlap.assemble_piles(recs, GA.N_IDS, *th)
    got = overlap.admit_piles_image(blob, GA.N_IDS, *th)
    GA._same(got[:3], want)
    assert got[3]["admit"]["groups_declined"] >= 1 and got[3]["codec"]["host_decodes"] == 1
    # nothing in
    r, off, seeds, st = overlap.admit_piles_image(b"", 10, 1250)
    assert r.shape == (0, 8) and off.tolist() == [0] and seeds.size == 0 and st["codec"]["records"] == 0 and st["codec"]["bytes_uploaded"] == 0


# ---------------------------------------------------------------- 6. the command lines
def _stage_dir(tmp_path):
    """The stage fixture with the two step-1 files written by the host encoder, and the fofn files."""
    import shutil
    d = str(tmp_path / "w")
    shutil.copytree(STAGE, d)
    images, _files, _sl, _mn = _stage_images()
    fofn = os.path.join(d, "ovl.fofn")
    with open(fofn, "w") as f:
        for k, b in enumerate(images):
            p = os.path.join(d, "raw%d.ovl" % k)
            open(p, "wb").write(b)
            f.write(p + "\n")
    idxs = os.path.join(d, "idxs.fofn")
    with open(idxs, "w") as f:
        for n in sorted(os.listdir(d)):
            if n.startswith(".input.") and n.endswith(".idx"):
                f.write(os.path.join(d, n) + "\n")
    return d, fofn, idxs


def _setenv(monkeypatch, name, on):
    if on:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("codec", [False, True], ids=["host-codec", "device-codec"])
def test_ovl_sort_command_writes_the_golden_files(codec, tmp_path, monkeypatch):
    from nextdenovo_amd import ovl_sort
    _setenv(monkeypatch, "NDGPU_CODEC_DEVICE", codec)
    d, fofn, _ = _stage_dir(tmp_path)
    so = os.path.join(d, "mine.sorted.ovl")
    assert ovl_sort.run(["-m", "2g", "-t", "4", "-k", "40", "-i", os.path.join(d, ".input.seed.001.idx"), "-o", so, fofn]) == 0
    assert open(so, "rb").read() == GS._golden("input.seed.001.sorted.ovl")
    assert open(so + ".bl", "rb").read() == GS._golden("input.seed.001.sorted.ovl.bl")


@pytest.mark.parametrize("admit", [False, True], ids=["host-admit", "device-admit"])
@pytest.mark.parametrize("codec", [False, True], ids=["host-codec", "device-codec"])
def test_nextcorrect_command_writes_the_golden_fasta(codec, admit, tmp_path):
    d, _, idxs = _stage_dir(tmp_path)
    so = os.path.join(d, "input.seed.001.sorted.ovl")
    out = os.path.join(d, "cns.fasta")
    env = {k: v for k, v in os.environ.items() if k not in ("NDGPU_CODEC_DEVICE", "NDGPU_ADMIT_DEVICE")}
    if codec:
        env["NDGPU_CODEC_DEVICE"] = "1"
    if admit:
        env["NDGPU_ADMIT_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "nextdenovo_amd.nextcorrect", "-f", idxs, "-i", so, "-r", "ont", "-p", "4", "-min_len_seed", "1250", "-o", out]
    r = subprocess.run(cmd, cwd=os.path.dirname(HERE), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == GS._golden("cns.default.fasta", gz=True)
    assert open(out + ".idx", "rb").read() == GS._golden("cns.default.fasta.idx", gz=True)


def test_keep_files_of_the_fused_stage_with_the_device_encoder(tmp_path, monkeypatch):
    """correct_stage --keep under NDGPU_CODEC_DEVICE=1: the sorted.ovl it keeps is the golden one."""
    from nextdenovo_amd import correct_stage
    monkeypatch.setenv("NDGPU_CODEC_DEVICE", "1")
    keep = str(tmp_path / "keep")
    out = str(tmp_path / "cns")
    assert correct_stage.run(["-d", STAGE, "-x", "ava-ont", "-k", "40", "-r", "ont", "-min_len_seed", "1250", "-p", "4", "-o", out, "--keep", keep]) == 0
    assert open(os.path.join(keep, "input.seed.001.sorted.ovl"), "rb").read() == GS._golden("input.seed.001.sorted.ovl")
    assert open(out + ".001.fasta", "rb").read() == GS._golden("cns.default.fasta", gz=True)


# ---------------------------------------------------------------- 7. the interface
NEW_NAMES = {"ndgpu_ovl_decode_batch", "ndgpu_ovl_encode_batch", "ndgpu_ovl_sort_images", "ndgpu_admit_piles_image"}


def test_the_new_entry_points_are_exported_and_declared():
    from nextdenovo_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.OVL_LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NEW_NAMES <= names
    assert all(n.startswith(("ndgpu_", "__hip_cuid_")) or n == "ksw_extd2_sse" for n in names), sorted(names)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ndgpu_overlap.h")).read()
    assert all(n + "(" in header for n in NEW_NAMES) and "ndgpu_ovl_codec_stats" in header


def test_the_host_flag_gives_the_same_answers_without_device_time():
    from nextdenovo_amd import overlap
    gold = _golden()[:3]
    blobs = [g[1] for g in gold] + [b"\x81\x82", bytes(20)]
    dev = overlap.decode_images(blobs)
    host = overlap.decode_images(blobs, flags=1)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tolist() == host[1].tolist() and dev[2].tolist() == host[2].tolist()
    assert host[3]["decode_ms"] == 0 and host[3]["encode_ms"] == 0 and host[3]["host_decodes"] == len(blobs) and dev[3]["decode_ms"] > 0
    p1, p2 = np.asarray([5, 6], dtype=np.uint32), np.asarray([5, 6], dtype=np.uint32)
    a, st_a = overlap.encode_device(dev[0], p1, want_stats=True)
    b, st_b = overlap.encode_device(dev[0], p2, flags=1, want_stats=True)
    assert a == b and p1.tolist() == p2.tolist() and st_b["encode_ms"] == 0 and st_b["decode_ms"] == 0 and st_a["encode_ms"] > 0


def test_argument_errors_leave_the_out_pointers_null():
    from nextdenovo_amd import overlap
    lib = overlap.load()
    overlap.decode_images([])                               # (binds the argument types)
    overlap.encode_device(np.zeros(0, dtype=overlap.REC), np.zeros(2, dtype=np.uint32))
    overlap.sort_images([], np.zeros(1, dtype=np.uint32), 0)
    overlap.admit_piles_image(b"", 1, 1)
    P = C.c_void_p
    recs, per, st = P(), (C.c_int64 * 2)(7, 7), overlap.CodecStats()
    one = (C.c_uint64 * 1)(16)
    assert lib.ndgpu_ovl_decode_batch(None, one, 1, 0, C.byref(recs), per, None, C.byref(st)) < 0 and not recs.value and per[0] == 7
    assert lib.ndgpu_ovl_decode_batch(None, None, -1, 0, C.byref(recs), per, None, C.byref(st)) < 0 and not recs.value
    nullp = (P * 1)(None)
    assert lib.ndgpu_ovl_decode_batch(nullp, one, 1, 0, C.byref(recs), per, None, None) < 0 and not recs.value
    out = P()
    prev = np.asarray([3, 4], dtype=np.uint32)
    assert lib.ndgpu_ovl_encode_batch(None, 5, prev.ctypes.data, 0, C.byref(out), None) < 0 and not out.value and prev.tolist() == [3, 4]
    assert lib.ndgpu_ovl_encode_batch(None, -1, prev.ctypes.data, 0, C.byref(out), None) < 0 and not out.value
    img, bid, bk, nb, nbl = P(), P(), P(), C.c_uint64(9), C.c_int64(9)
    assert lib.ndgpu_ovl_sort_images(nullp, one, 1, None, 0, 0, 40, 300, 0, 0, C.byref(img), C.byref(nb), C.byref(bid), C.byref(bk), C.byref(nbl),
                                     None, None) < 0
    assert not img.value and not bid.value and not bk.value and nb.value == 0 and nbl.value == 0
    r8, off, sd, npl = P(), P(), P(), C.c_int64(9)
    assert lib.ndgpu_admit_piles_image(None, 16, 10, 1, 1, 1, 1, None, 0, 0, C.byref(r8), C.byref(off), C.byref(sd), C.byref(npl), None, None) < 0
    assert not r8.value and not off.value and not sd.value and npl.value == 0
