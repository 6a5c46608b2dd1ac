"""K16, the pile admission on the device (ndgpu_admit_piles, ndgpu_ovl_sort_piles): exact equality of recs8 / pile_off / seeds with the
host routine overlap.assemble_piles -- and, on the stage fixture, with the line-by-line loop nextcorrect.assemble_piles -- on the
fixture, on random streams (regular and irregular), on hand-built chunk / table / threshold edges, on streams that must decline,
through the fused sort + admission call and through the stage.  tests/test_simt_admit.py runs the same bodies under the interpreter."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_ovlsort as GS  # noqa: E402

pytestmark = pytest.mark.gpu
STAGE = GS.STAGE
FORCED_TABLE = "8"   # NDGPU_ADMIT_TABLE: groups of more than 4 records take the table in global memory
N_IDS = 4000         # of the hand-built streams


def _same(got, want):
    assert got[2].tolist() == want[2].tolist()
    assert got[1].tolist() == want[1].tolist()
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64 and got[2].dtype == np.uint32


def _rows(rows):
    from nextdenovo_amd import overlap
    return overlap.from_decoded(np.asarray(rows, dtype=np.uint32).reshape(-1, 8))


def _check(recs, n_ids, th, skip=(), monkeypatch=None, forced=False):
    """admit_piles == assemble_piles on one stream; returns the admission's stats."""
    from nextdenovo_amd import overlap
    if monkeypatch is not None:
        if forced:
            monkeypatch.setenv("NDGPU_ADMIT_TABLE", FORCED_TABLE)
        else:
            monkeypatch.delenv("NDGPU_ADMIT_TABLE", raising=False)
    want = overlap.assemble_piles(recs, n_ids, *th, sorted(skip))
    got = overlap.admit_piles(recs, n_ids, *th, sorted(skip))
    _same(got[:3], want)
    st = got[3]
    assert st["sorted_records"] == recs.size and st["admitted"] == want[0].shape[0] and st["piles"] == want[2].size
    return st


# ---------------------------------------------------------------- 1. the stage fixture
_FIXTURE = {}


def _fixture_cases():
    """The eight cases of test_native_pile_assembly_equals_the_reference_loop with the loop's answer, computed once."""
    if _FIXTURE:
        return _FIXTURE["cases"], _FIXTURE["n_ids"]
    from nextdenovo_amd import nextcorrect as nc, ovl
    recs = ovl.decode_ovl(os.path.join(STAGE, "input.seed.001.sorted.ovl"))
    dup = np.concatenate([recs[:40], recs[5:12], recs[40:]])
    dup = dup[np.argsort(dup[:, 0], kind="stable")]
    rng = np.random.default_rng(3)
    noisy = recs.copy()
    cut = rng.random(noisy.shape[0]) < 0.2
    noisy[cut, 3] = noisy[cut, 2] + rng.integers(0, 600, int(cut.sum())).astype(noisy.dtype)
    n_ids = int(max(recs[:, 0].max(), recs[:, 4].max())) + 1
    args = nc.build_parser().parse_args(["-f", "x", "-i", "y", "-r", "ont"])
    cases = []
    for r, th, skip in [(recs, (1250, 500, 130, 10), set()), (recs, (3000, 900, 4, 2), {3, 5, 40}), (recs, (0, 500, 1, 1), set()),
                        (dup, (1250, 500, 130, 10), set()), (noisy, (1250, 500, 130, 10), {7}), (noisy, (1, 1, 2, 0), set()),
                        (recs[:0], (1250, 500, 130, 10), set()), (recs[:1], (1, 1, 130, 0), set())]:
        args.min_len_seed, args.min_len_aln, args.max_cov_aln, args.min_cov_seed = th
        loop = list(nc.assemble_piles(r, args, skip))
        cases.append((r, th, skip, loop))
    _FIXTURE["cases"], _FIXTURE["n_ids"] = cases, n_ids
    return cases, n_ids


def test_stage_fixture_equals_the_host_routine_and_the_loop():
    """3,473 records, 143 groups of 6 to 61: the eight threshold / input cases; no group is irregular on the unmodified records."""
    cases, n_ids = _fixture_cases()
    assert cases[0][0].shape[0] == 3473
    for k, (r, th, skip, loop) in enumerate(cases):
        from nextdenovo_amd import overlap
        st = _check(overlap.from_decoded(r), n_ids, th, skip)
        got = overlap.admit_piles(overlap.from_decoded(r), n_ids, *th, sorted(skip))
        assert [s for s, _ in loop] == got[2].tolist(), k
        assert got[1].tolist() == np.r_[0, np.cumsum([len(x) for _, x in loop])].astype(np.int64).tolist(), k
        rows = np.concatenate([np.asarray(x, dtype=np.int64) for _, x in loop]) if loop else np.zeros(0, dtype=np.int64)
        assert np.array_equal(got[0], r[rows].astype(np.uint32).reshape(-1, 8)), k
        if k < 3:
            assert st["groups_declined"] == 0 and st["groups"] == 143, (k, st)


# ---------------------------------------------------------------- 2. random streams
def test_random_record_streams_regular_and_irregular():
    """The generator of test_native_pile_assembly_on_random_record_streams (seed 77, 60 trials x 2 threshold sets): equal in all 120
    cases, some of them declined (missing self records, out-of-range query ids), most of them not."""
    rng = np.random.default_rng(77)
    declined = clean = 0
    for trial in range(60):
        n_seeds = int(rng.integers(1, 12))
        rows = []
        for s in rng.permutation(40)[:n_seeds]:
            slen = int(rng.integers(200, 6000))
            if rng.random() < 0.9:
                rows.append([s, 0, 0, slen - 1, s, 0, slen - 1, 0])
            for _ in range(int(rng.integers(0, 25))):
                a = int(rng.integers(0, slen - 1))
                b = int(min(slen - 1, a + rng.integers(1, 1500)))
                qn = int(rng.integers(0, 45))
                rows.append([s, int(rng.integers(0, 2)), a, b, qn, 0, b - a, int(rng.integers(0, 500))])
        skip = set(int(x) for x in rng.integers(0, 40, int(rng.integers(0, 4))))
        for th in ((int(rng.integers(0, 3000)), int(rng.integers(0, 800)), int(rng.integers(1, 6)), int(rng.integers(0, 4))), (1, 1, 1000, 0)):
            st = _check(_rows(rows), 48, th, skip)
            declined += st["groups_declined"] > 0
            clean += st["groups_declined"] == 0
    assert declined + clean == 120 and declined > 0 and clean > 0, (declined, clean)


# ---------------------------------------------------------------- 3. chunk and table edges
def _self(seed, slen):
    return [seed, 0, 0, slen - 1, seed, 0, slen - 1, 0]


def _group(seed, slen, n, span=300, q0=1000):
    """A regular group of n records: the self record, then n - 1 overlaps of `span` bases from distinct query reads."""
    rows = [_self(seed, slen)]
    for j in range(1, n):
        a = (j * 7) % (slen - span)
        rows.append([seed, j & 1, a, a + span - 1, q0 + j, 5, 5 + span - 1, span - j % 50])
    return rows


def _spans(seed, slen, spans, q0=1000):
    """The self record, then one overlap per entry of `spans` (t_e - t_s + 1 = the entry), distinct query reads."""
    return [_self(seed, slen)] + [[seed, 0, 10, 10 + sp - 1, q0 + j, 0, sp - 1, 1] for j, sp in enumerate(spans)]


def _edge_streams():
    big = (600, 100, 100000, 1)   # min_len_seed, min_len_aln, max_cov_aln (no depth cut-off), min_cov_seed
    out = []
    # group sizes around the 64-record chunk
    for sizes in ((1, 2, 63, 64, 65), (66, 128, 129, 130), (201, 5)):
        rows = []
        for i, n in enumerate(sizes):
            rows += _group(3 + i, 600 + 2100 * i, n, q0=1000 + 300 * i)
        out.append(("sizes %s" % (sizes,), rows, big, ()))
    # a repeated query read: same chunk (lanes 10 and 40), different chunks (records 10 and 70; 63 and 64)
    for a, b in ((10, 40), (10, 70), (63, 64)):
        rows = _group(9, 4000, 100)
        rows[b][4] = rows[a][4]
        out.append(("repeat %d/%d" % (a, b), rows, big, ()))
    # ... whose first record fails min_len_aln, so that the second is the first occurrence
    for a, b in ((10, 40), (10, 70)):
        rows = _group(9, 4000, 100)
        rows[b][4] = rows[a][4]
        rows[a][3] = rows[a][2] + 99            # t_e - t_s = 99 < 100
        out.append(("short first of a repeat %d/%d" % (a, b), rows, big, ()))
    # the self record's own id as a later query read
    rows = _group(9, 4000, 80)
    rows[30][4] = rows[70][4] = 9
    out.append(("self id again", rows, big, ()))
    # the depth cut-off: seed of 1000 bases, max_cov_aln 2 -> a record is admitted while before <= 3000
    out.append(("cut-off met exactly", _spans(5, 1000, [500] * 8) + _group(6, 900, 3), (600, 100, 2, 1), ()))
    out.append(("cut-off one base past", _spans(5, 1000, [500, 500, 500, 501] + [500] * 4) + _group(6, 900, 3), (600, 100, 2, 1), ()))
    # ... at a chunk boundary (max_cov_aln 10 -> 15000): record 63 sees exactly 15000, record 64 -- the next chunk's first -- 15200
    out.append(("cut-off at record 63", _spans(5, 1000, [225] * 61 + [275] + [200] * 30), (600, 100, 10, 1), ()))
    out.append(("cut-off at record 64", _spans(5, 1000, [222] * 62 + [236] + [200] * 30), (600, 100, 10, 1), ()))
    out.append(("cut-off behind record 64", _spans(5, 1000, [222] * 62 + [237] + [200] * 30), (600, 100, 10, 1), ()))
    # the pile's own depth: total == min_cov_seed * seed_len exactly, and one base below; min_cov_seed = 0
    out.append(("pile kept exactly", _spans(5, 1000, [500] * 4) + _spans(6, 1000, [500, 500, 500, 499]) + _group(7, 800, 6), (600, 100, 100000, 3), ()))
    out.append(("min_cov_seed 0", _group(5, 700, 1) + _group(6, 9000, 70), (600, 100, 3, 0), ()))
    # every seed rejected: too short, or in the skip set
    out.append(("all rejected", _group(5, 700, 9) + _group(6, 800, 70) + _group(7, 9000, 5), (900, 100, 100000, 1), (7,)))
    # spans of 2^27 in a 40-record group: `before` passes 2^32 in front of the cut-off (36 x the seed)
    s27 = 1 << 27
    out.append(("before beyond 2^32", _spans(5, s27, [s27] * 39), (600, 100, 24, 1), ()))
    out.append(("before beyond 2^32, no cut-off", _spans(5, s27, [s27 - 3] * 39) + _group(6, 900, 3), (600, 100, 100000, 39), ()))
    return out


_EDGES = _edge_streams()


@pytest.mark.parametrize("forced", [False, True], ids=["lds", "forced-table"])
@pytest.mark.parametrize("case", _EDGES, ids=[c[0] for c in _EDGES])
def test_chunk_and_table_edges(case, forced, monkeypatch):
    _name, rows, th, skip = case
    st = _check(_rows(rows), N_IDS, th, skip, monkeypatch, forced)
    assert st["groups_declined"] == 0, st
    assert (st["groups_wide"] > 0) == forced, st


def test_the_edges_are_the_edges():
    """What the hand-built streams claim about themselves, checked on the host routine's answers."""
    from nextdenovo_amd import overlap
    by = {c[0]: c for c in _EDGES}

    def n_admitted(name, seed):
        _n, rows, th, skip = by[name]
        r, off, seeds = overlap.assemble_piles(_rows(rows), N_IDS, *th, sorted(skip))
        p = seeds.tolist().index(seed) if seed in seeds.tolist() else None
        return None if p is None else int(off[p + 1] - off[p])
    assert n_admitted("cut-off met exactly", 5) == 1 + 5 and n_admitted("cut-off one base past", 5) == 1 + 4
    assert n_admitted("cut-off at record 63", 5) == 64 and n_admitted("cut-off at record 64", 5) == 65
    assert n_admitted("cut-off behind record 64", 5) == 64
    assert n_admitted("pile kept exactly", 5) == 5 and n_admitted("pile kept exactly", 6) is None
    assert n_admitted("repeat 10/70", 9) == 99 and n_admitted("short first of a repeat 10/70", 9) == 99
    assert n_admitted("self id again", 9) == 78
    assert n_admitted("all rejected", 5) is None and n_admitted("all rejected", 6) is None and n_admitted("all rejected", 7) is None
    assert n_admitted("before beyond 2^32", 5) == 37 and n_admitted("before beyond 2^32, no cut-off", 5) == 40


# ---------------------------------------------------------------- 4. decline, on purpose
_DECLINE = [
    ("valid seed shorter than min_len_aln + 1", _group(4, 3000, 20) + _group(5, 300, 6, span=120) + _group(6, 2000, 70), (200, 500, 130, 0)),
    ("missing self record", _group(4, 3000, 20) + [[5, 0, 100, 450, 77, 0, 350, 9]] + _group(5, 2500, 70)[1:] + _group(6, 2000, 9), (600, 100, 130, 0)),
    ("query id >= n_ids", _group(4, 3000, 70)[:40] + [[4, 0, 10, 900, N_IDS, 0, 890, 9]] + _group(4, 3000, 70)[40:], (600, 100, 130, 0)),
    ("t_e < t_s", _group(4, 3000, 70)[:66] + [[4, 0, 900, 10, 77, 0, 890, 9]] + _group(4, 3000, 70)[66:], (600, 100, 130, 0)),
]


@pytest.mark.parametrize("case", _DECLINE, ids=[c[0] for c in _DECLINE])
def test_irregular_streams_decline_to_the_host_routine(case):
    _name, rows, th = case
    st = _check(_rows(rows), N_IDS, th)
    assert st["groups_declined"] >= 1, st


# ---------------------------------------------------------------- 5. the fused call
_RAW = {}


def _stage_raw():
    from nextdenovo_amd import overlap, ovl_sort
    key = id(overlap._lib)
    if key not in _RAW:
        _RAW.clear()
        files = GS._device_raw([("seed", "part", True), ("seed", "seed", False)])
        sl, mn = ovl_sort.read_idx(os.path.join(STAGE, ".input.seed.001.idx"))
        # seed_len over every read id of the stage (n_ids = its size, as stage.Shard passes it): zero = not a seed of this file
        n_all = 1 + max(int(max(f["qname"].max(), f["tname"].max())) for f in files)
        _RAW[key] = (files, np.concatenate([sl, np.zeros(max(0, n_all - sl.size), dtype=sl.dtype)]), mn)
    return _RAW[key]


TH = (1250, 500, 130, 10)


def _fused(files, sl, mn, hq=False, use_bl=True, skip=(), want_sorted=False):
    from nextdenovo_amd import overlap
    return overlap.sort_piles(files, sl, mn, 40, 300, hq=hq, min_len_seed=TH[0], min_len_aln=TH[1], max_cov_aln=TH[2], min_cov_seed=TH[3],
                              use_bl=use_bl, skip=skip, want_sorted=want_sorted)


def _two_calls(files, sl, mn, hq=False, use_bl=True, skip=()):
    from nextdenovo_amd import overlap
    srt, bl, _ = overlap.sort_overlaps(files, sl, mn, 40, 300, hq=hq)
    return overlap.assemble_piles(srt, sl.size, *TH, sorted(set(skip) | ({rid for rid, _ in bl} if use_bl else set()))), bl, srt


def test_sort_piles_equals_sort_then_assemble(monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.delenv("NDGPU_OVLSORT_PIECE_RECORDS", raising=False)
    monkeypatch.delenv("NDGPU_OVLSORT_RANGE_CANDIDATES", raising=False)
    files, sl, mn = _stage_raw()
    golden_bl = GS._golden("input.seed.001.sorted.ovl.bl")
    want, bl, srt = _two_calls(files, sl, mn)
    assert want[2].size > 50 and len(bl) > 0
    extra = [int(want[2][1]), int(want[2][7])]   # two seeds that have piles
    for use_bl, skip in ((True, ()), (False, ()), (True, extra)):
        w = want if (use_bl and not skip) else _two_calls(files, sl, mn, use_bl=use_bl, skip=skip)[0]
        got = _fused(files, sl, mn, use_bl=use_bl, skip=skip)
        _same(got[:3], w)
        assert "".join("%d %s\n" % x for x in got[3]).encode() == golden_bl and got[4] is None
        st = got[5]
        assert st["admit"]["groups_declined"] == 0 and st["admit"]["sorted_records"] == srt.size == st["sort"]["kept"]
        assert st["admit"]["admitted"] == w[0].shape[0] and st["sort"]["ranges"] == 1
        assert st["admit"]["bytes_downloaded"] < srt.size * 32   # the sorted records stayed where they were
    assert not set(extra) & set(_fused(files, sl, mn, skip=extra)[2].tolist())
    # the sorted records on request
    got = _fused(files, sl, mn, want_sorted=True)
    _same(got[:3], want)
    assert overlap.encode(got[4], np.zeros(2, dtype=np.uint32)) == GS._golden("input.seed.001.sorted.ovl")
    # the out-of-core sort: the ranges' piles one after the other
    monkeypatch.setenv("NDGPU_OVLSORT_PIECE_RECORDS", "257")
    monkeypatch.setenv("NDGPU_OVLSORT_RANGE_CANDIDATES", "900")
    got = _fused(files, sl, mn)
    _same(got[:3], want)
    assert got[5]["sort"]["ranges"] >= 3 and "".join("%d %s\n" % x for x in got[3]).encode() == golden_bl
    monkeypatch.delenv("NDGPU_OVLSORT_PIECE_RECORDS")
    monkeypatch.delenv("NDGPU_OVLSORT_RANGE_CANDIDATES")
    # the high-quality-read filter in front
    w_hq, bl_hq, _ = _two_calls(files, sl, mn, hq=True)
    got = _fused(files, sl, mn, hq=True)
    _same(got[:3], w_hq)
    assert got[3] == bl_hq


# ---------------------------------------------------------------- 6. the stage
def _stage_shard(tmp_path):
    from nextdenovo_amd import ovl, stage
    files, sl, _mn = _stage_raw()
    idxs = os.path.join(str(tmp_path), "idxs.fofn")
    with open(idxs, "w") as f:
        for n in sorted(os.listdir(STAGE)):
            if n.startswith(".input.") and n.endswith(".idx"):
                f.write(os.path.join(STAGE, n) + "\n")
    words, off, lens = ovl.load_read_db(idxs)
    sh = stage.Shard(words, off, lens, preset="ava-ont", seed_cutoff=2500, read_cutoff=0, n_seed_files=1, sort_k=40, min_len_seed=1250)
    sh.seed_ids = [np.flatnonzero(sl[:lens.size]).astype(np.uint32)]   # the fixture's own seed file
    return sh, files


def test_shard_piles_with_and_without_the_device_admission(tmp_path, monkeypatch):
    sh, files = _stage_shard(tmp_path)
    try:
        monkeypatch.delenv("NDGPU_ADMIT_DEVICE", raising=False)
        a = sh.piles(0, files=files)
        monkeypatch.setenv("NDGPU_ADMIT_DEVICE", "1")
        b = sh.piles(0, files=files)
    finally:
        sh.close()
    _same(b[:3], a[:3])
    assert a[3] == b[3] and a[2].size > 50
    assert sh.admit_stats["groups_declined"] == 0 and sh.admit_stats["piles"] == a[2].size


def test_fused_stage_with_the_device_admission_writes_the_golden_fasta(tmp_path, monkeypatch):
    from nextdenovo_amd import correct_stage
    monkeypatch.setenv("NDGPU_ADMIT_DEVICE", "1")
    out = str(tmp_path / "cns")
    assert correct_stage.run(["-d", STAGE, "-x", "ava-ont", "-k", "40", "-r", "ont", "-min_len_seed", "1250", "-p", "4", "-o", out]) == 0
    assert open(out + ".001.fasta", "rb").read() == GS._golden("cns.default.fasta", gz=True)
    assert open(out + ".001.fasta.idx", "rb").read() == GS._golden("cns.default.fasta.idx", gz=True)


# ---------------------------------------------------------------- 7. the interface
def test_interface_empty_input_and_the_host_flag():
    from nextdenovo_amd import overlap
    r, off, seeds, st = overlap.admit_piles(np.zeros(0, dtype=overlap.REC), 10, 1250)
    assert r.shape == (0, 8) and off.tolist() == [0] and seeds.size == 0 and st["groups"] == 0
    cases, n_ids = _fixture_cases()
    for r, th, skip, _loop in cases[:6]:
        recs = overlap.from_decoded(r)
        dev = overlap.admit_piles(recs, n_ids, *th, sorted(skip))
        host = overlap.admit_piles(recs, n_ids, *th, sorted(skip), flags=1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dev[:3], host[:3]))
        assert host[3]["groups"] == 0 and host[3]["k16_ms"] == 0 and host[3]["admitted"] == dev[3]["admitted"]
    # every seed rejected: no pile
    r, off, seeds, st = overlap.admit_piles(overlap.from_decoded(cases[0][0]), n_ids, 10 ** 6, 500, 130, 10)
    assert r.shape == (0, 8) and off.tolist() == [0] and seeds.size == 0 and st["groups_declined"] == 0 and st["groups"] == 143
