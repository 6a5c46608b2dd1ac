"""Record sets (ndgpu_ovl_recset: the records of a map call left on the device) and K18, their stable split: map_dev against map,
the split against numpy's stable argsort, concat / upload / download, the sorts over sets, arrays and mixed lists against the sorts
over arrays, the stage with NDGPU_RECS_DEVICE=1 against the stage without, and what is left behind (nothing).  Every expected
value comes from calls that take host arrays, from numpy or from the golden files of tests/golden/stage.
tests/test_simt_recset.py runs the same bodies under the interpreter."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_overlap as GO  # noqa: E402
import test_gpu_ovlsort as GS  # noqa: E402
import test_zz_gpu_admit as GA  # noqa: E402

pytestmark = pytest.mark.gpu
STAGE = GS.STAGE
WAVE, TILE = 64, 512            # lanes of a wavefront; records of a split tile (kSplitIters x 64, csrc/ovlsort_kernels.hip)
N_IDS = 3000                    # of the hand-built records
JOBS = [("seed", "part", True), ("seed", "seed", False)]   # GS._device_raw's two jobs of the stage fixture
TH = GA.TH


def _sets():
    from nextdenovo_amd import overlap
    return {k: overlap.ReadSet.from_2bit(os.path.join(STAGE, "input.%s.001.2bit" % k)) for k in ("seed", "part")}


def _opt(dual):
    from nextdenovo_amd import overlap
    o = overlap.preset("ava-ont")
    if dual:
        o.no_dual = 0
    return o


def _stats():
    from nextdenovo_amd import overlap
    return overlap.recset_stats()


@contextlib.contextmanager
def _nothing_left():
    """Live pool memory and live sets after the block are what they were before it."""
    from nextdenovo_amd import overlap
    live0, sets0 = overlap.pool_bytes()[0], _stats()["sets_live"]
    yield
    assert _stats()["sets_live"] == sets0 == 0
    assert overlap.pool_bytes()[0] == live0


# ---------------------------------------------------------------- 1. map
def test_map_dev_equals_map_on_the_stage_fixture():
    from nextdenovo_amd import overlap
    rs = _sets()
    with _nothing_left():
        for t, q, dual in JOBS:
            with overlap.Index(_opt(dual), rs[t]) as ix:
                want = ix.map(rs[q], ix.mid_occ())
                with ix.map_dev(rs[q], ix.mid_occ()) as s:
                    assert len(s) == s.size == want.size > 500
                    got = s.download()
            assert got.dtype == overlap.REC and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("lanes", [1, 2])
def test_map_dev_in_several_batches(lanes, monkeypatch):
    from nextdenovo_amd import overlap
    rs = _sets()
    monkeypatch.delenv("NDGPU_OVL_BATCH_ANCHORS", raising=False)
    monkeypatch.delenv("NDGPU_OVL_LANES", raising=False)
    with overlap.Index(_opt(True), rs["seed"]) as ix:
        mid = ix.mid_occ()
        ix.reset_stats()
        want = ix.map(rs["part"], mid)
        anchors = ix.stats()["anchors"]
        assert anchors > 8 * 1024
        monkeypatch.setenv("NDGPU_OVL_BATCH_ANCHORS", str(anchors // 5))   # a batch closes before it passes this many
        monkeypatch.setenv("NDGPU_OVL_LANES", str(lanes))
        ix.reset_stats()
        d0 = _stats()["bytes_d2d"]
        with ix.map_dev(rs["part"], mid) as s:
            got = s.download()
        assert ix.stats()["batches"] >= 3
    assert got.tobytes() == want.tobytes() and want.size > 500
    assert _stats()["bytes_d2d"] - d0 == want.size * 32   # batch after batch, appended device to device


def test_map_dev_of_an_empty_query_set():
    from nextdenovo_amd import overlap
    rs = _sets()
    with _nothing_left():
        with overlap.Index(_opt(False), rs["seed"]) as ix:
            with ix.map_dev(rs["seed"].subset(0, 0), ix.mid_occ()) as s:
                assert len(s) == 0 and s.download().size == 0 and s.download().dtype == overlap.REC


def check_map_dev_mode3(n_reads=None):
    from nextdenovo_amd import overlap
    hs = overlap.ReadSet.from_2bit(os.path.join(GO.GOLD, "hseed.2bit"))
    if n_reads is not None:
        hs = hs.subset(0, n_reads)
    o = GO.dev_opt("ava-hifi", False, ("--mode", "3"))
    with overlap.Index(o, hs) as ix:
        want = ix.map(hs, ix.mid_occ())
        ix.reset_stats()
        with ix.map_dev(hs, ix.mid_occ()) as s:
            got = s.download()
        assert ix.stats()["ext_problems"] > 0
    assert want.size > 20 and got.tobytes() == want.tobytes()


def test_map_dev_mode3():
    """The inputs of tests/test_zz_gpu_mode3.py: the records are the extended ones."""
    check_map_dev_mode3()


def test_map_dev_refuses_step2_options():
    from nextdenovo_amd import overlap
    rs = _sets()
    with overlap.Index(_opt(False), rs["seed"]) as ix:
        o = _opt(False)
        o.step = 2
        n0 = _stats()["sets_made"]
        with pytest.raises(RuntimeError):
            ix.map_dev(rs["seed"], 50, opt=o)
        assert _stats()["sets_made"] == n0


# ---------------------------------------------------------------- 2. split
def _records(qnames):
    """Only qname matters; the other fields are a running number, so that order shows."""
    from nextdenovo_amd import overlap
    n = len(qnames)
    r = np.zeros(n, dtype=overlap.REC)
    r["qname"] = qnames
    for k, name in enumerate(("rev", "qs", "qe", "tname", "ts", "te", "match")):
        r[name] = np.arange(n, dtype=np.uint32) * 7 + k
    return r


def _ids_per_file(n_files, n_ids=N_IDS):
    """Read id x belongs to file x % n_files."""
    return [np.arange(f, n_ids, n_files, dtype=np.uint32) for f in range(n_files)]


def _numpy_cut(recs, ids_per_file, n_ids):
    file_of = np.zeros(n_ids, dtype=np.int64)
    for f, x in enumerate(ids_per_file):
        file_of[x] = f
    rf = file_of[recs["qname"]]
    order = np.argsort(rf, kind="stable")
    cut = np.searchsorted(rf[order], np.arange(len(ids_per_file) + 1))
    return [recs[order][cut[f]:cut[f + 1]] for f in range(len(ids_per_file))]


def _check_split(qnames, ids_per_file, n_ids=N_IDS):
    from nextdenovo_amd import overlap
    recs = _records(np.asarray(qnames, dtype=np.uint32))
    want = _numpy_cut(recs, ids_per_file, n_ids)
    with _nothing_left():
        with overlap.RecordSet.upload(recs) as rs:
            parts = overlap.split_set(rs, ids_per_file, n_ids)
            try:
                assert len(parts) == len(ids_per_file) and sum(len(p) for p in parts) == recs.size
                for f, (p, w) in enumerate(zip(parts, want)):
                    assert len(p) == w.size and p.download().tobytes() == w.tobytes(), f
                assert rs.download().tobytes() == recs.tobytes()   # (the input is read-only)
            finally:
                for p in parts:
                    p.close()
    return [w.size for w in want]


SPLIT_N = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1)
SPLIT_FILES = (1, 2, 3, 64, 256)


@pytest.mark.parametrize("n_files", SPLIT_FILES)
@pytest.mark.parametrize("n", SPLIT_N)
def test_split_sizes_around_the_wavefront_and_the_tile(n, n_files):
    rng = np.random.default_rng(n * 1000 + n_files)
    _check_split(rng.integers(0, N_IDS, n), _ids_per_file(n_files))


def _patterns():
    rng = np.random.default_rng(18)
    n = 2 * TILE + 70
    out = [("all in one file of three", np.full(n, 1) + 3 * rng.integers(0, 900, n), 3),      # qname % 3 == 1
           ("one file empty", rng.integers(0, 900, n) * 3 + rng.integers(0, 2, n) * 2, 3),     # qname % 3 in {0, 2}
           ("alternating runs, part-major", np.concatenate([np.full(300, f) + 2 * rng.integers(0, 1000, 300) for f in (0, 1, 0, 1, 0, 1)]), 2),
           ("a wavefront of 64 distinct files", np.concatenate([rng.permutation(64) + 64 * rng.integers(0, 40, 64) for _ in range(9)]), 64),
           ("random, 20000 records", rng.integers(0, N_IDS, 20000), 7),
           ("random, 20000 records, 256 files", rng.integers(0, N_IDS, 20000), 256)]
    return out


_PATTERNS = _patterns()


@pytest.mark.parametrize("case", _PATTERNS, ids=[c[0] for c in _PATTERNS])
def test_split_file_patterns(case):
    _name, qnames, n_files = case
    _check_split(qnames, _ids_per_file(n_files))


def test_the_split_cases_are_what_they_claim():
    """The n values straddle the wavefront and the kernel's tile (read from its source), and the patterns are the patterns."""
    src = open(os.path.join(os.path.dirname(HERE), "nextdenovo_amd", "csrc", "ovlsort_kernels.hip")).read()
    assert int(re.search(r"kSplitIters = (\d+);", src).group(1)) * WAVE == TILE
    assert int(re.search(r"kSplitMaxFiles = (\d+);", src).group(1)) == max(SPLIT_FILES) == 256
    assert {WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 0, 1} <= set(SPLIT_N)
    by = {c[0]: c for c in _PATTERNS}
    sizes = lambda name: [w.size for w in _numpy_cut(_records(np.asarray(by[name][1], dtype=np.uint32)), _ids_per_file(by[name][2]), N_IDS)]  # noqa: E731
    assert sizes("all in one file of three")[0] == sizes("all in one file of three")[2] == 0
    s = sizes("one file empty")
    assert s[1] == 0 and s[0] > 0 and s[2] > 0
    q = np.asarray(by["alternating runs, part-major"][1]) % 2
    assert q.size > 3 * TILE and np.flatnonzero(np.diff(q)).size == 5
    q = np.asarray(by["a wavefront of 64 distinct files"][1]) % 64
    assert q.size > TILE and all(np.unique(q[w:w + 64]).size == 64 for w in range(0, q.size, 64))
    assert min(sizes("random, 20000 records, 256 files")) > 0 and by["random, 20000 records"][1].size == 20000 > 30 * TILE


def _raw_split(recs, file_of, n_files):
    """ndgpu_ovl_recset_split itself -> (return value, sets made by the call)."""
    from nextdenovo_amd import overlap
    lib = overlap.load()
    file_of = np.ascontiguousarray(file_of, dtype=np.uint32)
    out = (C.c_void_p * max(1, n_files))()
    with overlap.RecordSet.upload(recs) as rs:
        made0 = _stats()["sets_made"]
        rc = lib.ndgpu_ovl_recset_split(rs._handle(), file_of.ctypes.data_as(C.c_void_p), file_of.size, n_files, out)
        made = _stats()["sets_made"] - made0
    for f in range(n_files):
        if out[f]:
            lib.ndgpu_ovl_recset_free(out[f])
    return int(rc), made, [bool(out[f]) for f in range(n_files)]


def test_split_refuses_records_that_belong_to_no_file():
    from nextdenovo_amd import overlap
    with _nothing_left():
        q = np.arange(700, dtype=np.uint32) % 100
        file_of = (np.arange(100) % 2).astype(np.uint32)
        assert _raw_split(_records(q), file_of, 2)[:2] == (0, 2)
        bad = q.copy()
        bad[TILE + 3] = 100                                    # qname >= n_ids
        assert _raw_split(_records(bad), file_of, 2) == (-2, 0, [False, False])
        hole = file_of.copy()
        hole[37] = 0xffffffff                                  # a read that is in no file
        assert _raw_split(_records(q), hole, 2) == (-2, 0, [False, False])
        with overlap.RecordSet.upload(_records(bad)) as rs:
            with pytest.raises(ValueError):
                overlap.split_set(rs, [np.arange(0, 100, 2), np.arange(1, 100, 2)], 100)


def test_split_of_more_than_256_files_is_the_callers():
    from nextdenovo_amd import overlap
    with _nothing_left():
        q = np.arange(900, dtype=np.uint32)
        assert _raw_split(_records(q), np.arange(900) % 257, 257)[:2] == (-4, 0)
        assert _raw_split(_records(q), np.arange(900) % 256, 256)[:2] == (0, 256)
        with overlap.RecordSet.upload(_records(q)) as rs:
            with pytest.raises(overlap.TooManyFiles):
                overlap.split_set(rs, _ids_per_file(257, 900), 900)


# ---------------------------------------------------------------- 3. concat, upload, download
@pytest.mark.parametrize("n", [0, 1, 65])
def test_upload_then_download_is_the_identity(n):
    from nextdenovo_amd import overlap
    recs = _records(np.arange(n, dtype=np.uint32))
    with _nothing_left():
        up0 = _stats()["bytes_uploaded"]
        with overlap.RecordSet.upload(recs) as rs:
            assert len(rs) == n and rs.download().tobytes() == recs.tobytes()
        assert _stats()["bytes_uploaded"] - up0 == n * 32


def test_concat_of_the_fixtures_sets_equals_concatenate():
    from nextdenovo_amd import overlap
    files, _sl, _mn = GA._stage_raw()
    with _nothing_left():
        sets = [overlap.RecordSet.upload(f) for f in files] + [overlap.RecordSet.upload(files[0][:0])]
        try:
            with overlap.concat_sets(sets) as c:
                assert c.download().tobytes() == np.concatenate(files).tobytes()
            with overlap.concat_sets([]) as c:
                assert len(c) == 0
            assert [s.download().tobytes() for s in sets[:2]] == [f.tobytes() for f in files]   # the inputs stay as they are
        finally:
            for s in sets:
                s.close()


# ---------------------------------------------------------------- 4. the sorts
def _forms(files):
    """The fixture's files as sets, as arrays and as a mixed list; the sets are the caller's to close."""
    from nextdenovo_amd import overlap
    sets = [overlap.RecordSet.upload(f) for f in files]
    return sets, {"sets": sets, "arrays": list(files), "mixed": [sets[0], files[1]]}


@pytest.mark.parametrize("hq", [False, True], ids=["plain", "H"])
def test_sorts_over_sets_arrays_and_mixed_lists(hq, monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.delenv("NDGPU_OVLSORT_PIECE_RECORDS", raising=False)
    monkeypatch.delenv("NDGPU_OVLSORT_RANGE_CANDIDATES", raising=False)
    files, sl, mn = GA._stage_raw()
    want_srt, want_bl, want_st = overlap.sort_overlaps(files, sl, mn, 40, 300, hq=hq)
    want = GA._fused(files, sl, mn, hq=hq, want_sorted=True)
    assert want[4].tobytes() == want_srt.tobytes() and want[3] == want_bl and want[2].size > 50
    if not hq:
        assert overlap.encode(want_srt, np.zeros(2, dtype=np.uint32)) == GS._golden("input.seed.001.sorted.ovl")
    with _nothing_left():
        sets, forms = _forms(files)
        try:
            for name, lst in forms.items():
                overlap.recset_stats(reset=True)
                srt, bl, st = overlap.sort_overlaps(lst, sl, mn, 40, 300, hq=hq)
                assert srt.tobytes() == want_srt.tobytes() and bl == want_bl, name
                assert {k: v for k, v in st.items() if k != "gpu_ms"} == {k: v for k, v in want_st.items() if k != "gpu_ms"}, name
                got = GA._fused(lst, sl, mn, hq=hq, want_sorted=True)
                GA._same(got[:3], want[:3])
                assert got[3] == want[3] and got[4].tobytes() == want_srt.tobytes(), name
                assert got[5]["admit"]["admitted"] == want[5]["admit"]["admitted"] and got[5]["sort"]["ranges"] == 1
                if not hq:
                    assert overlap.encode(got[4], np.zeros(2, dtype=np.uint32)) == GS._golden("input.seed.001.sorted.ovl")
                rst = _stats()
                if name == "sets":      # in core, with sets: no record crossed the bus on the way in
                    assert rst["bytes_uploaded"] == 0 and rst["sets_downloaded"] == 0 and rst["bytes_d2d"] == 2 * sum(f.size for f in files) * 32
                if name == "mixed":     # the array of a mixed list is uploaded as a set of the call, twice here
                    assert rst["bytes_uploaded"] == 2 * files[1].size * 32 and rst["sets_downloaded"] == 0
                if name == "arrays":    # today's path: no set is made
                    assert rst["sets_made"] == 0 and rst["bytes_d2d"] == 0
            # one set read by two successive sorts: both right (above: each set was read by four)
            a = overlap.sort_overlaps(sets, sl, mn, 40, 300, hq=hq)
            b = overlap.sort_overlaps(sets, sl, mn, 40, 300, hq=hq)
            assert a[0].tobytes() == b[0].tobytes() == want_srt.tobytes() and a[1] == b[1] == want_bl
            assert [s.download().tobytes() for s in sets] == [f.tobytes() for f in files]
        finally:
            for s in sets:
                s.close()


def test_sorts_over_sets_in_seed_ranges(monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.delenv("NDGPU_OVLSORT_PIECE_RECORDS", raising=False)
    monkeypatch.delenv("NDGPU_OVLSORT_RANGE_CANDIDATES", raising=False)
    files, sl, mn = GA._stage_raw()
    want_srt, want_bl, _ = overlap.sort_overlaps(files, sl, mn, 40, 300)
    want = GA._fused(files, sl, mn)
    monkeypatch.setenv("NDGPU_OVLSORT_PIECE_RECORDS", "257")
    monkeypatch.setenv("NDGPU_OVLSORT_RANGE_CANDIDATES", "900")
    with _nothing_left():
        sets, _ = _forms(files)
        try:
            overlap.recset_stats(reset=True)
            srt, bl, st = overlap.sort_overlaps(sets, sl, mn, 40, 300)
            assert srt.tobytes() == want_srt.tobytes() and bl == want_bl and st["ranges"] >= 3
            rst = _stats()
            assert rst["sets_downloaded"] == len(sets) and rst["bytes_downloaded"] == sum(f.size for f in files) * 32
            got = GA._fused(sets, sl, mn)
            GA._same(got[:3], want[:3])
            assert got[3] == want[3] and got[5]["sort"]["ranges"] >= 3
            assert _stats()["sets_downloaded"] == 2 * len(sets)
        finally:
            for s in sets:
                s.close()


# ---------------------------------------------------------------- 5. the stage
@pytest.mark.parametrize("admit", [False, True], ids=["host-admission", "device-admission"])
def test_shard_piles_with_and_without_the_device_records(admit, tmp_path, monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.setitem(overlap._recset_local, "budget", None)
    monkeypatch.delenv("NDGPU_RECS_DEVICE_BYTES", raising=False)
    if admit:
        monkeypatch.setenv("NDGPU_ADMIT_DEVICE", "1")
    else:
        monkeypatch.delenv("NDGPU_ADMIT_DEVICE", raising=False)
    with _nothing_left():
        sh, _files = GA._stage_shard(tmp_path)
        try:
            monkeypatch.delenv("NDGPU_RECS_DEVICE", raising=False)
            overlap.recset_stats(reset=True)
            a = sh.piles(0)
            assert _stats()["sets_made"] == 0                  # unset: no set anywhere
            monkeypatch.setenv("NDGPU_RECS_DEVICE", "1")
            b = sh.piles(0)
            rst = _stats()
        finally:
            sh.close()
    GA._same(b[:3], a[:3])
    assert a[3] == b[3] and a[2].size > 50
    assert rst["sets_made"] == 2 and rst["bytes_uploaded"] == 0 and rst["bytes_downloaded"] == 0 and rst["budget_fallbacks"] == 0
    monkeypatch.setitem(overlap._recset_local, "budget", None)


def _synth_shard(stage, synth, n_seed_files=2, backend=None):
    g = synth.make_genome(40000, seed=5, n_repeats=3, repeat_len=1500)
    rs = synth.simulate_reads(g, 12, "ont", seed=6, mu=7.9, sigma=0.5, min_len=500)
    words, off, lens = synth.pack_db(rs)
    return stage.Shard(words, off, lens, preset="ava-ont", seed_cutoff=2500, read_cutoff=500, n_seed_files=n_seed_files, sort_k=20, backend=backend)


def test_grouped_jobs_are_cut_on_the_device(monkeypatch):
    """Seed file 0 of two: its part job and the job against seed file 1 map against one index with one set of options, so they are one
    call, and the target splits into several -I parts: the call's records come back part-major (file 0, 1, 0, 1) and K18 cuts them."""
    from nextdenovo_amd import minimap2_nd, overlap, stage, synth
    monkeypatch.setitem(overlap._recset_local, "budget", None)
    monkeypatch.delenv("NDGPU_RECS_DEVICE_BYTES", raising=False)
    parts_of = minimap2_nd.index_parts
    monkeypatch.setattr(minimap2_nd, "index_parts", lambda lens_, batch: parts_of(lens_, 90000, 30000))
    outs = {}
    with _nothing_left():
        for mode in ("serial", "device"):
            if mode == "serial":
                monkeypatch.setenv("NDGPU_STAGE_SERIAL", "1")
                monkeypatch.delenv("NDGPU_RECS_DEVICE", raising=False)
            else:
                monkeypatch.delenv("NDGPU_STAGE_SERIAL")
                monkeypatch.setenv("NDGPU_RECS_DEVICE", "1")
            sh = _synth_shard(stage, synth)
            try:
                assert 100 < sh.lens.size < 1000 and len(sh.jobs_of(0)) > 2
                assert len(minimap2_nd.index_parts(sh.lens[sh.seed_ids[0]], 0)) > 1
                overlap.recset_stats(reset=True)
                got = sh.overlaps(0)
                if mode == "device":
                    assert all(isinstance(x, overlap.RecordSet) for x in got)
                    assert _stats()["split_calls"] >= 1 and sh.backend.calls < len(sh.jobs_of(0))
                    outs[mode] = [x.download() for x in got]
                    for x in got:
                        x.close()
                else:
                    assert sh.backend.calls == len(sh.jobs_of(0))
                    outs[mode] = got
            finally:
                sh.close()
    assert len(outs["serial"]) == len(outs["device"]) and sum(r.size for r in outs["serial"]) > 200
    for a, b in zip(outs["serial"], outs["device"]):
        assert a.size == b.size and a.tobytes() == b.tobytes()
    monkeypatch.setitem(overlap._recset_local, "budget", None)


def _run_stage(tmp_path, tag, keep=False):
    from nextdenovo_amd import correct_stage
    out = str(tmp_path / ("cns_" + tag))
    keep_dir = str(tmp_path / ("keep_" + tag))
    argv = ["-d", STAGE, "-x", "ava-ont", "-k", "40", "-r", "ont", "-min_len_seed", "1250", "-p", "4", "-o", out] + (["--keep", keep_dir] if keep else [])
    assert correct_stage.run(argv) == 0
    assert open(out + ".001.fasta", "rb").read() == GS._golden("cns.default.fasta", gz=True)
    assert open(out + ".001.fasta.idx", "rb").read() == GS._golden("cns.default.fasta.idx", gz=True)
    if keep:
        assert open(os.path.join(keep_dir, "input.seed.001.sorted.ovl"), "rb").read() == GS._golden("input.seed.001.sorted.ovl")
        assert open(os.path.join(keep_dir, "input.seed.001.sorted.ovl.bl"), "rb").read() == GS._golden("input.seed.001.sorted.ovl.bl")


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_fused_stage_with_the_device_records_writes_the_golden_files(keep, tmp_path, monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.setitem(overlap._recset_local, "budget", None)
    monkeypatch.delenv("NDGPU_RECS_DEVICE_BYTES", raising=False)
    monkeypatch.setenv("NDGPU_RECS_DEVICE", "1")
    if not keep:
        monkeypatch.setenv("NDGPU_ADMIT_DEVICE", "1")        # both switches: no record reaches the host between K5 and recs8
    overlap.recset_stats(reset=True)
    with _nothing_left():
        _run_stage(tmp_path, "dev", keep)
    rst = _stats()
    assert rst["sets_made"] == 2 and rst["budget_fallbacks"] == 0 and rst["bytes_uploaded"] == 0
    assert (rst["bytes_downloaded"] > 0) == keep               # --keep downloads a set to write its .ovl
    monkeypatch.setitem(overlap._recset_local, "budget", None)


def test_fused_stage_past_the_budget_falls_back_to_arrays(tmp_path, monkeypatch):
    from nextdenovo_amd import overlap
    monkeypatch.setitem(overlap._recset_local, "budget", None)
    monkeypatch.setenv("NDGPU_RECS_DEVICE_BYTES", "1")
    monkeypatch.setenv("NDGPU_RECS_DEVICE", "1")
    overlap.recset_stats(reset=True)
    with _nothing_left():
        _run_stage(tmp_path, "budget")
    rst = _stats()
    assert rst["budget_fallbacks"] == len(JOBS) == rst["sets_made"] and rst["bytes_d2d"] == 0
    monkeypatch.setitem(overlap._recset_local, "budget", None)


# ---------------------------------------------------------------- 6. lifetime
def test_close_twice_and_use_after_close():
    from nextdenovo_amd import overlap
    with _nothing_left():
        rs = overlap.RecordSet.upload(_records(np.arange(10, dtype=np.uint32)))
        assert _stats()["sets_live"] == 1 and overlap.pool_bytes()[0] >= 320
        rs.close()
        rs.close()
        for use in (rs.download, lambda: len(rs), lambda: overlap.concat_sets([rs]), lambda: overlap.split_set(rs, [np.arange(10)], 10),
                    lambda: overlap.sort_overlaps([rs], np.zeros(10, dtype=np.uint32), 0)):
            with pytest.raises(ValueError):
                use()
        with overlap.RecordSet.upload(_records(np.arange(3, dtype=np.uint32))) as r2:
            assert len(r2) == 3
        with pytest.raises(ValueError):
            len(r2)


def test_trim_leaves_a_live_set_alone():
    from nextdenovo_amd import overlap
    recs = _records(np.arange(1000, dtype=np.uint32))
    with _nothing_left():
        with overlap.RecordSet.upload(recs) as rs:
            live = overlap.pool_bytes()[0]
            overlap.trim()
            assert overlap.pool_bytes()[0] == live >= recs.size * 32 and rs.download().tobytes() == recs.tobytes()


def test_a_failed_sort_leaves_no_set_behind(tmp_path, monkeypatch):
    from nextdenovo_amd import overlap, stage
    monkeypatch.setitem(overlap._recset_local, "budget", None)
    monkeypatch.delenv("NDGPU_RECS_DEVICE_BYTES", raising=False)
    monkeypatch.delenv("NDGPU_ADMIT_DEVICE", raising=False)
    monkeypatch.setenv("NDGPU_RECS_DEVICE", "1")

    class FailingSort(stage.DeviceBackend):
        seen = None

        def sort(self, files, *a):
            FailingSort.seen = [type(f).__name__ for f in files]
            raise RuntimeError("injected")

    with _nothing_left():
        sh, _files = GA._stage_shard(tmp_path)
        try:
            sh.backend = FailingSort(sh.opt)
            with pytest.raises(RuntimeError, match="injected"):
                sh.piles(0)
            assert FailingSort.seen == ["RecordSet", "RecordSet"] and _stats()["sets_live"] == 0
            # a caller's list is the caller's: not closed by piles
            theirs = [overlap.RecordSet.upload(f) for f in _files]
            with pytest.raises(RuntimeError, match="injected"):
                sh.piles(0, files=theirs)
            assert [len(s) for s in theirs] == [f.size for f in _files]
            for s in theirs:
                s.close()
        finally:
            sh.close()
    monkeypatch.setitem(overlap._recset_local, "budget", None)


# ---------------------------------------------------------------- 7. the interface
NEW_NAMES = {"ndgpu_ovl_map_dev", "ndgpu_ovl_recset_size", "ndgpu_ovl_recset_download", "ndgpu_ovl_recset_upload", "ndgpu_ovl_recset_concat",
             "ndgpu_ovl_recset_split", "ndgpu_ovl_recset_free", "ndgpu_ovl_sort_sets", "ndgpu_ovl_sort_piles_sets", "ndgpu_ovl_recset_stats"}


def test_the_new_entry_points_are_exported_and_declared():
    from nextdenovo_amd import build, overlap
    out = subprocess.run(["nm", "-D", "--defined-only", build.OVL_LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NEW_NAMES <= names
    assert all(n.startswith(("ndgpu_", "__hip_cuid_")) or n == "ksw_extd2_sse" for n in names), sorted(names)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ndgpu_overlap.h")).read()
    assert all(n + "(" in header for n in NEW_NAMES) and "typedef struct ndgpu_ovl_recset ndgpu_ovl_recset;" in header
    for n in ("RecordSet", "concat_sets", "split_set", "recset_stats"):
        assert hasattr(overlap, n)
    assert hasattr(overlap.Index, "map_dev") and hasattr(overlap.RecordSet, "upload")
