"""The phasing and ranking of HiFi candidates on the device (K22: hifi_phase_kernel and hifi_phase_rank_kernel of lq_kernels.hip under
DeviceAligner::run_phase -- ndgpu_hifi_phase_batch -- and behind K11 in DeviceAligner::run_extract with NDGPU_PHASE_DEVICE=1) on a
machine without a GPU: the library's own sources on the lane-accurate interpreter under tests/simt.  The batched entry against the
engine's host rule (hifi_phase_host of nd_phase.h) and against the restatement of the reference's lines in phase_util.py; the engine
with the switch and without on the HiFi piles of the fixtures, against what the compiled reference answered for them.  The switches and
the interpreter's lane order and wavefront schedule are read once per process, so every variant is a child process.
tests/test_zz_gpu_phase.py runs the same, and more, on the MI355X."""
import ctypes as C
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import phase_util as pu


@pytest.fixture(scope="module")
def piles():
    return pu.case_piles() + pu.fuzz_piles(300)


@pytest.fixture(scope="module")
def want(piles):
    return [pu.restate(*p) for p in piles]


def test_directed_piles_and_fuzz_set_reach_every_branch():
    """Each directed pile reaches the branches it is there for, and 300 fuzz piles reach every counter of the restatement 20 times."""
    cases = pu.check_directed()
    assert len(cases) >= 27
    fz = pu.fuzz_piles(300)
    assert len(fz) == 300 and all(1 <= len(p[1]) <= 12 and 1 <= p[0] <= 64 for p in fz)
    assert all(1 <= len(g[2]) <= 40 and all(len(s) <= 160 for s in g[2]) for p in fz for g in p[1])
    _, cnt = pu.fuzz_counters(fz)
    low = {b: cnt.get(b, 0) for b in pu.BRANCHES if cnt.get(b, 0) < 20}
    assert not low and set(cnt) <= set(pu.BRANCHES), (low, set(cnt) - set(pu.BRANCHES))


@pytest.mark.parametrize("call", [1, 7, 100000])
def test_host_rule_against_the_restatement(native_lib, piles, want, call):
    """flags bit 0 needs no device: the engine's own rule on the directed piles and the fuzz piles."""
    from nextdenovo_amd import api
    got = []
    for a in range(0, len(piles), call):
        got += api.hifi_phase_batch(piles[a:a + call], host=True)
    assert all(r["declined"] == 0 for r in got)
    bad = [i for i, (g, w) in enumerate(zip(pu.strip(got), want)) if g != w]
    assert not bad, bad[:20]


@pytest.mark.parametrize("env,call", [
    ({}, 100000),                               # the default schedule, one call
    ({"SIMT_LANES_DESCENDING": "1"}, 7),        # lanes highest first, calls of seven piles
    ({"SIMT_SCHEDULE": "7"}, 1),                # a random wavefront runs ahead, pile by pile
])
def test_phase_batch_on_the_interpreter(env, call):
    """The directed piles and 300 fuzz piles: device, host=True and the restatement give equal records."""
    r = pu.child("simt", "batch", 300, call, NDGPU_TRACE="1", **env)
    st = r["stats"]
    assert r["n"] >= 327 and r["bad_dev"] == [] and r["bad_host"] == [] and r["declined"] == 0, r
    launches = (r["n"] + call - 1) // call
    assert st["piles"] == r["n"] and st["regions"] == r["regions"] and st["kind"] == r["kinds"] and min(r["kinds"]) > 0, (st, r["kinds"])
    assert st["pass2_piles"] == r["pass2"] > 20 and st["tail_passes"] == r["tails"] > 20, st
    assert st["launches"] == launches == r["trace_lines"] and st["ms"] > 0 and st["declined"] == [0] * 5, (st, launches)
    assert st["d2h_record_bytes"] == 32 * r["n"] + 128 * r["regions"] and st["d2h_string_bytes"] == 0, st


def test_decline_hook():
    """NDGPU_PHASE_DECLINE=3: every third pile is left by the kernel and takes the host rule -- the same records."""
    r = pu.child("simt", "batch", 60, 100000, NDGPU_PHASE_DECLINE="3")
    assert r["bad_dev"] == [] and r["declined"] == r["n"] // 3 > 0, r
    assert r["stats"]["declined"] == [0, 0, 0, r["n"] // 3, 0] and r["stats"]["piles"] == r["n"] - r["n"] // 3, r["stats"]


def test_a_pile_above_the_read_capacity_is_declined():
    """2,049 aligned reads: over the LDS table's capacity (kPhaseReads of nd_device.h); the answer is the host rule's."""
    r = pu.child("simt", "capacity")
    assert r["declined"] == [0, 1, 0] and r["same"] and r["stats"]["declined"] == [1, 0, 0, 0, 0] and r["stats"]["piles"] == 2, r


def test_argument_errors(native_lib):
    from nextdenovo_amd import api
    seqs = (C.c_char_p * 41)(*[b"ACGTACGTAC"] * 41)
    lens = (C.c_uint16 * 41)(*[10] * 41)
    srcs = (C.c_uint16 * 41)(*range(41))
    res = (api.PhaseRegion * 4)()
    pls = (api.PhasePile * 2)()
    C.memset(res, 0x55, C.sizeof(res))
    C.memset(pls, 0x55, C.sizeof(pls))
    P = lambda t, a: C.cast(a, C.POINTER(t))

    def region(n_cand, s=seqs, l=lens, r=srcs):
        return api.PhaseRegionIn(10, 19, n_cand, 0, P(C.c_char_p, s) if s else None, P(C.c_uint16, l) if l else None,
                                 P(C.c_uint16, r) if r else None)

    good = (api.PhaseRegionIn * 1)(region(3))
    for bad_region, n_aligned in ((region(41), 64), (region(-1), 64), (region(3, s=None), 64), (region(3, l=None), 64),
                                  (region(3, r=None), 64), (region(5), 4)):      # (the last: source read 4 of 4 aligned reads)
        bad = (api.PhaseRegionIn * 1)(bad_region)
        jobs = (api.PhaseJob * 2)(api.PhaseJob(64, 1, good), api.PhaseJob(n_aligned, 1, bad))
        for flags in (0, 1):
            assert native_lib.ndgpu_hifi_phase_batch(jobs, 2, flags, res, pls) == -2
    jobs = (api.PhaseJob * 1)(api.PhaseJob(64, 1, None))
    for flags in (0, 1):
        assert native_lib.ndgpu_hifi_phase_batch(jobs, 1, flags, res, pls) == -2
        assert native_lib.ndgpu_hifi_phase_batch(None, 1, flags, res, pls) == -2
        assert native_lib.ndgpu_hifi_phase_batch(jobs, -1, flags, res, pls) == -2
    jobs = (api.PhaseJob * 1)(api.PhaseJob(64, 1, good))
    assert native_lib.ndgpu_hifi_phase_batch(jobs, 1, 1, None, pls) == -2 and native_lib.ndgpu_hifi_phase_batch(jobs, 1, 1, res, None) == -2
    assert bytes(res) == b"\x55" * C.sizeof(res) and bytes(pls) == b"\x55" * C.sizeof(pls)      # nothing written for those batches
    assert native_lib.ndgpu_hifi_phase_batch(None, 0, 0, None, None) == 0 and native_lib.ndgpu_hifi_phase_batch(None, 0, 1, None, None) == 0
    assert api.hifi_phase_batch([], host=True) == []
    with pytest.raises(ValueError):
        api.hifi_phase_batch([(4, [(10, 19, [b"ACGT"] * 41, list(range(41)))])], host=True)
    empty = api.hifi_phase_batch([(4, [])], host=True)       # a pile without regions
    assert empty == [dict(has_heter=0, pass2=0, declined=0, regions=[])]
    assert set(api.phase_stats()) >= {"piles", "regions", "kind", "declined", "launches", "ms", "d2h_record_bytes", "d2h_string_bytes"}


@pytest.fixture(scope="module")
def pile_runs():
    """The HiFi piles of piles.npz, edge_piles.npz and hifi_phase_piles.npz through correct_batch: with the switch, without it, with the
    switch and every other pile declined by the hook."""
    envs = [dict(NDGPU_PHASE_DEVICE="1", NDGPU_TRACE="1"), {}, dict(NDGPU_PHASE_DEVICE="1", NDGPU_PHASE_DECLINE="2")]
    with ThreadPoolExecutor(3) as ex:
        return list(ex.map(lambda e: pu.child("simt", "piles", "golden,edge,phase", "all", **e), envs))


def test_engine_with_the_switch_and_without(pile_runs):
    dev, plain, hook = pile_runs
    assert dev["n"] == plain["n"] == hook["n"] >= 3 + 38
    assert dev["bad"] == [] and plain["bad"] == [] and hook["bad"] == [], (dev["bad"], plain["bad"], hook["bad"])   # the reference's answers
    assert dev["rec"] == plain["rec"] == hook["rec"]    # length, float32 identity bits, bases
    st = dev["phase"]
    assert st["piles"] > 0 and st["regions"] > 0 and st["launches"] == dev["trace_lines"] > 0 and sum(st["declined"]) == 0, st
    assert st["d2h_record_bytes"] > 0 and st["d2h_string_bytes"] > 0, st
    # the engine applies records of every kind the fixtures reach: ranked with and without the tail pass, seeds in either case; the
    # second pass ran (no fixture pile reaches a dropped region: DESIGN.md)
    assert st["kind"][3] >= 40 and 3 <= st["tail_passes"] < st["kind"][3] and 0 < st["seed_lower"] < st["kind"][2] and st["pass2_piles"] >= 3, st
    assert plain["phase"]["launches"] == 0 and plain["phase"]["piles"] == 0, plain["phase"]
    assert hook["phase"]["declined"][3] > 0 and hook["phase"]["piles"] + hook["phase"]["declined"][3] == st["piles"], hook["phase"]


def test_host_rule_in_a_sanitizer_build(tmp_path, piles, want):
    """hifi_phase_host (csrc/nd_phase.h: what the host flag and the engine compute with) in a stand-alone program built with
    -fsanitize=address,undefined (tests/csrc/phase_check.cpp), fed the directed piles and 80 fuzz piles with the restatement's answers
    as a binary file.  Host code only, nothing preloaded."""
    n_dir = len(pu.case_piles())
    words = [n_dir + 80]
    for (n_aligned, regions), w in list(zip(piles, want))[:n_dir + 80]:
        words += [n_aligned, len(regions), w["has_heter"], w["pass2"]]
        for (start, end, seqs, src), g in zip(regions, w["regions"]):
            words += [start, end, len(seqs)]
            for s, r in zip(seqs, src):
                words += [r, len(s)] + list(s)
            words += [g["kind"], g["lower"], g["indexs"], g["tail"], g["n"], g["seed"], g["seed_pos"]] + g["perm"] + g["kscore"]
    dump = tmp_path / "phase_cases.bin"
    dump.write_bytes(struct.pack("<%di" % len(words), *words))
    exe = str(tmp_path / "phase_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(pu.ROOT, "nextdenovo_amd", "csrc"), "-o", exe,
                    os.path.join(pu.HERE, "csrc", "phase_check.cpp")], check=True)
    out = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "%d piles checked" % (n_dir + 80)


def test_hifi_phase_piles_fixture():
    piles = pu.load_phase_piles()
    assert os.path.getsize(os.path.join(pu.HERE, "golden", "hifi_phase_piles.npz")) <= 1 << 20
    assert len(piles) >= 38 and {p["read_type"] for p in piles} == {3} and {len(p["seqs"]) - 1 for p in piles} == {6, 9, 30}
    tags = [p["tag"] for p in piles]
    assert sum("/hap/" in t for t in tags) >= 9 and any("minority" in t for t in tags) and sum("/own/" in t for t in tags) >= 25
    assert all(p["exp_len"] > 4 for p in piles)


def test_hifi_phase_piles_through_the_host_engine(host_harness):
    """The fixture itself: the host engine (oracle aligner as backend, the host rule) gives the reference's recorded answers."""
    import util
    fn, fr = util.bind_correct(host_harness, "ndtest_correct", "ndtest_free")
    bad = [w for w in (util.edge_wrong(p, util.call_correct(fn, fr, p, **util.edge_args(p))) for p in pu.load_phase_piles()) if w]
    assert not bad, bad
