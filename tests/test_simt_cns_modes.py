"""The HiFi and -fast forms of the loop behind the main walk on the device (K21 cns_walk_kernel of msa_kernels.hip:
ndgpu_cns_walk_batch under DeviceAligner::run_cns_walk, and inside DeviceAligner::run_main with NDGPU_CNS_HIFI=1 / NDGPU_CNS_FAST=1)
on a machine without a GPU: the library's own sources on the lane-accurate interpreter under tests/simt.  The batched entry against
the engine's host routines (cns_kmer_host, cns_fast_host of csrc/nd_cns.h) and against the restatements of the reference's lines in
cns_modes_util.py; the engine against what the compiled reference answered for whole piles.  The switches and the interpreter's lane
order and wavefront schedule are read once per process, so every variant is a child process.  tests/test_zz_gpu_cns_modes.py runs
the same, and more, on the MI355X."""
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import cns_modes_util as cm

N_FUZZ, MAX_ITEMS = 300, 1500
N_DIRECTED = {1: 30, 2: 34}


def test_directed_cases_are_what_they_claim():
    cases = cm.check_directed()
    assert len(cases) == sum(N_DIRECTED.values())
    assert sum(1 for w in cases.values() if w[4] == 1) == N_DIRECTED[1]


def test_the_fuzz_sets_take_every_branch():
    """Conditions on the inputs, computed by the restatements alone: over the 300 walks of each mode every branch counter at least
    20; at least 20 -fast walks truncate, at least 20 have no closed slot, at least 20 HiFi walks merge."""
    for mode, names in ((1, cm.K_BRANCHES), (2, cm.F_BRANCHES)):
        walks = cm.fuzz_walks(mode, N_FUZZ, MAX_ITEMS)
        assert len(walks) == N_FUZZ and max(w[0].shape[0] for w in walks) <= MAX_ITEMS
        tot, extra = cm.branch_totals(walks)
        assert all(tot[k] >= 20 for k in names), (mode, tot)
        if mode == 1:
            assert extra["merged"] >= 20, extra
        else:
            assert extra["truncated"] >= 20 and extra["no_closed"] >= 20, extra


SCHEDULES = [
    {},                                                       # the default schedule
    {"SIMT_LANES_DESCENDING": "1"},                           # lanes highest first: lane 0's stores run last
    {"SIMT_SCHEDULE": "7", "SIMT_LANES_DESCENDING": "1"},     # a random wavefront runs ahead
    {"SIMT_SCHEDULE": "1"},                                   # the lowest wavefront runs ahead
]


@pytest.fixture(scope="module")
def batch_runs():
    """Both modes under the four schedules of test_simt_cns_windows.py: eight child processes, side by side."""
    todo = [(mode, k) for mode in (1, 2) for k in range(len(SCHEDULES))]
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda mk: cm.child("simt", "batch", mk[0], N_FUZZ, MAX_ITEMS, "1,7,0", **SCHEDULES[mk[1]]), todo))
    return dict(zip(todo, res))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("sched", range(len(SCHEDULES)))
def test_batch_on_the_interpreter(batch_runs, mode, sched):
    """The directed cases and 300 fuzz walks of a mode in calls of 1, 7 and all: device == host=True == restatement.  The entry and
    the counters do not exist before this feature."""
    r = batch_runs[(mode, sched)]
    st, ms = r["stats"], r["mode_stats"]
    n = N_FUZZ + N_DIRECTED[mode]
    assert r["n"] == n and r["bad_host"] == [] and r["bad_dev"] == {"1": [], "7": [], str(n): []}, r
    launches = n + (n + 6) // 7 + 1
    if mode == 1:
        assert ms["hifi_jobs"] == 3 * n and ms["hifi_regions"] == 3 * r["regions"] > 600 and ms["fast_jobs"] == 0, ms
    else:
        assert ms["fast_jobs"] == 3 * n and ms["hifi_jobs"] == ms["hifi_regions"] == 0, ms
    assert ms["hifi_declined"] == ms["fast_declined"] == 0 and ms["launches"] == launches and ms["d2h_bytes"] > 0, ms
    assert st["cns_jobs"] == st["cns_launches"] == st["cns_d2h_bytes"] == st["walk_d2h_bytes"] == 0, st     # the raw form's counters stay its own
    assert len(r["trace"]) == 0


def test_mode_0_is_the_existing_entry():
    """K20's directed cases through mode 0, alone and interleaved with walks of the other modes: api.cns_windows_batch's answer."""
    r = cm.child("simt", "mode0")
    assert r["n"] == 29
    for host in ("False", "True"):
        assert r["res"][host] == dict(same=True, mixed_raw=True, mixed_other=True), r


@pytest.mark.parametrize("mode", [1, 2])
def test_batch_with_every_third_walk_declined(mode):
    """NDGPU_CNS_DECLINE=3: the kernel leaves every third walk, the host routine answers for it -- the same results."""
    r = cm.child("simt", "batch", mode, 60, 400, "0", NDGPU_CNS_DECLINE="3", NDGPU_TRACE="1")
    ms = r["mode_stats"]
    jobs, declined = ("hifi_jobs", "hifi_declined") if mode == 1 else ("fast_jobs", "fast_declined")
    assert r["bad_host"] == [] and r["bad_dev"] == {str(r["n"]): []}, r
    assert ms[declined] == r["n"] // 3 and ms[jobs] == r["n"] - r["n"] // 3, ms
    assert len(r["trace"]) == 1 and ("%d HiFi, %d -fast" % ((r["n"], 0) if mode == 1 else (0, r["n"]))) in r["trace"][0], r["trace"]


def test_argument_errors():
    r = cm.child("simt", "args")
    for flags in (0, 1):
        for what in ("mode3", "mode-neg", "hifi-null-seed", "hifi-short-seed", "cov0-0", "cov0-1", "cov0-2", "base6-0", "base6-1", "base6-2"):
            assert r["%s/%d" % (what, flags)] == [-2, True], (what, flags, r)      # -2, nothing written
        for what in ("hifi-seed-just-fits", "hifi-gap-outside-seed", "fast-null-seed", "ok-0", "ok-1", "ok-2", "empty-job-0", "empty-job-1",
                     "empty-job-2"):
            assert r["%s/%d" % (what, flags)] == [0, False], (what, flags, r)
        assert r["n0/%d" % flags] == 0 and r["n-neg/%d" % flags] == -2, r
    assert r["py-empty"] is True


@pytest.fixture(scope="module")
def pile_runs():
    """The golden piles through correct_batch: both switches on, on with every second walk declined, nothing set."""
    on = dict(NDGPU_CNS_HIFI="1", NDGPU_CNS_FAST="1")
    envs = [dict(on, NDGPU_TRACE="1"), dict(on, NDGPU_CNS_DECLINE="2"), {}]
    with ThreadPoolExecutor(3) as ex:
        return list(ex.map(lambda e: cm.child("simt", "piles", "golden", **e), envs))


def test_engine_three_ways(pile_runs):
    dev, dec, plain = pile_runs
    assert dev["n"] == dec["n"] == plain["n"] == 16
    assert dev["bad"] == [] and dec["bad"] == [] and plain["bad"] == [], (dev["bad"], dec["bad"], plain["bad"])   # the reference's answers
    assert dev["rec"] == dec["rec"] == plain["rec"]       # length, float32 identity bits, bases
    h, f, raw = dev["kinds"]["hifi"], dev["kinds"]["fast"], dev["kinds"]["raw"]
    assert h["piles"] == 5 and f["piles"] == 2 and raw["piles"] == 9
    assert h["hifi_jobs"] > 0 and h["fast_jobs"] == 0 and f["fast_jobs"] > 0 and f["hifi_jobs"] == 0, (h, f)
    for g, p in ((h, plain["kinds"]["hifi"]), (f, plain["kinds"]["fast"])):
        assert g["walk_d2h_bytes"] == 0 and 0 < g["d2h_bytes"] < p["walk_d2h_bytes"] and g["launches"] > 0, (g, p)
        assert g["hifi_declined"] == g["fast_declined"] == 0 and g["cns_jobs"] == 0, g
    assert raw["walk_d2h_bytes"] > 0 and raw["launches"] == raw["d2h_bytes"] == 0 and dev["stats"]["cns_jobs"] == 0, raw     # raw piles: the parent's way
    assert len(dev["trace"]) == h["launches"] + f["launches"]
    d = dec["kinds"]
    assert d["hifi"]["hifi_declined"] + d["fast"]["fast_declined"] > 0 and d["hifi"]["hifi_jobs"] + d["fast"]["fast_jobs"] > 0, d
    assert d["hifi"]["walk_d2h_bytes"] + d["fast"]["walk_d2h_bytes"] > 0, d
    assert all(v == 0 for v in plain["mode_stats"].values()), plain["mode_stats"]       # unset: every new counter 0
    assert all(plain["kinds"][k]["walk_d2h_bytes"] > 0 for k in ("hifi", "fast", "raw"))


def test_a_seed_with_an_n():
    """One golden HiFi pile with a seed base replaced by N, in the ASCII form: the device backend reports a pile with bytes outside
    ACGT as uncorrectable before any walk exists, so K21 never sees such a seed -- the same answer with the switch and without."""
    on = cm.child("simt", "seed-n", NDGPU_CNS_HIFI="1")
    off = cm.child("simt", "seed-n")
    assert len(on["out"]) == 1 and on["out"] == off["out"], (on, off)
    assert on["out"][0][0] != on["out"][0][1]                 # (the N changes the answer: the pile was really altered)
    assert on["mode_stats"]["hifi_jobs"] == 1 and on["mode_stats"]["hifi_declined"] == 0, on      # the unaltered pile took K21
    assert all(v == 0 for v in off["mode_stats"].values())


def test_host_routines_in_a_sanitizer_build(tmp_path):
    """cns_kmer_host and cns_fast_host (csrc/nd_cns.h: what the host flag and the engine compute with) in a stand-alone program built
    with -fsanitize=address,undefined (tests/csrc/cns_modes_check.cpp), fed the directed cases and 40 fuzz walks per mode with the
    restatements' answers as a binary file.  Host code only, nothing preloaded."""
    walks = [w for k, w in cm.directed_cases()] + cm.fuzz_walks(1, 40, 400, seed=11) + cm.fuzz_walks(2, 40, 400, seed=12)
    words = [len(walks)]
    for w in walks:
        steps, min_cov, lq_max_len, ratio, mode, seed = w
        e = cm.restate(w)
        words += [mode, steps.shape[0], min_cov] + [int(x) for x in steps.reshape(-1)]
        if mode == 1:
            words += [len(seed)] + list(seed)
            words += [e["len"], e["lqseq_total_length"], len(e["regions"])] + [int(x) for r in e["regions"] for x in r] + e["bases"]
        else:
            words += [e["len"], e["lq_total_len"], e["out_len"], len(e["seq"])] + list(e["seq"])
    dump = tmp_path / "cns_mode_cases.bin"
    dump.write_bytes(struct.pack("<%di" % len(words), *words))
    exe = str(tmp_path / "cns_modes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(cm.ROOT, "nextdenovo_amd", "csrc"), "-o", exe,
                    os.path.join(cm.HERE, "csrc", "cns_modes_check.cpp")], check=True)
    out = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "%d cases checked" % len(walks)
