"""The splice of the pseudo-seeds into the consensus, its table of lower-case runs and the terminal SSR trim on the device (K24
splice_kernel of msa_kernels.hip: ndgpu_splice_batch under DeviceAligner::run_splice) on a machine without a GPU: the library's own
sources on the lane-accurate interpreter under tests/simt.  The batched entry against the host statement (splice_host,
ssr_trim_host of csrc/nd_splice.h) and against the restatement of the reference's lines in splice_util.py.  The interpreter's lane
order and wavefront schedule and the decline hook are read once per process, so every variant is a child process.
tests/test_zz_gpu_splice.py runs the same, and more, on the MI355X."""
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import splice_util as su

N_FUZZ, MAX_WORDS = 300, 3000
N_DIRECTED, N_GATE = 82, 925
RECORD = 48                                       # bytes of the fixed record a job brings down


def test_directed_cases_are_what_they_claim():
    cases = su.check_directed()
    assert len(cases) == N_DIRECTED
    fam = su.gate_family()
    assert len(fam) == N_GATE
    su.check_gate_family(fam)


def test_the_fuzz_set_takes_every_branch():
    """Conditions on the inputs, computed by the restatement alone: over the 300 jobs every branch counter at least 20 (but the one
    no input reaches: a string that begins in lower case closes or bumps slot 0, so `lq_i == 0` never meets a leading lower-case run,
    :1471-1478); at least 20 jobs are cut at the tenth slot inside a pseudo-seed and 20 on a base; at least 20 are trimmed at each end."""
    jobs = su.fuzz_jobs(N_FUZZ, MAX_WORDS)
    assert len(jobs) == N_FUZZ and max(w[0].shape[0] for w in jobs) <= MAX_WORDS
    tot, extra = su.branch_totals(jobs)
    assert tot.pop("raw_none_lead") == 0
    assert all(v >= 20 for v in tot.values()), tot
    assert all(v >= 20 for v in extra.values()), extra


SCHEDULES = [
    {},                                                       # the default schedule
    {"SIMT_LANES_DESCENDING": "1"},                           # lanes highest first: lane 0's stores run last
    {"SIMT_SCHEDULE": "7", "SIMT_LANES_DESCENDING": "1"},     # a random wavefront runs ahead
    {"SIMT_SCHEDULE": "1"},                                   # the lowest wavefront runs ahead
]


@pytest.fixture(scope="module")
def batch_runs():
    with ThreadPoolExecutor(4) as ex:
        return list(ex.map(lambda env: su.child("simt", "batch", N_FUZZ, MAX_WORDS, 1, "1,7,0", **env), SCHEDULES))


@pytest.mark.parametrize("sched", range(len(SCHEDULES)))
def test_batch_on_the_interpreter(batch_runs, sched):
    """The directed cases, the gate family (every 37th length above 1100, all below) and 300 fuzz jobs in calls of 1, 7 and all:
    device == host=True == restatement on every field, the float's bits and the bytes.  The entry and the counters do not exist
    before this feature."""
    r = batch_runs[sched]
    st = r["stats"]
    n = N_DIRECTED + N_GATE + N_FUZZ
    assert r["n"] == n and r["bad_host"] == [] and r["bad_dev"] == {"1": [], "7": [], str(n): []}, r
    assert st["jobs"] == 3 * n and st["declined"] == 0 and st["launches"] == n + (n + 6) // 7 + 1, st
    assert st["d2h_bytes"] == 3 * (RECORD * n + r["bytes"]), (st, r["bytes"])      # the fixed record a job and one byte a result base
    assert st["h2d_bytes"] > 0 and st["trimmed"] > 3 * 400 and st["ms"] > 0, st
    assert len(r["trace"]) == 0


def test_batch_with_every_third_job_declined():
    """NDGPU_SPLICE_DECLINE=3: the runtime leaves every third job, the host statement answers for it -- the same results."""
    r = su.child("simt", "batch", 60, 800, 0, "0", NDGPU_SPLICE_DECLINE="3", NDGPU_TRACE="1")
    st = r["stats"]
    assert r["bad_host"] == [] and r["bad_dev"] == {str(r["n"]): []}, r
    assert st["jobs"] == r["n"] and st["declined"] == r["n"] // 3 and st["launches"] == 1, st
    assert 0 < st["d2h_bytes"] < RECORD * r["n"] + r["bytes"], st
    assert len(r["trace"]) == 1 and ("splice %d jobs" % (r["n"] - r["n"] // 3)) in r["trace"][0], r["trace"]


def test_argument_errors():
    r = su.child("simt", "args")
    for flags in (0, 1):
        for what in ("strips-cross", "descending", "start-above-end", "null-words", "null-regions", "null-seed", "null-res", "null-seqs"):
            assert r["%s/%d" % (what, flags)] == [-2, True], (what, flags, r)      # -2, nothing written
        for what in ("ok", "ok-regions", "strips-meet", "descending-under-strip", "equal-positions", "null-words-empty", "null-seed-empty"):
            assert r["%s/%d" % (what, flags)] == [0, False], (what, flags, r)
        assert r["n0/%d" % flags] == 0 and r["n-neg/%d" % flags] == -2, r
    assert r["py-empty"] is True
    assert r["far"] == [True, True] and r["far-stats"]["jobs"] == 2 and r["far-stats"]["declined"] == 1, r


@pytest.fixture(scope="module")
def pile_runs():
    with ThreadPoolExecutor(5) as ex:
        return list(ex.map(lambda e: su.child("simt", "piles", "golden,edge,rank", **e), su.PILE_ENVS))


def test_engine_five_ways(pile_runs):
    """The engine on the piles of tests/golden/piles.npz, edge_piles.npz and rank_piles.npz with NDGPU_SPLICE_DEVICE=1: alone, beside
    every other opt-in, with every second job declined, on a backend without the entry, and unset.  All 180 piles equal the compiled
    reference's recorded answers; the splice counters are positive with the switch and zero without it."""
    su.check_pile_runs(pile_runs, 180)


def test_host_statement_in_a_sanitizer_build(tmp_path):
    """splice_host and ssr_trim_host (csrc/nd_splice.h: what the host flag and the engine compute with) in a stand-alone program built
    with -fsanitize=address,undefined (tests/csrc/splice_check.cpp), fed the directed cases and 40 fuzz jobs with the restatement's
    answers -- the table and the emitted string included -- as a binary file.  Host code only, nothing preloaded."""
    jobs = [w for k, w in su.directed_cases()] + su.fuzz_jobs(40, 1500, seed=11)
    words = [len(jobs)]
    for w in jobs:
        ws, lstrip, rstrip, regions, read_type = w
        e = su.restate(w)
        words += [ws.shape[0], lstrip, rstrip, read_type, len(regions)] + [int(x) for x in ws]
        for a, b, ln, sd in regions:
            words += [a, b, ln, len(sd)] + list(sd)
        idn = np.float32(e["identity"])
        words += [e["len"], e["lq_total_len"], -1 if np.isnan(idn) else int(idn.view(np.int32)), e["out_len"], e["lq_m"], e["hq_m"], e["lq_i"],
                  e["clip_s"], e["clip_e"], len(e["seq"])] + list(e["seq"])
        words += [v for s in e["table"] for v in s] + list(e["out"])
    dump = tmp_path / "splice_cases.bin"
    dump.write_bytes(struct.pack("<%di" % len(words), *[v - (1 << 32) if v >= 1 << 31 else v for v in words]))
    exe = str(tmp_path / "splice_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(su.ROOT, "nextdenovo_amd", "csrc"), "-o", exe,
                    os.path.join(su.HERE, "csrc", "splice_check.cpp")], check=True)
    out = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "%d cases checked" % len(jobs)
