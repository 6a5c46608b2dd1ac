"""The consensus words and low-quality windows of the main walk on the device (K20 cns_windows_kernel of msa_kernels.hip:
ndgpu_cns_windows_batch under DeviceAligner::run_cns, and inside DeviceAligner::run_main with NDGPU_CNS_DEVICE=1) on a machine
without a GPU: the library's own sources on the lane-accurate interpreter under tests/simt.  The batched entry against the engine's
host routine (cns_windows_host, csrc/nd_cns.h) and against the restatement of the reference's lines in cns_util.py; the engine
against what the compiled reference answered for whole piles.  The switches and the interpreter's lane order and wavefront schedule
are read once per process, so every variant is a child process.  tests/test_zz_gpu_cns_windows.py runs the same, and more, on the
MI355X."""
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cns_util
import util

N_FUZZ, MAX_ITEMS = 300, 400


def test_directed_cases_are_what_they_claim():
    cases = cns_util.check_directed()
    assert len(cases) == 29


def test_the_fuzz_set_takes_every_branch():
    """A condition on the inputs, computed by the restatement alone: every branch at least 20 times over the 300 walks."""
    walks = cns_util.fuzz_walks(N_FUZZ, MAX_ITEMS)
    tot = cns_util.branch_totals(walks)
    assert len(walks) == N_FUZZ and max(w[0].shape[0] for w in walks) <= MAX_ITEMS
    assert all(tot[k] >= 20 for k in cns_util.BRANCHES), tot
    assert sum(1 for w in walks if w[2] < 10000) == N_FUZZ // 4 and {w[2] for w in walks if w[2] < 10000} <= set(range(12, 41))


@pytest.mark.parametrize("env", [
    {},                                                       # the default schedule
    {"SIMT_LANES_DESCENDING": "1"},                           # lanes highest first: lane 0's stores run last
    {"SIMT_SCHEDULE": "7", "SIMT_LANES_DESCENDING": "1"},     # a random wavefront runs ahead
    {"SIMT_SCHEDULE": "1"},                                   # the lowest wavefront runs ahead
])
def test_batch_on_the_interpreter(env):
    """The directed cases and 300 fuzz walks in calls of 1, 7 and all: device == host=True == restatement.  The entry and the
    counters do not exist before this feature."""
    r = cns_util.child("simt", "batch", N_FUZZ, MAX_ITEMS, 0, "1,7,0", **env)
    st = r["stats"]
    assert r["n"] == N_FUZZ + 29 and r["bad_host"] == [] and r["bad_dev"] == {"1": [], "7": [], str(r["n"]): []}, r
    assert st["cns_jobs"] == 3 * r["n"] and st["cns_declined"] == 0 and st["cns_regions"] == 3 * r["regions"] > 600, st
    assert st["cns_launches"] == r["n"] + (r["n"] + 6) // 7 + 1 and st["cns_d2h_bytes"] > 0 and st["walk_d2h_bytes"] == 0, st


def test_batch_with_every_third_walk_declined():
    """NDGPU_CNS_DECLINE=3: the kernel leaves every third walk, the host routine answers for it -- the same results."""
    r = cns_util.child("simt", "batch", 60, MAX_ITEMS, 0, "0", NDGPU_CNS_DECLINE="3")
    st = r["stats"]
    assert r["bad_host"] == [] and r["bad_dev"] == {str(r["n"]): []}, r
    assert st["cns_declined"] == r["n"] // 3 and st["cns_jobs"] == r["n"] - r["n"] // 3, st


def test_argument_errors():
    r = cns_util.child("simt", "args")
    for flags in (0, 1):
        for what in ("cov0", "base6", "tpos-high", "tpos-neg"):
            assert r["%s/%d" % (what, flags)] == [-2, True], (what, flags, r)      # -2, nothing written
        for what in ("gap-any", "tpos-top", "empty-job"):
            assert r["%s/%d" % (what, flags)] == [0, False], (what, flags, r)
        assert r["n0/%d" % flags] == 0 and r["n-neg/%d" % flags] == -2, r
    assert r["py-empty"] is True and r["top-pos"] == (1 << 21) - 2


@pytest.fixture(scope="module")
def pile_runs():
    """The golden piles through correct_batch: with the switch, with the switch and every second pile declined, without."""
    envs = [dict(NDGPU_CNS_DEVICE="1", NDGPU_TRACE="1"), dict(NDGPU_CNS_DEVICE="1", NDGPU_CNS_DECLINE="2"), {}]
    with ThreadPoolExecutor(3) as ex:
        return list(ex.map(lambda e: cns_util.child("simt", "piles", "golden", **e), envs))


def test_engine_three_ways(pile_runs):
    dev, dec, plain = pile_runs
    assert dev["n"] == dec["n"] == plain["n"] == 16
    assert dev["bad"] == [] and dec["bad"] == [] and plain["bad"] == [], (dev["bad"], dec["bad"], plain["bad"])   # the reference's answers
    assert dev["rec"] == dec["rec"] == plain["rec"]       # length, float32 identity bits, bases
    raw = dev["raw"]
    assert raw["piles"] == 9 and raw["cns_jobs"] >= raw["expected"] > 0 and raw["cns_declined"] == 0 and raw["cns_launches"] > 0, raw
    assert raw["walk_d2h_bytes"] == 0 and 0 < raw["cns_d2h_bytes"] < plain["raw"]["walk_d2h_bytes"], (raw, plain["raw"])
    assert dev["stats"]["cns_jobs"] == raw["cns_jobs"] and len(dev["trace"]) > 0       # no HiFi or -fast pile takes the kernel
    assert dec["raw"]["cns_declined"] > 0 and dec["raw"]["cns_jobs"] > 0 and dec["raw"]["walk_d2h_bytes"] > 0, dec["raw"]
    st = plain["stats"]
    assert st["cns_jobs"] == st["cns_launches"] == st["cns_declined"] == st["cns_d2h_bytes"] == 0 and st["walk_d2h_bytes"] > 0, st


def test_stats_keys_stand_behind_backtrack_ms(native_lib):
    from nextdenovo_amd import api
    names = [f[0] for f in api.Stats._fields_]
    assert names[-7:] == ["cns_jobs", "cns_declined", "cns_launches", "cns_regions", "cns_ms", "cns_d2h_bytes", "walk_d2h_bytes"]   # the C ABI grows at its end


def test_host_routine_in_a_sanitizer_build(tmp_path):
    """cns_windows_host (csrc/nd_cns.h: what the host flag and the engine compute with) in a stand-alone program built with
    -fsanitize=address,undefined (tests/csrc/cns_windows_check.cpp), fed the directed cases and 40 fuzz walks with the restatement's
    answers as a binary file.  Host code only, nothing preloaded."""
    walks = [c[1] for c in cns_util.directed_cases()] + cns_util.fuzz_walks(40, MAX_ITEMS, seed=11)
    words = [len(walks)]
    for steps, min_cov, lq_max_len, ratio in walks:
        e = cns_util.restate(steps, min_cov, lq_max_len, ratio)
        words += [steps.shape[0], min_cov, lq_max_len] + [int(x) for x in steps.reshape(-1)]
        words += [e["len"], e["uncorrected_len"], e["lstrip"], e["rstrip"], e["lqseq_total_length"], len(e["regions"])]
        words += [int(x) for r in e["regions"] for x in r] + e["bases"]
    dump = tmp_path / "cns_cases.bin"
    dump.write_bytes(struct.pack("<%di" % len(words), *words))
    exe = str(tmp_path / "cns_windows_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(cns_util.ROOT, "nextdenovo_amd", "csrc"), "-o", exe,
                    os.path.join(cns_util.HERE, "csrc", "cns_windows_check.cpp")], check=True)
    out = subprocess.run([exe, str(dump)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "%d cases checked" % len(walks)
