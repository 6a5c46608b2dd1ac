"""Batched global alignment with the CIGARs built on the device (ndgpu_align_batch / ndgpu_align_db_batch: K7 / K8a under
DeviceAligner::align_batch_runs, then K15 aln_runs_kernel of ond_kernels.hip) on a machine without a GPU: the library's own sources on
the lane-accurate interpreter under tests/simt.  Expected records come from the reference alone (aln_util.py: the golden pairs and the
oracle, run-length-encoded with numpy).  The chunk hook and the interpreter's lane order and wavefront schedule are read once per
process, so every variant is a child process.  tests/test_zz_gpu_align_batch.py runs the same, and more, on the MI355X."""
import ctypes as C

import pytest

import aln_util

SMALL = 2000    # golden pairs with q_len + t_len <= 2,000: 26 of the 71
MEDIUM = 6500   # ... <= 6,500: 53 of them, the two aborts included (single align() calls are what is slow on the interpreter)


@pytest.mark.parametrize("env", [
    {},                                   # the default schedule
    {"SIMT_LANES_DESCENDING": "1"},       # lanes highest first
    {"SIMT_SCHEDULE": "7"},               # a random wavefront runs ahead
])
def test_align_batch_on_the_interpreter(oracle_lib, env):
    """The directed set and the small golden pairs in one call: device == host flag == expected, field by field and run by run."""
    r = aln_util.child("simt", "batch", SMALL, **env)
    st = r["stats"]
    assert r["n"] == 23 + 26 and r["bad_dev"] == [] and r["bad_host"] == [], r
    assert {0, 1} <= set(r["statuses"])
    assert st["aln_batch_jobs"] == r["n"] and st["aln_batch_runs"] == r["runs"] > 4000 and st["aln_batch_launches"] == 1, st
    assert st["aln_batch_ms"] > 0 and st["forward_launches"] == 1 and st["wide_tasks"] >= 1, st
    assert r["stats_after_host"]["aln_batch_jobs"] == r["n"]       # (the host flag counts nothing)


def test_the_same_jobs_in_chunks(oracle_lib):
    r = aln_util.child("simt", "batch", SMALL, NDGPU_ALIGN_CHUNK_JOBS="9")
    st = r["stats"]
    assert r["bad_dev"] == [] and r["bad_host"] == [], r
    assert st["forward_launches"] == (r["n"] + 8) // 9 >= 3 and 3 <= st["aln_batch_launches"] <= st["forward_launches"], st
    assert st["aln_batch_jobs"] == r["n"] and st["aln_batch_runs"] == r["runs"], st


def test_strings_flag_against_align(oracle_lib):
    """q_aln / t_aln, aln_len, aln_t_len and aln_q_len equal what align() / align_hq() of the same library write, for the directed set
    and the golden pairs up to 6,500 bases (cut by length alone; the two aborts are among them), with the device tail and with the
    host flag."""
    r = aln_util.child("simt", "strings", MEDIUM)
    assert r["n"] == 23 + 53 and r["bad"] == [] and r["aligned"] > 50 and r["aborts"] == 2, r


def test_db_form(oracle_lib):
    """Windows of a resident DB of 20 reads under all four (q_rev, t_rev): equal to the ASCII form on host copies of the same windows
    and to the oracle; a read or a window outside the DB is refused with nothing written."""
    r = aln_util.child("simt", "db")
    assert r["bad_db"] == [] and r["bad_ascii"] == [] and r["strings_differ"] == [], r
    assert r["revs"] == [[0, 0], [0, 1], [1, 0], [1, 1]] and r["aligned"] >= 12, r
    assert r["stats"]["pool_bases"] == 0 and r["stats"]["aln_batch_jobs"] == r["n"], r["stats"]     # nothing packed or uploaded
    assert all(rc < 0 and untouched for rc, untouched in r["rcs"]), r["rcs"]


def test_argument_errors_and_an_empty_batch(native_lib):
    from nextdenovo_amd import api
    f = native_lib.ndgpu_align_batch
    good = api.AlnJob(b"ACGTACGT", 8, b"ACGTACGT", 8, 0)
    res = (api.AlnResult * 2)()
    C.memset(res, 0x55, C.sizeof(res))
    cg, qa, ta = C.c_void_p(0x5555), C.c_void_p(0x5555), C.c_void_p(0x5555)
    for bad in (api.AlnJob(b"ACGT", -1, b"ACGT", 4, 0), api.AlnJob(b"ACGT", 4, b"ACGT", -4, 0), api.AlnJob(None, 4, b"ACGT", 4, 0),
                api.AlnJob(b"ACGT", 4, None, 4, 0)):
        jobs = (api.AlnJob * 2)(good, bad)
        for flags in (0, 1, 2, 3):
            assert f(jobs, 2, flags, res, C.byref(cg), C.byref(qa), C.byref(ta)) < 0
    jobs = (api.AlnJob * 2)(good, good)
    for flags in (0, 1):
        assert f(jobs, -1, flags, res, C.byref(cg), None, None) < 0
        assert f(None, 2, flags, res, C.byref(cg), None, None) < 0
        assert f(jobs, 2, flags, None, C.byref(cg), None, None) < 0
        assert f(jobs, 2, flags, res, None, None, None) < 0
        assert f(jobs, 2, flags | 2, res, C.byref(cg), None, C.byref(ta)) < 0       # the strings flag without a place for them
        assert f(jobs, 2, flags | 2, res, C.byref(cg), C.byref(qa), None) < 0
    g = native_lib.ndgpu_align_db_batch
    dbjobs = (api.AlnDbJob * 2)()
    assert g(None, dbjobs, 2, 0, res, C.byref(cg), None, None) < 0 and g(None, dbjobs, -1, 0, res, C.byref(cg), None, None) < 0
    assert bytes(res) == b"\x55" * C.sizeof(res) and cg.value == qa.value == ta.value == 0x5555      # nothing written
    for flags in (0, 1, 2, 3):
        assert f(None, 0, flags, None, None, None, None) == 0 and g(None, None, 0, flags, None, None, None, None) == 0
    assert api.align_batch([]) == [] and api.align_batch([], host=True, strings=True) == []
    assert api.cigar_string([5 << 4 | 7, 1 << 4 | 1, 300 << 4 | 2]) == "5=1I300D"
    st = api.stats()
    assert {"aln_batch_jobs", "aln_batch_launches", "aln_batch_runs", "aln_batch_ms"} <= set(st)
    assert list(st)[-4:] == ["aln_batch_jobs", "aln_batch_launches", "aln_batch_runs", "aln_batch_ms"]     # appended


def test_host_run_length_routine_under_sanitizers(oracle_lib, tmp_path):
    """aln_runs_host (csrc/nd_host.h: what the host flag reports from) in a stand-alone program built with
    -fsanitize=address,undefined (tests/csrc/aln_runs_check.cpp), fed the golden pairs' and the directed set's column kinds from
    exact-size heap blocks: equal to the numpy run-length encoding, and no report from either sanitizer."""
    import os
    import struct
    import subprocess
    import numpy as np
    import util
    exe = str(tmp_path / "aln_runs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(aln_util.ROOT, "nextdenovo_amd", "csrc"), "-o", exe,
                    os.path.join(aln_util.HERE, "csrc", "aln_runs_check.cpp")], check=True)
    streams = [np.asarray(p["ops"], dtype=np.uint8) for p in util.load_pairs()]
    streams += [util.strings_to_ops(*util.oracle_align(oracle_lib, q, t, hq)[1:3]) for _, q, t, hq in aln_util.directed_jobs()]
    streams += [np.zeros(0, np.uint8), np.array([2], np.uint8), np.array([1, 1, 0], np.uint8)]
    data = b"".join(struct.pack("<I", s.size) + s.tobytes() for s in streams)
    out = subprocess.run([exe], input=data, capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stderr == b"", out.stderr[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == len(streams) and sum(s.size for s in streams) > 180000
    for s, ln in zip(streams, lines):
        got = [int(x) for x in ln.split()]
        e = aln_util.expect(1, 0, 0, s)
        assert got[:6] == [e["cigar"].size, e["n_match"], e["n_ins"], e["n_del"], e["max_gap_run"], s.size] and got[6:] == e["cigar"].tolist()
