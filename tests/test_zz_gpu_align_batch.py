"""Batched global alignment with the CIGARs built on the MI355X: ndgpu_align_batch / ndgpu_align_db_batch (K7 / K8a under
DeviceAligner::align_batch_runs, K15 aln_runs_kernel of ond_kernels.hip) against the reference's answers -- the golden pairs and the
oracle, run-length-encoded with numpy in aln_util.py; only fixtures are read.  tests/test_simt_align_batch.py asks the same of the
interpreted kernels."""
import numpy as np
import pytest

import aln_util
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(oracle_lib):
    """The directed set + all 71 golden pairs with their expected records; computed once, never changed."""
    jobs, exp = aln_util.check_directed(oracle_lib)
    gj, ge = aln_util.golden_jobs(oracle_lib)
    aln_util.check_golden(ge)
    return jobs + gj, exp + ge


def test_golden_and_directed_in_one_call(native_lib, case):
    from nextdenovo_amd import api
    jobs, exp = case
    api.reset_stats()
    dev = api.align_batch(jobs)
    st = api.stats()
    host = api.align_batch(jobs, host=True)
    assert aln_util.diff(dev, exp) == [] and aln_util.diff(host, exp) == []
    assert st["wide_tasks"] >= 1 and st["max_band"] > 253, st
    assert st["aln_batch_jobs"] == len(jobs) and st["aln_batch_runs"] == sum(e["cigar"].size for e in exp), st
    assert st["aln_batch_launches"] == st["forward_launches"] == 1 and st["aln_batch_ms"] > 0, st
    assert api.stats()["aln_batch_jobs"] == len(jobs)      # (the host flag counts nothing)


def test_fuzz_against_the_oracle(native_lib, oracle_lib):
    """250 pairs of test_align_fuzz_vs_oracle's generator in calls of 100: status, aln_len, q_used, t_used, counts and runs."""
    from nextdenovo_amd import api
    pairs = aln_util.fuzz_pairs(250)
    exp = [aln_util.oracle_expect(oracle_lib, *p) for p in pairs]
    got = []
    for a in range(0, len(pairs), 100):
        got += api.align_batch(pairs[a:a + 100])
    assert aln_util.diff(got, exp) == []
    assert sum(1 for e in exp if e["status"] == 1) > 120


def test_order_and_singles(native_lib, case):
    from nextdenovo_amd import api
    jobs, exp = case
    perm = np.random.default_rng(5).permutation(len(jobs))
    got = api.align_batch([jobs[i] for i in perm])
    assert aln_util.diff([got[k] for k in np.argsort(perm)], exp) == []
    some = list(range(0, len(jobs), 5))
    assert aln_util.diff([api.align_batch([jobs[i]])[0] for i in some], [exp[i] for i in some]) == []


def test_forced_chunks(oracle_lib):
    r = aln_util.child("native", "order", NDGPU_ALIGN_CHUNK_JOBS="11")
    st = r["stats"]
    assert r["n"] == 94 and r["bad_dev"] == [], r
    assert st["forward_launches"] == 9 and 3 <= st["aln_batch_launches"] <= 9 and st["aln_batch_jobs"] == 94, st


def test_strings_flag_against_align(native_lib, oracle_lib):
    from nextdenovo_amd import api
    jobs, _ = aln_util.golden_jobs(oracle_lib)
    for host in (False, True):
        got = api.align_batch(jobs, strings=True, host=host)
        for i, ((q, t, hq), g) in enumerate(zip(jobs, got)):
            n, tu, qu, ts, qs = util.gpu_align(native_lib, q, t, hq)
            assert (n, tu, qu, ts, qs) == (g["aln_len"], g["t_used"], g["q_used"], g["t_aln"], g["q_aln"]), (host, i)


def test_db_form(oracle_lib):
    r = aln_util.child("native", "db")
    assert r["bad_db"] == [] and r["bad_ascii"] == [] and r["strings_differ"] == [], r
    assert r["revs"] == [[0, 0], [0, 1], [1, 0], [1, 1]] and r["aligned"] >= 12, r
    assert r["stats"]["pool_bases"] == 0 and r["stats"]["aln_batch_jobs"] == r["n"], r["stats"]
    assert all(rc < 0 and untouched for rc, untouched in r["rcs"]), r["rcs"]
