"""The batched device POA on the MI355X: ndgpu_poa_batch (K13 of lq_kernels.hip under DeviceAligner::run_poa) against what the compiled
reference's poa_to_consensus returned (tests/golden/poa.npz, tests/golden/poa_device.npz: only the fixtures are read), against the
library's own host poa_to_consensus on random jobs (tests/test_host_engine.py::test_poa_golden pins that routine to the reference), and
the engine with its regions' POA problems on the device against the same engine with them on the host.  tests/test_simt_poa.py asks
the first of the interpreted kernels."""
import ctypes as C

import numpy as np
import pytest

import poa_util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return poa_util.fixtures()


def test_fixtures_in_one_call_shuffled_and_singly(native_lib, cases):
    from nextdenovo_amd import api
    want = [c[1] for c in cases]
    api.reset_stats()
    assert api.poa_batch([c[0] for c in cases]) == want
    st = api.stats()
    assert st["poa_jobs"] == len(cases) and st["poa_declined"] == 0 and st["poa_rounds"] == 5 and st["poa_launches"] >= 5, st
    assert st["poa_cells"] > 20_000_000   # (the 2 x 3,100 case alone is 9.6 M cells)
    perm = np.random.default_rng(5).permutation(len(cases))
    got = api.poa_batch([cases[i][0] for i in perm])
    assert [got[k] for k in np.argsort(perm)] == want
    api.reset_stats()
    assert [api.poa_batch([c[0]])[0] for c in cases] == want
    st = api.stats()
    assert st["poa_jobs"] == len(cases) and st["poa_declined"] == 0, st


@pytest.mark.parametrize("form", ["wave", "group"])
def test_each_kernel_form_forced(form):
    r = poa_util.child("native", "fixtures", NDGPU_POA_FORM=form)
    st = r["stats"]
    assert r["bad"] == [] and r["n"] >= 86, r["bad"]
    assert st["poa_declined"] == 0 and st["poa_launches"] == st["poa_rounds"] > 0, st   # one form: one launch a round


def test_fuzz_against_the_host_routine(native_lib):
    from nextdenovo_amd import api
    jobs = poa_util.fuzz_jobs(1500)
    assert {len(j) for j in jobs} == {2, 3, 4, 5, 6} and min(len(s) for j in jobs for s in j) == 1 and max(len(s) for j in jobs for s in j) == 600
    api.reset_stats()
    got = []
    for a in range(0, len(jobs), 500):
        got += api.poa_batch(jobs[a:a + 500])
    st = api.stats()
    assert st["poa_jobs"] == 1500 and st["poa_declined"] == 0, st
    bad = [i for i, j in enumerate(jobs) if got[i] != poa_util.host_poa(native_lib, j)]
    assert not bad, bad[:20]


def test_engine_with_its_poa_on_the_device_and_on_the_host():
    """The golden piles (ONT, CLR, HiFi, -fast, -s) through correct_batch: the regions' POA problems as device requests, the same with
    NDGPU_POA_HOST (the backend offers nothing: the engine computes them), and with every request declined by the budget hook."""
    dev = poa_util.child("native", "piles", NDGPU_POA_DEVICE="1")
    host = poa_util.child("native", "piles", NDGPU_POA_DEVICE="1", NDGPU_POA_HOST="1")
    dec = poa_util.child("native", "piles", NDGPU_POA_DEVICE="1", NDGPU_POA_BUDGET="0")
    assert dev["bad"] == [] and host["bad"] == [] and dec["bad"] == [], (dev["bad"], host["bad"], dec["bad"])
    assert dev["rec"] == host["rec"] == dec["rec"] and dev["groups"] >= 4   # length, float32 identity bits, bases
    assert dev["stats"]["poa_jobs"] > 0 and dev["stats"]["poa_declined"] == 0 and dev["stats"]["poa_launches"] > 0, dev["stats"]
    assert host["stats"]["poa_jobs"] == 0, host["stats"]
    assert dec["stats"]["poa_declined"] == dec["stats"]["poa_jobs"] == dev["stats"]["poa_jobs"], dec["stats"]


def test_empty_batch_and_a_job_outside_the_device_limits(native_lib):
    from nextdenovo_amd import api
    assert native_lib.ndgpu_poa_batch(None, 0, None) == 0
    rng = np.random.default_rng(11)
    long_one = poa_util.util.ASC[rng.integers(0, 4, 10500, dtype=np.uint8)].tobytes()   # beyond struct seq_'s 9,999 bases
    jobs = [[long_one[:300], long_one[5:290]], [long_one, long_one[:120]], [long_one[40:200]]]
    api.reset_stats()
    got = api.poa_batch(jobs)
    st = api.stats()
    assert st["poa_jobs"] == 3 and st["poa_declined"] == 1, st
    assert got[0] == poa_util.host_poa(native_lib, jobs[0])
    # the host path's bytes for the declined one: a second sequence that is a prefix of the first leaves the first as the consensus
    assert got[1] == long_one
    assert got[2] == jobs[2][0]   # (one sequence: nothing to align)
