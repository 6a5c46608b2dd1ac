"""Resident POA graphs on the MI355X: ndgpu_poa_batch_flags with bit 1 / NDGPU_POA_RESIDENT=1 (K19 of lq_kernels.hip under
DeviceAligner::run_poa's resident form) against what the compiled reference's poa_to_consensus returned (tests/golden/poa.npz,
poa_device.npz, poa_resident.npz: only the fixtures are read), against the library's own host poa_to_consensus on random jobs
(tests/test_host_engine.py::test_poa_golden pins that routine to the reference), and the engine with its regions' POA problems on the
resident path against the same engine with K13's rounds.  tests/test_simt_poa_resident.py asks the first of the interpreted kernels.

A condition of every run here but the over-bound problem: no problem is declined by the resident path and none reaches a loop bound
(poa_resident_jobs == poa_jobs, poa_resident_declined == 0).  The largest node bound below is 6,203 (poa_device.npz), of 65,535."""
import numpy as np
import pytest

import poa_resident_util as pr
import poa_util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return poa_util.fixtures() + pr.cases()


def test_fixtures_in_one_call_shuffled_and_singly(native_lib, cases):
    from nextdenovo_amd import api
    want = [c[1] for c in cases]
    assert max(pr.bound(c[0]) for c in cases) == 6203 and len(cases) == 135
    api.reset_stats()
    assert api.poa_batch([c[0] for c in cases], resident=True) == want
    st = api.stats()
    assert st["poa_jobs"] == st["poa_resident_jobs"] == len(cases) and st["poa_resident_declined"] == 0 and st["poa_declined"] == 0, st
    assert st["poa_rounds"] == 49 and st["poa_graph_launches"] == 2 + 2 * 49 and st["poa_graph_ms"] > 0 and st["poa_cells"] > 20_000_000, st
    perm = np.random.default_rng(5).permutation(len(cases))
    got = api.poa_batch([cases[i][0] for i in perm], resident=True)
    assert [got[k] for k in np.argsort(perm)] == want
    api.reset_stats()
    assert [api.poa_batch([c[0]], resident=True)[0] for c in cases] == want
    st = api.stats()
    assert st["poa_jobs"] == st["poa_resident_jobs"] == len(cases) and st["poa_resident_declined"] == 0 and st["poa_declined"] == 0, st


@pytest.mark.parametrize("form", ["wave", "group"])
def test_each_align_form_forced(form):
    r = poa_util.child("native", "fixtures", NDGPU_POA_FORM=form, NDGPU_POA_RESIDENT="1")
    st = r["stats"]
    assert r["bad"] == [] and r["n"] >= 86, r["bad"]
    assert st["poa_resident_jobs"] == st["poa_jobs"] == 2 * r["n"] and st["poa_resident_declined"] == 0 and st["poa_declined"] == 0, st
    assert st["poa_launches"] == st["poa_rounds"] > 0, st   # one form: one launch a round


def test_fuzz_resident_against_rounds_against_the_host_routine(native_lib):
    from nextdenovo_amd import api
    jobs = poa_util.fuzz_jobs(600) + [pr.many_sequences(64)]
    want = api.poa_batch(jobs, host=True)
    assert want[:600] == [poa_util.host_poa(native_lib, j) for j in jobs[:600]]
    api.reset_stats()
    res = api.poa_batch(jobs, resident=True)
    st_res = api.stats()
    api.reset_stats()
    rounds = api.poa_batch(jobs, resident=False)
    st_rounds = api.stats()
    bad = [i for i in range(len(jobs)) if not res[i] == rounds[i] == want[i]]
    assert not bad, bad[:20]
    assert st_res["poa_jobs"] == st_res["poa_resident_jobs"] == len(jobs) and st_res["poa_resident_declined"] == 0 and st_res["poa_declined"] == 0, st_res
    assert st_rounds["poa_jobs"] == len(jobs) and st_rounds["poa_resident_jobs"] == 0 and st_rounds["poa_graph_launches"] == 0, st_rounds
    assert 0 < st_res["poa_d2h_bytes"] < st_rounds["poa_d2h_bytes"] and 0 < st_res["poa_h2d_bytes"] < st_rounds["poa_h2d_bytes"], (st_res, st_rounds)


def test_a_problem_over_the_node_bound(native_lib):
    """7 x 9,999 bases of one letter: node bound 70,000 > 65,535 -- declined from the resident path, computed by K13's rounds in the
    same call, counted; the small problem beside it stays resident."""
    from nextdenovo_amd import api
    over = [c for c in pr.load() if pr.bound(c[0]) > pr.OVER_BOUND]
    small = pr.cases(20)[:1]
    assert len(over) == 1 and len(small) == 1
    api.reset_stats()
    got = api.poa_batch([over[0][0], small[0][0]], resident=True)
    st = api.stats()
    assert got == [over[0][1], small[0][1]]
    assert st["poa_jobs"] == 2 and st["poa_resident_jobs"] == 1 and st["poa_resident_declined"] == 1 and st["poa_declined"] == 0, st
    assert st["poa_rounds"] == 6 + 1 and st["poa_cells"] > 6 * 9_999 * 9_999, st


def test_engine_with_resident_graphs_and_with_rounds():
    res = poa_util.child("native", "piles", NDGPU_POA_DEVICE="1", NDGPU_POA_RESIDENT="1")
    dev = poa_util.child("native", "piles", NDGPU_POA_DEVICE="1")
    assert res["bad"] == [] and dev["bad"] == [], (res["bad"], dev["bad"])
    assert res["rec"] == dev["rec"] and res["groups"] >= 4   # length, float32 identity bits, bases
    st = res["stats"]
    assert st["poa_jobs"] == dev["stats"]["poa_jobs"] > 0 and st["poa_resident_jobs"] == st["poa_jobs"], (st, dev["stats"])
    assert st["poa_resident_declined"] == 0 and st["poa_declined"] == 0 and st["poa_graph_launches"] > 0, st
    assert dev["stats"]["poa_resident_jobs"] == 0 and dev["stats"]["poa_graph_launches"] == 0, dev["stats"]


def test_empty_batch_and_flags(native_lib):
    from nextdenovo_amd import api
    assert native_lib.ndgpu_poa_batch_flags(None, 0, 2, None) == 0
    assert native_lib.ndgpu_poa_batch_flags(None, 0, 6, None) == -2 and native_lib.ndgpu_poa_batch_flags(None, 0, 8, None) == -2
    assert api.poa_batch([], resident=True) == []
    assert api.poa_batch([[b"ACGTN"]], resident=True) == [b"ACGTN"]   # one sequence: nothing to align
