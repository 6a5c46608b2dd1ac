"""Resident POA graphs (K19: the poa_graph_* kernels of lq_kernels.hip under DeviceAligner::run_poa's resident form) on a machine
without a GPU: the library's own sources on the lane-accurate interpreter under tests/simt, against what the compiled reference's
poa_to_consensus returned (tests/golden/poa.npz, poa_device.npz, poa_resident.npz).  Cases up to 300 bases a sequence: the interpreter is
slow, and tests/test_zz_gpu_poa_resident.py runs the long ones.  NDGPU_POA_RESIDENT, the kernel form, the budget and the interpreter's
lane order and wavefront schedule are read once per process, so every variant is a child process.

A condition of every run here but the forced-budget ones: no problem is declined by the resident path and none reaches a loop bound
(poa_resident_jobs == poa_jobs, poa_resident_declined == 0).  The largest node bound among these cases is 50 x 41 = 2,050, of
65,535."""
import pytest

import poa_resident_util as pr
import poa_util

MAX_LEN = 300


def test_fixture_holds_the_directed_cases():
    fx = pr.load()
    seqs = [c[0] for c in fx]
    assert len(fx) == 50 and all(len(c[1]) > 0 for c in fx)
    for n in range(2, 7):
        for L in (1, 2, 3):
            assert any(len(s) == n and len(set(s)) == 1 and len(s[0]) == L for s in seqs)                   # equal
            assert any(len(s) == n and len(set(s)) == n and {len(x) for x in s} == {L} for s in seqs)       # all different
    assert any(len(s) == 6 and all(len(set(x)) == 1 for x in s) and len(set(b"".join(s))) == 6 for s in seqs)   # six single letters
    assert set(b"".join(b"".join(s) for s in seqs)) >= set(b"ACGTNR")
    for L in (5, 70):
        assert any(len(s[0]) == L and s[0].startswith(s[1]) and s[0] != s[1] for s in seqs)                 # a strict prefix
        assert any(len(s[0]) == L and s[0].endswith(s[1]) and s[0] != s[1] for s in seqs)                   # a strict suffix
    assert any(len(s) == 3 and len(set(s)) == 1 for s in seqs) and any(len(s) == 6 and len(set(s)) == 1 and len(s[0]) > 3 for s in seqs)
    assert {63, 64, 65, 128, 129} <= {len(s[0]) for s in seqs if len(s) == 2}
    assert any(len(s[1]) == len(s[0]) + 20 and s[1].endswith(s[0]) for s in seqs)                           # an insertion at the front
    assert any(len(s[1]) == len(s[0]) - 20 and s[0].startswith(s[1]) for s in seqs)                         # a deletion at the end
    assert any(len(s) == 50 for s in seqs)
    over = [s for s in seqs if pr.bound(s) > pr.OVER_BOUND]
    assert len(over) == 1 and len(over[0]) == 7 and {len(x) for x in over[0]} == {9999}
    assert max(pr.bound(c[0]) for c in pr.cases(MAX_LEN) + poa_util.fixtures(MAX_LEN)) == 2050
    assert len(pr.cases(MAX_LEN)) == 49
    many = pr.many_sequences(64)
    assert len(many) == 64 and {len(x) for x in many} == {40} and len(set(many)) > 40


@pytest.mark.parametrize("env", [
    {},                                                             # the product's choice of align form per job
    {"SIMT_LANES_DESCENDING": "1"},                                 # lanes highest first: lane 0's steps run last
    {"SIMT_SCHEDULE": "1"},                                         # the lowest wavefront runs ahead
    {"SIMT_SCHEDULE": "7", "SIMT_LANES_DESCENDING": "1"},           # a random wavefront runs ahead
    {"NDGPU_POA_FORM": "wave"},                                     # K13's one-wavefront form on the device-made tables
    {"NDGPU_POA_FORM": "group", "SIMT_SCHEDULE": "7"},              # K13's workgroup form on them
])
def test_fixtures_with_resident_graphs_on_the_interpreter(env):
    """Every case of poa.npz and poa_device.npz in one call and one by one: the reference's bytes, every problem finished on the
    resident path.  The stats fields do not exist before this feature."""
    r = poa_util.child("simt", "fixtures", MAX_LEN, NDGPU_POA_RESIDENT="1", **env)
    st = r["stats"]
    assert r["bad"] == [] and r["n"] >= 70, r
    assert st["poa_jobs"] == 2 * r["n"] and st["poa_resident_jobs"] == st["poa_jobs"], st
    assert st["poa_resident_declined"] == 0 and st["poa_declined"] == 0 and st["poa_graph_launches"] > 0, st
    assert st["poa_launches"] >= st["poa_rounds"] >= 5 and st["poa_cells"] > 0, st
    # start + consensus per call, rows + thread per round
    assert st["poa_graph_launches"] == 2 * (1 + r["n"]) + 2 * st["poa_rounds"], st


@pytest.mark.parametrize("variable", [None, "1"])
def test_directed_cases_and_the_flags_entry(variable):
    """poa_resident.npz up to 300 bases: api.poa_batch with the variable's choice (in one call and singly), resident=True,
    resident=False and host=True, whatever the variable says."""
    r = pr.child("simt", "resident", MAX_LEN, **({"NDGPU_POA_RESIDENT": variable} if variable else {}))
    n = r["n"]
    assert n == 49
    for name in ("env", "singly", "resident", "rounds", "host"):
        assert r[name]["bad"] == [], (name, r[name])
    for name in ("resident",) + (("env", "singly") if variable else ()):
        st = r[name]["stats"]
        assert st["poa_jobs"] == st["poa_resident_jobs"] == n and st["poa_resident_declined"] == 0 and st["poa_declined"] == 0, (name, st)
        assert st["poa_graph_launches"] > 0 and st["poa_d2h_bytes"] > 0, (name, st)
    for name in ("rounds",) + (() if variable else ("env", "singly")):
        st = r[name]["stats"]
        assert st["poa_jobs"] == n and st["poa_resident_jobs"] == 0 and st["poa_graph_launches"] == 0 and st["poa_declined"] == 0, (name, st)
    assert r["host"]["stats"]["poa_jobs"] == 0 and r["host"]["stats"]["poa_h2d_bytes"] == 0, r["host"]
    # per round 16 + 4 bytes a problem up and 8 down: the resident form moves less than the rounds with their tables and routes
    assert r["resident"]["stats"]["poa_d2h_bytes"] < r["rounds"]["stats"]["poa_d2h_bytes"], r
    assert r["resident"]["stats"]["poa_rounds"] == r["rounds"]["stats"]["poa_rounds"] == 49, r


def test_nothing_fits_the_budget():
    r = poa_util.child("simt", "fixtures", MAX_LEN, NDGPU_POA_RESIDENT="1", NDGPU_POA_BUDGET="0")
    st = r["stats"]
    assert r["bad"] == [] and r["n"] >= 70, r
    assert st["poa_resident_declined"] == st["poa_declined"] == st["poa_jobs"] == 2 * r["n"], st
    assert st["poa_resident_jobs"] == 0 and st["poa_graph_launches"] == 0 and st["poa_launches"] == 0 and st["poa_h2d_bytes"] == 0, st


def test_a_budget_some_arenas_fit():
    """20,000 cells = 120,000 bytes: the arenas may take half of it -- the first small problems of a call stay resident, the rest goes
    to K13's rounds, whose larger problems the host path answers."""
    r = poa_util.child("simt", "fixtures", MAX_LEN, NDGPU_POA_RESIDENT="1", NDGPU_POA_BUDGET="20000")
    st = r["stats"]
    assert r["bad"] == [] and r["n"] >= 70, r
    assert 0 < st["poa_resident_jobs"] < st["poa_jobs"] and 0 < st["poa_declined"] < st["poa_resident_declined"] < st["poa_jobs"], st
    assert st["poa_graph_launches"] > 0, st


def test_a_batch_whose_problems_leave_the_rounds_at_different_times():
    r = pr.child("simt", "mixed", MAX_LEN, NDGPU_POA_RESIDENT="1")
    st = r["stats"]
    assert r["n_two"] >= 10 and r["n_six"] >= 10 and r["many_len"] >= 38, r
    assert r["bad"] == [], r
    assert st["poa_rounds"] == 63 and st["poa_resident_jobs"] == st["poa_jobs"] == r["n"] and st["poa_resident_declined"] == 0, st


def test_argument_errors_of_the_flags_entry():
    r = pr.child("simt", "args")
    for flags in ("6", "7", "8", "16", str(1 << 20), "-1"):
        assert r["rc"][flags] == [-2, True, None], (flags, r)      # -2 and the output slot untouched
    for flags in ("0", "1", "2", "4"):
        assert r["rc"][flags] == [0, False, "ACGT"], (flags, r)
    assert r["empty"] == 0


def test_engine_with_resident_graphs():
    """The golden piles through correct_batch with the regions' POA problems on the resident path: the records of the run without
    either variable."""
    res = poa_util.child("simt", "piles", NDGPU_POA_DEVICE="1", NDGPU_POA_RESIDENT="1")
    plain = poa_util.child("simt", "piles")
    assert res["bad"] == [] and plain["bad"] == [], (res["bad"], plain["bad"])
    assert res["rec"] == plain["rec"] and res["groups"] >= 4
    st = res["stats"]
    assert st["poa_jobs"] > 0 and st["poa_resident_jobs"] == st["poa_jobs"] and st["poa_resident_declined"] == 0 and st["poa_declined"] == 0, st
    assert plain["stats"]["poa_jobs"] == 0, plain["stats"]
