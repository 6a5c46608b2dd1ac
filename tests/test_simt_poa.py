"""The batched device POA (ndgpu_poa_batch: K13 of lq_kernels.hip under DeviceAligner::run_poa) on a machine without a GPU: the
library's own sources on the lane-accurate interpreter under tests/simt, against what the compiled reference's poa_to_consensus
returned (tests/golden/poa.npz, tests/golden/poa_device.npz).  Cases up to 257 bases a sequence: the interpreter is slow, and
tests/test_zz_gpu_poa.py runs the long ones.  The kernel form, the budget and the interpreter's lane order and wavefront schedule
are read once per process, so every variant is a child process."""
import pytest

import poa_util

MAX_LEN = 300   # (a 257-base case's mutated copies run a few bases over)


def test_fixture_holds_what_the_device_path_must_meet():
    dev = poa_util.load("poa_device.npz")
    lens = sorted({len(s) for seqs, _ in dev for s in seqs})
    assert len(poa_util.load("poa.npz")) == 40 and len(dev) >= 40
    assert {1, 2, 3, 64, 128, 256} <= set(lens) and any(900 < x < 1200 for x in lens) and max(lens) > 3000
    assert any(len(set(seqs)) == 1 and len(seqs) > 2 for seqs, _ in dev)                            # all sequences identical
    assert any(len(seqs) == 2 and seqs[0].startswith(seqs[1]) and seqs[0] != seqs[1] for seqs, _ in dev)   # a prefix only
    assert any(len(seqs) == 2 and seqs[0].endswith(seqs[1]) and seqs[0] != seqs[1] for seqs, _ in dev)     # a suffix only
    assert any(len(set(b"".join(seqs))) == 1 for seqs, _ in dev) and any(len(set(b"".join(seqs))) == 2 for seqs, _ in dev)
    assert len(poa_util.fixtures(MAX_LEN)) >= 70


@pytest.mark.parametrize("env,launches", [
    ({}, True),                                                                            # the product's choice of form per job
    ({"NDGPU_POA_FORM": "wave", "SIMT_LANES_DESCENDING": "1"}, True),                     # one wavefront per job, lanes highest first
    ({"NDGPU_POA_FORM": "group", "SIMT_SCHEDULE": "7", "SIMT_LANES_DESCENDING": "1"}, True),   # one workgroup per job, a random wavefront runs ahead, lanes highest first
    ({"NDGPU_POA_GROUP_MIN": "64", "SIMT_SCHEDULE": "1"}, True),                           # both forms in every round, the lowest wavefront runs ahead
    ({"NDGPU_POA_BUDGET": "0"}, False),                                                    # nothing fits: every job declined, host path
    ({"NDGPU_POA_BUDGET": "20000"}, True),                                                 # small slices, the larger jobs declined
])
def test_poa_batch_on_the_interpreter(env, launches):
    """Every case in one call and one by one: the reference's bytes, whichever kernel form took the job and whatever was declined."""
    r = poa_util.child("simt", "fixtures", MAX_LEN, **env)
    st = r["stats"]
    assert r["bad"] == [] and r["n"] >= 70, r
    assert st["poa_jobs"] == 2 * r["n"], st
    if not launches:
        assert st["poa_declined"] == st["poa_jobs"] and st["poa_launches"] == 0 and st["poa_cells"] == 0, st
    elif env.get("NDGPU_POA_BUDGET"):
        assert 0 < st["poa_declined"] < st["poa_jobs"] and st["poa_launches"] > st["poa_rounds"] > 0, st
    else:
        assert st["poa_declined"] == 0 and st["poa_launches"] >= st["poa_rounds"] >= 5 and st["poa_cells"] > 0, st
    if env.get("NDGPU_POA_GROUP_MIN"):
        assert st["poa_launches"] > st["poa_rounds"], st       # (two launches in the rounds of the call with every case)
