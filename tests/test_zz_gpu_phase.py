"""The phasing and ranking of HiFi candidates on the MI355X: ndgpu_hifi_phase_batch (K22: hifi_phase_kernel and hifi_phase_rank_kernel
of lq_kernels.hip under DeviceAligner::run_phase) against the engine's host rule and the restatement of the reference's lines in
phase_util.py, and the engine with its regions phased behind K11 (NDGPU_PHASE_DEVICE=1, alone and with the POA switches) against the
compiled reference's recorded answers for the HiFi piles of tests/golden/piles.npz, edge_piles.npz and hifi_phase_piles.npz (only the
fixtures are read).
tests/test_simt_phase.py asks the same of the interpreted kernels."""
import numpy as np
import pytest

import phase_util as pu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def piles():
    return pu.case_piles() + pu.fuzz_piles(2000, seed=515)


@pytest.fixture(scope="module")
def host(native_lib, piles):
    from nextdenovo_amd import api
    return pu.strip(api.hifi_phase_batch(piles, host=True))


def _run(api, piles, call):
    out = []
    for a in range(0, len(piles), call):
        out += api.hifi_phase_batch(piles[a:a + call])
    assert all(r["declined"] == 0 for r in out)
    return pu.strip(out)


def test_fuzz_device_host_and_restatement(native_lib, piles, host):
    """Directed piles + 2,000 fuzz piles in calls of 500: the device against the host rule (all) and the restatement (every third),
    with the byte accounting of phase_stats."""
    from nextdenovo_amd import api
    pu.check_directed()
    api.reset_stats()
    dev = _run(api, piles, 500)
    st = api.phase_stats()
    bad = [i for i in range(len(piles)) if dev[i] != host[i]]
    assert not bad, (bad[:20], dev[bad[0]], host[bad[0]])
    third = list(range(len(pu.case_piles()))) + list(range(len(pu.case_piles()), len(piles), 3))
    bad = [i for i in third if dev[i] != pu.restate(*piles[i])]
    assert not bad, bad[:20]
    regions = sum(len(p[1]) for p in piles)
    kinds = [sum(1 for r in host for g in r["regions"] if g["kind"] == k) for k in range(4)]
    assert st["piles"] == len(piles) and st["regions"] == regions and st["kind"] == kinds and min(kinds) > 0, (st, kinds)
    assert st["pass2_piles"] == sum(r["pass2"] for r in host) > 100 and st["tail_passes"] == sum(g["tail"] for r in host for g in r["regions"]) > 100
    assert st["launches"] == (len(piles) + 499) // 500 and st["ms"] > 0 and st["declined"] == [0] * 5, st
    assert st["d2h_record_bytes"] == 32 * len(piles) + 128 * regions and st["d2h_string_bytes"] == 0, st
    api.hifi_phase_batch(piles[:50], host=True)
    assert api.phase_stats()["piles"] == len(piles)      # (the host flag counts nothing)


def test_fuzz_shuffled_and_singly(native_lib, piles, host):
    from nextdenovo_amd import api
    perm = np.random.default_rng(5).permutation(len(piles))
    got = _run(api, [piles[i] for i in perm], 1000)
    assert [got[k] for k in np.argsort(perm)] == host
    some = list(range(len(pu.case_piles()))) + list(range(100, len(piles), 41))
    assert [_run(api, [piles[i]], 1)[0] for i in some] == [host[i] for i in some]


def test_a_pile_of_3000_regions(native_lib):
    from nextdenovo_amd import api
    big = pu.big_pile(3000)
    dev = api.hifi_phase_batch([big])
    assert dev[0]["declined"] == 0
    assert pu.strip(dev) == pu.strip(api.hifi_phase_batch([big], host=True))
    assert {g["kind"] for g in dev[0]["regions"]} == {1, 2, 3}


def test_a_pile_above_the_read_capacity_comes_back_declined(native_lib):
    """2,049 aligned reads: one over the LDS table (kPhaseReads of nd_device.h); the record is the host rule's."""
    from nextdenovo_amd import api
    cap = pu.capacity_piles()
    api.reset_stats()
    dev = api.hifi_phase_batch(cap)
    assert [r["declined"] for r in dev] == [0, 1, 0]
    assert pu.strip(dev) == pu.strip(api.hifi_phase_batch(cap, host=True)) == [pu.restate(*p) for p in cap]
    st = api.phase_stats()
    assert st["declined"] == [1, 0, 0, 0, 0] and st["piles"] == 2, st


@pytest.fixture(scope="module")
def pile_runs():
    """The HiFi piles of piles.npz and edge_piles.npz through correct_batch in child processes, one after the other (each plans the
    device's memory), each under its own time limit; a failed child ends the test: without the switch, with it, with it and the POA on
    the device, with it and the resident POA graphs."""
    envs = [{}, dict(NDGPU_PHASE_DEVICE="1", NDGPU_TRACE="1"), dict(NDGPU_PHASE_DEVICE="1", NDGPU_POA_DEVICE="1"),
            dict(NDGPU_PHASE_DEVICE="1", NDGPU_POA_DEVICE="1", NDGPU_POA_RESIDENT="1")]
    return [pu.child("native", "piles", "golden,edge,phase", "all", timeout=120, **e) for e in envs]


def test_engine_with_its_phasing_on_the_device(pile_runs):
    plain, dev, poa, resident = pile_runs
    assert plain["n"] == dev["n"] == poa["n"] == resident["n"] >= 3 + 38
    for r in pile_runs:
        assert r["bad"] == [], r["bad"]      # the reference's answers
    assert plain["rec"] == dev["rec"] == poa["rec"] == resident["rec"]    # length, float32 identity bits, bases
    assert plain["phase"]["launches"] == 0 and plain["phase"]["piles"] == 0, plain["phase"]
    for r in (dev, poa, resident):
        st = r["phase"]
        assert st["piles"] > 0 and st["regions"] > 0 and st["launches"] > 0 and sum(st["declined"]) == 0, st
        assert st["d2h_record_bytes"] > 0 and st["d2h_string_bytes"] > 0, st
        # records of every kind the fixtures reach go through the engine: ranked with and without the tail pass, seeds in either
        # case; the second pass ran (no fixture pile reaches a dropped region: DESIGN.md)
        assert st["kind"][3] >= 40 and 3 <= st["tail_passes"] < st["kind"][3] and 0 < st["seed_lower"] < st["kind"][2], st
        assert st["pass2_piles"] >= 3, st
    assert dev["trace_lines"] == dev["phase"]["launches"]
