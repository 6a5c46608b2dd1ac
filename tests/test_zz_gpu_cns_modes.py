"""The HiFi and -fast forms of the loop behind the main walk on the MI355X: ndgpu_cns_walk_batch (K21 cns_walk_kernel of
msa_kernels.hip under DeviceAligner::run_cns_walk) against the engine's host routines and the restatements of the reference's lines
in cns_modes_util.py, and the engine with K21 inside its main phase (NDGPU_CNS_HIFI=1, NDGPU_CNS_FAST=1) against the compiled
reference's recorded answers for whole piles (tests/golden/piles.npz, edge_piles.npz, rank_piles.npz: only the fixtures are read).
tests/test_simt_cns_modes.py asks the same of the interpreted kernel.

Every GPU step is a child process under a time limit of its own (the switches are read once per process anyway); a child that dies
fails its fixture, and nothing is launched after it.  The host routine answers for every walk; the restatement (pure Python) for
the directed cases, every third fuzz walk and the long one."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import cns_modes_util as cm

pytestmark = pytest.mark.gpu

N_FUZZ, MAX_ITEMS, LONG = 2000, 1500, 100000
N_DIRECTED = {1: 30, 2: 34}


@pytest.fixture(scope="module", params=[1, 2])
def batch(request, native_lib):
    return request.param, cm.child("native", "gpu", request.param, N_FUZZ, MAX_ITEMS, LONG, timeout=300)


def test_device_host_and_restatement(batch):
    """Directed cases, 2,000 fuzz walks of up to 1,500 items and one of 100,000 per mode, in calls of 1,000; the same walks shuffled,
    and a sample of them singly."""
    mode, r = batch
    cm.check_directed()
    n = N_DIRECTED[mode] + N_FUZZ + 1
    assert r["n"] == n and r["n_dir"] == N_DIRECTED[mode] and r["longest"] == LONG and r["longest_fuzz"] <= MAX_ITEMS, r
    assert r["bad_dev"] == [] and r["bad_restate"] == [] and r["n_restate"] == N_DIRECTED[mode] + (N_FUZZ + 2) // 3 + 1, r
    assert r["bad_shuffled"] == [] and r["bad_singly"] == [] and r["n_singly"] > N_DIRECTED[mode] + 20, r
    assert all(r["br"][k] >= 20 for k in (cm.K_BRANCHES if mode == 1 else cm.F_BRANCHES)), r["br"]


def test_byte_accounting(batch):
    """What came down in the calls of 1,000: 32 bytes a walk, and for HiFi 4 a consensus base and 8 a window; for -fast the strings,
    one byte a base, packed one behind the other without padding (the 4 bytes a job the bound allows are not used)."""
    mode, r = batch
    st, ms = r["stats"], r["mode_stats"]
    n = r["n"]
    if mode == 1:
        assert ms["hifi_jobs"] == n and ms["fast_jobs"] == 0 and ms["hifi_regions"] == r["regions"] > 2000, ms
        assert ms["d2h_bytes"] == 32 * n + 4 * r["sum_len"] + 8 * r["regions"], (ms, r["sum_len"])
    else:
        assert ms["fast_jobs"] == n and ms["hifi_jobs"] == ms["hifi_regions"] == 0, ms
        assert 32 * n + r["sum_len"] <= ms["d2h_bytes"] <= 32 * n + r["sum_len"] + 4 * n, (ms, r["sum_len"])
    assert ms["hifi_declined"] == ms["fast_declined"] == 0 and ms["launches"] >= (n + 999) // 1000 and ms["ms"] > 0, ms
    assert st["walk_d2h_bytes"] == 0 and st["cns_jobs"] == st["cns_d2h_bytes"] == 0, st


@pytest.fixture(scope="module")
def pile_runs(native_lib):
    """piles.npz, edge_piles.npz and rank_piles.npz through correct_batch in child processes (the child drops a caller's NDGPU_CNS*
    variables): both switches on; on beside the four other opt-ins; nothing set; on with every third walk declined; and
    NDGPU_CNS_DEVICE alone, for the raw groups' counters."""
    on = dict(NDGPU_CNS_HIFI="1", NDGPU_CNS_FAST="1")
    envs = [on,
            dict(on, NDGPU_CNS_DEVICE="1", NDGPU_RANK_DEVICE="1", NDGPU_POA_DEVICE="1", NDGPU_POA_RESIDENT="1"),
            {},
            dict(on, NDGPU_CNS_DECLINE="3"),
            dict(NDGPU_CNS_DEVICE="1")]
    with ThreadPoolExecutor(len(envs)) as ex:
        return list(ex.map(lambda e: cm.child("native", "piles", "golden,edge,rank", timeout=600, **e), envs))


def test_engine_equals_the_reference_with_and_without_the_switches(pile_runs):
    on, all_on, unset, declined, raw_only = pile_runs
    for r in pile_runs:
        assert r["n"] == 16 + 133 + 31 and r["bad"] == [], r["bad"]          # all 180 piles: the reference's recorded answers
    assert on["rec"] == all_on["rec"] == unset["rec"] == declined["rec"]     # length, float32 identity bits, bases
    for r in pile_runs:
        k = r["kinds"]
        assert k["hifi"]["piles"] == 32 and k["fast"]["piles"] == 8 and k["raw"]["piles"] == 140, k
    u = unset["kinds"]
    for r in (on, all_on):
        for kind, jobs in (("hifi", "hifi_jobs"), ("fast", "fast_jobs")):
            g = r["kinds"][kind]
            assert g["walk_d2h_bytes"] == 0 and 0 < g["d2h_bytes"] < u[kind]["walk_d2h_bytes"], (kind, g, u[kind])
            assert g[jobs] > 0 and g["hifi_declined"] == g["fast_declined"] == 0 and g["launches"] > 0 and g["cns_jobs"] == 0, (kind, g)
        assert r["kinds"]["hifi"]["fast_jobs"] == 0 and r["kinds"]["fast"]["hifi_jobs"] == 0
    # NDGPU_CNS_DEVICE goes on meaning the raw groups alone, beside the new switches or without them
    assert all_on["kinds"]["raw"]["cns_jobs"] == raw_only["kinds"]["raw"]["cns_jobs"] == raw_only["stats"]["cns_jobs"] > 100
    assert all_on["stats"]["cns_jobs"] == all_on["kinds"]["raw"]["cns_jobs"] and all_on["kinds"]["raw"]["walk_d2h_bytes"] == 0
    assert on["kinds"]["raw"]["cns_jobs"] == 0 and on["kinds"]["raw"]["walk_d2h_bytes"] > 0 and on["kinds"]["raw"]["launches"] == 0
    assert all(v == 0 for v in raw_only["mode_stats"].values()) and all(v == 0 for v in unset["mode_stats"].values())
    assert unset["stats"]["cns_jobs"] == 0 and all(u[k]["walk_d2h_bytes"] > 0 for k in ("hifi", "fast", "raw"))
    d = declined["kinds"]
    assert d["hifi"]["hifi_declined"] > 0 and d["hifi"]["hifi_jobs"] > 0 and d["fast"]["fast_declined"] + d["hifi"]["hifi_declined"] > 0, d
    assert d["fast"]["fast_jobs"] > 0 and d["hifi"]["walk_d2h_bytes"] > 0, d
