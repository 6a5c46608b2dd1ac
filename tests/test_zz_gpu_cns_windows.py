"""The consensus words and low-quality windows of the main walk on the MI355X: ndgpu_cns_windows_batch (K20 cns_windows_kernel of
msa_kernels.hip under DeviceAligner::run_cns) against the engine's host routine and the restatement of the reference's lines in
cns_util.py, and the engine with K20 inside its main phase (NDGPU_CNS_DEVICE=1) against the compiled reference's recorded answers
for whole piles (tests/golden/piles.npz, edge_piles.npz, rank_piles.npz: only the fixtures are read).
tests/test_simt_cns_windows.py asks the same of the interpreted kernel.

The host routine answers for every walk; the restatement (pure Python, a microsecond an item) for the directed cases, every third
fuzz walk and the long one -- tests/test_simt_cns_windows.py holds the two equal on its whole set."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cns_util

pytestmark = pytest.mark.gpu

N_FUZZ, MAX_ITEMS, LONG = 5000, 3000, 200000


@pytest.fixture(scope="module")
def walks():
    return [c[1] for c in cns_util.directed_cases()] + cns_util.fuzz_walks(N_FUZZ, MAX_ITEMS) + [cns_util.long_walk(LONG)]


@pytest.fixture(scope="module")
def jobs(native_lib, walks):
    from nextdenovo_amd import api
    return cns_util.to_jobs(api, walks)


@pytest.fixture(scope="module")
def host(jobs):
    from nextdenovo_amd import api
    return api.cns_windows_batch(jobs, host=True)


KEYS = ("len", "uncorrected_len", "lstrip", "rstrip", "lqseq_total_length", "ok")


def same(a, b):
    return all(a[k] == b[k] for k in KEYS) and np.array_equal(a["bases"], b["bases"]) and np.array_equal(a["regions"], b["regions"])


def test_device_host_and_restatement(walks, jobs, host):
    """Directed cases, 5,000 fuzz walks of up to 3,000 items and one of 200,000, in calls of 1,000."""
    from nextdenovo_amd import api
    cns_util.check_directed()
    n_dir = len(cns_util.directed_cases())
    assert len(walks) == n_dir + N_FUZZ + 1 and walks[-1][0].shape[0] == LONG and max(w[0].shape[0] for w in walks[:-1]) <= MAX_ITEMS
    api.reset_stats()
    dev = []
    for a in range(0, len(jobs), 1000):
        dev += api.cns_windows_batch(jobs[a:a + 1000])
    st = api.stats()
    bad = [i for i in range(len(jobs)) if not same(dev[i], host[i])]
    assert not bad, bad[:20]
    some = list(range(n_dir)) + list(range(n_dir, len(walks) - 1, 3)) + [len(walks) - 1]
    tot = dict.fromkeys(cns_util.BRANCHES, 0)
    for i in some:
        e = cns_util.restate(*walks[i])
        for k, v in e["br"].items():
            tot[k] += v
        e["bases"], e["regions"] = np.asarray(e["bases"], dtype=np.uint32), np.asarray(e["regions"], dtype=np.uint32).reshape(-1, 2)
        assert same(dev[i], e), i
    assert all(tot[k] >= 20 for k in cns_util.BRANCHES), tot
    n_reg = sum(len(r["regions"]) for r in host)
    assert st["cns_jobs"] == len(jobs) and st["cns_declined"] == 0 and st["cns_regions"] == n_reg > 5000, st
    assert st["cns_launches"] >= (len(jobs) + 999) // 1000 and st["cns_ms"] > 0 and st["walk_d2h_bytes"] == 0, st
    # what came down: 32 bytes a walk, 4 a consensus base, 8 a window
    assert st["cns_d2h_bytes"] == 32 * len(jobs) + 4 * sum(r["len"] for r in host) + 8 * n_reg, st


def test_shuffled_and_singly(jobs, host):
    from nextdenovo_amd import api
    perm = np.random.default_rng(5).permutation(len(jobs))
    got = []
    for a in range(0, len(jobs), 1000):
        got += api.cns_windows_batch([jobs[i] for i in perm[a:a + 1000]])
    assert all(same(got[k], host[int(i)]) for k, i in enumerate(perm))
    some = list(range(len(cns_util.directed_cases()))) + list(range(100, len(jobs), 97)) + [len(jobs) - 1]
    assert all(same(api.cns_windows_batch([jobs[i]])[0], host[i]) for i in some)


@pytest.fixture(scope="module")
def pile_runs():
    """piles.npz, edge_piles.npz and rank_piles.npz through correct_batch in child processes (the switches are read once per
    process; the child drops a caller's NDGPU_CNS* variables): K20 on, K20 on beside the three other opt-ins, nothing set, and K20
    on with every third pile declined."""
    envs = [dict(NDGPU_CNS_DEVICE="1"),
            dict(NDGPU_CNS_DEVICE="1", NDGPU_RANK_DEVICE="1", NDGPU_POA_DEVICE="1", NDGPU_POA_RESIDENT="1"),
            {},
            dict(NDGPU_CNS_DEVICE="1", NDGPU_CNS_DECLINE="3")]
    with ThreadPoolExecutor(4) as ex:
        return list(ex.map(lambda e: cns_util.child("native", "piles", "golden,edge,rank", timeout=600, **e), envs))


def test_engine_equals_the_reference_with_and_without_the_switch(pile_runs):
    on, all_on, unset, declined = pile_runs
    for r in pile_runs:
        assert r["n"] == 16 + 133 + 31 and r["bad"] == [], r["bad"]          # the reference's recorded answers
    assert on["rec"] == all_on["rec"] == unset["rec"] == declined["rec"]     # length, float32 identity bits, bases
    # 7 + 4 of 16, 74 + 30 of 133 and 31 of 31 piles are raw reads; 2 and 6 piles are -fast calls, two of the six on HiFi reads
    for r in pile_runs:
        assert r["raw"]["piles"] == (11 - 2) + (104 - 4) + 31, r["raw"]
    for r in (on, all_on):
        raw = r["raw"]
        assert raw["cns_declined"] == 0 and raw["cns_jobs"] >= raw["expected"] > 100 and raw["cns_launches"] > 0, raw
        assert raw["walk_d2h_bytes"] == 0 and 0 < raw["cns_d2h_bytes"] < unset["raw"]["walk_d2h_bytes"], (raw, unset["raw"])
        assert r["stats"]["cns_jobs"] == raw["cns_jobs"]                     # no HiFi or -fast pile takes the kernel
    st = unset["stats"]
    assert st["cns_jobs"] == st["cns_launches"] == 0 and st["walk_d2h_bytes"] > 0 and unset["raw"]["walk_d2h_bytes"] > 0, st
    assert declined["raw"]["cns_declined"] > 0 and declined["raw"]["cns_jobs"] > 0, declined["raw"]
