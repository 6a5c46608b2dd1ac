"""The 8-mer ranking of low-quality-region candidates on the MI355X: ndgpu_lq_rank_batch (K14 lq_rank_kernel of lq_kernels.hip under
DeviceAligner::run_rank) against the engine's host routine and the restatement of the reference's lines in rank_util.py, and the
engine with its regions ranked behind K11 (NDGPU_RANK_DEVICE=1) against the compiled reference's recorded answers for whole piles
(tests/golden/piles.npz, edge_piles.npz, rank_piles.npz: only the fixtures are read).  tests/test_simt_rank.py asks the same of the
interpreted kernel."""
import numpy as np
import pytest

import rank_util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jobs():
    return [c[1] for c in rank_util.directed_cases()] + rank_util.fuzz_jobs(5000)


@pytest.fixture(scope="module")
def restated(jobs):
    return [rank_util.rank(j) for j in jobs]    # (order, kscore, tail, swapped)


@pytest.fixture(scope="module")
def want(restated):
    return [tuple(r[:3]) for r in restated]


def _run(api, jobs, call, host=False):
    out = []
    for a in range(0, len(jobs), call):
        out += api.lq_rank_batch(jobs[a:a + call], host=host)
    return [tuple(r) for r in out]


def test_fuzz_device_host_and_restatement(native_lib, jobs, restated, want):
    """Directed cases + 5,000 fuzz jobs in calls of 1,000."""
    from nextdenovo_amd import api
    rank_util.check_directed()
    assert sum(r[3] for r in restated) >= 20      # jobs in which find_ref_lqseq swaps
    api.reset_stats()
    dev = _run(api, jobs, 1000)
    st = api.stats()
    host = _run(api, jobs, 1000, host=True)
    bad = [i for i in range(len(jobs)) if dev[i] != want[i] or host[i] != want[i]]
    assert not bad, (bad[:20], [(dev[i], want[i]) for i in bad[:2]])
    tails = sum(w[2] for w in want)
    assert st["rank_jobs"] == len(jobs) and st["rank_tail"] == tails > 500 and st["rank_launches"] == (len(jobs) + 999) // 1000, st
    assert api.stats()["rank_jobs"] == len(jobs)      # (the host flag counts nothing)


def test_fuzz_shuffled_and_singly(native_lib, jobs, want):
    from nextdenovo_amd import api
    perm = np.random.default_rng(5).permutation(len(jobs))
    got = _run(api, [jobs[i] for i in perm], 1000)
    assert [got[k] for k in np.argsort(perm)] == want
    some = list(range(len(rank_util.directed_cases()))) + list(range(100, len(jobs), 17))
    assert [_run(api, [jobs[i]], 1)[0] for i in some] == [want[i] for i in some]


@pytest.fixture(scope="module")
def pile_runs():
    """piles.npz, edge_piles.npz and all of rank_piles.npz through correct_batch in child processes: the ranking on the device, the
    ranking and the POA on the device, neither."""
    envs = [dict(NDGPU_RANK_DEVICE="1", NDGPU_TRACE="1"), dict(NDGPU_RANK_DEVICE="1", NDGPU_POA_DEVICE="1", NDGPU_TRACE="1"), {}]
    return [rank_util.child("native", "piles", "golden,edge,rank", "all", **e) for e in envs]   # (one after the other: each plans the device's memory)


def test_engine_with_its_ranking_on_the_device(pile_runs):
    rank, both, plain = pile_runs
    assert rank["n"] == both["n"] == plain["n"] >= 180
    assert rank["bad"] == [] and both["bad"] == [] and plain["bad"] == [], (rank["bad"], both["bad"], plain["bad"])   # the reference's answers
    assert rank["rec"] == both["rec"] == plain["rec"]    # length, float32 identity bits, bases
    for r in (rank, both):
        st = r["stats"]
        assert st["rank_jobs"] >= 100 and st["rank_tail"] >= 6, st
        assert 0 < st["rank_launches"] <= r["extract_launches"], (st["rank_launches"], r["extract_launches"])
    assert both["stats"]["poa_jobs"] > 0 and rank["stats"]["poa_jobs"] == 0
    assert plain["stats"]["rank_jobs"] == 0 and plain["stats"]["rank_launches"] == 0, plain["stats"]


def test_rank_piles_fixture_on_the_device():
    """The fixture's own conditions, from the stats of a device run: at least 100 regions ranked and 6 tail passes in all of it, a tail
    pass among the piles of nine or fewer reads (what the interpreter runs)."""
    whole = rank_util.child("native", "piles", "rank", "all", NDGPU_RANK_DEVICE="1")
    small = rank_util.child("native", "piles", "rank", 9, NDGPU_RANK_DEVICE="1")
    assert whole["bad"] == [] and small["bad"] == []
    assert whole["stats"]["rank_jobs"] >= 100 and whole["stats"]["rank_tail"] >= 6, whole["stats"]
    assert small["stats"]["rank_tail"] >= 1 and small["n"] < whole["n"], small["stats"]


def test_extract_retakes_a_string_pool_that_was_too_small():
    """The piles of nine or fewer reads of rank_piles.npz on one context, each run a process of its own (the pool only grows, so only
    a process's first calls can find it short): NDGPU_EXTRACT_POOL=1 takes the retake path of DeviceAligner::run_extract."""
    env = dict(NDGPU_RANK_DEVICE="1", NDGPU_CONTEXTS="1", NDGPU_TRACE="1")
    short = rank_util.child("native", "piles", "rank", 9, NDGPU_EXTRACT_POOL="1", **env)
    rank_util.check_pool_retake(short, rank_util.child("native", "piles", "rank", 9, **env))
