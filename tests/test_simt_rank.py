"""The 8-mer ranking of low-quality-region candidates on the device (K14 lq_rank_kernel of lq_kernels.hip: ndgpu_lq_rank_batch under
DeviceAligner::run_rank, and behind K11 in DeviceAligner::run_extract with NDGPU_RANK_DEVICE=1) on a machine without a GPU: the
library's own sources on the lane-accurate interpreter under tests/simt.  The batched entry against the engine's host routine and
against the restatement of the reference's lines in rank_util.py; the engine against what the compiled reference answered for whole
piles (the ranking functions of the reference are static).  The switches and the interpreter's lane order and wavefront schedule are
read once per process, so every variant is a child process.  tests/test_zz_gpu_rank.py runs the same, and more, on the MI355X."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import pytest

import rank_util
import util


def test_directed_cases_are_what_they_claim():
    cases = rank_util.check_directed()
    assert len(cases) >= 20
    jobs = rank_util.fuzz_jobs(300)
    lens = {len(s) for j in jobs for s in j}
    assert {len(j) for j in jobs} >= {1, 2, 5, 10, 11, 40} and set(rank_util.FUZZ_LENS) <= lens


@pytest.mark.parametrize("env", [
    {},                                   # the default schedule
    {"SIMT_LANES_DESCENDING": "1"},       # lanes highest first
    {"SIMT_SCHEDULE": "7"},               # a random wavefront runs ahead
])
def test_rank_batch_on_the_interpreter(env):
    """The directed cases and 300 fuzz jobs: device, host=True and the restatement give equal order, kscore and tail."""
    r = rank_util.child("simt", "batch", 300, 1000, **env)
    st = r["stats"]
    assert r["n"] >= 320 and r["bad_dev"] == [] and r["bad_host"] == [], r
    assert st["rank_jobs"] == r["n"] and st["rank_tail"] == r["tails"] > 20 and st["rank_launches"] == 1 and st["rank_ms"] > 0, st


@pytest.fixture(scope="module")
def pile_runs():
    """The golden piles and the rank_piles cases of nine or fewer reads through correct_batch: with the device ranking, without the
    switch, with the switch while the backend offers nothing, and like the first with a string pool of one byte to start with."""
    envs = [dict(NDGPU_RANK_DEVICE="1", NDGPU_TRACE="1"), {}, dict(NDGPU_RANK_DEVICE="1", NDGPU_RANK_HOST="1"),
            dict(NDGPU_RANK_DEVICE="1", NDGPU_TRACE="1", NDGPU_EXTRACT_POOL="1")]
    with ThreadPoolExecutor(4) as ex:
        return list(ex.map(lambda e: rank_util.child("simt", "piles", "golden,rank", 9, **e), envs))


def test_engine_with_its_ranking_on_the_device_and_on_the_host(pile_runs):
    dev, plain, host = pile_runs[:3]
    assert dev["n"] == plain["n"] == host["n"] >= 30
    assert dev["bad"] == [] and plain["bad"] == [] and host["bad"] == [], (dev["bad"], plain["bad"], host["bad"])   # the reference's answers
    assert dev["rec"] == plain["rec"] == host["rec"]    # length, float32 identity bits, bases
    st = dev["stats"]
    assert st["rank_jobs"] > 0 and st["rank_tail"] > 0 and 0 < st["rank_launches"] <= dev["extract_launches"], (st, dev["extract_launches"])
    assert plain["stats"]["rank_jobs"] == 0 and plain["stats"]["rank_launches"] == 0, plain["stats"]
    assert host["stats"]["rank_jobs"] == 0 and host["stats"]["rank_launches"] == 0, host["stats"]


def test_extract_retakes_a_string_pool_that_was_too_small(pile_runs):
    """NDGPU_EXTRACT_POOL=1 (one context, as every interpreted run): the retake path of DeviceAligner::run_extract."""
    rank_util.check_pool_retake(pile_runs[3], pile_runs[0])


def test_a_job_of_41_sequences_and_an_empty_batch(native_lib):
    from nextdenovo_amd import api
    seqs = (C.c_char_p * 41)(*[b"ACGTACGTAC"] * 41)
    lens = (C.c_uint16 * 41)(*[10] * 41)
    res = (api.RankResult * 2)()
    C.memset(res, 0x55, C.sizeof(res))
    for count in (41, 0, -1):
        jobs = (api.RankJob * 2)(api.RankJob(C.cast(seqs, C.POINTER(C.c_char_p)), C.cast(lens, C.POINTER(C.c_uint16)), 3),
                                 api.RankJob(C.cast(seqs, C.POINTER(C.c_char_p)), C.cast(lens, C.POINTER(C.c_uint16)), count))
        for flags in (0, 1):
            assert native_lib.ndgpu_lq_rank_batch(jobs, 2, flags, res) < 0
    assert bytes(res) == b"\x55" * C.sizeof(res)      # nothing written for that batch
    assert native_lib.ndgpu_lq_rank_batch(None, 0, 0, None) == 0 and native_lib.ndgpu_lq_rank_batch(None, 0, 1, None) == 0
    assert api.lq_rank_batch([], host=True) == []
    with pytest.raises(RuntimeError):
        api.lq_rank_batch([[b"ACGT"] * 41], host=True)


def test_host_routine_against_the_restatement(native_lib):
    """flags bit 0 needs no device: the engine's own routine on the directed cases and the fuzz jobs."""
    from nextdenovo_amd import api
    jobs = [c[1] for c in rank_util.directed_cases()] + rank_util.fuzz_jobs(300)
    got = api.lq_rank_batch(jobs, host=True)
    exp = rank_util.want(jobs)
    bad = [i for i in range(len(jobs)) if tuple(got[i]) != tuple(exp[i])]
    assert not bad, bad[:20]


def test_rank_piles_fixture():
    piles = rank_util.load_rank_piles()
    import os
    assert os.path.getsize(os.path.join(util.GOLD, "rank_piles.npz")) <= 1 << 20
    assert len(piles) >= 24 and {p["read_type"] for p in piles} == {1, 2}
    assert sum(1 for p in piles if len(p["seqs"]) - 1 <= 9) >= 12 and any(len(p["seqs"]) - 1 == 45 for p in piles)
    assert all(p["exp_len"] > 4 for p in piles)


def test_rank_piles_through_the_host_engine(host_harness):
    """The fixture itself: the host engine (oracle aligner as backend, host ranking) gives the reference's recorded answers."""
    fn, fr = util.bind_correct(host_harness, "ndtest_correct", "ndtest_free")
    bad = [w for w in (util.edge_wrong(p, util.call_correct(fn, fr, p, **util.edge_args(p))) for p in rank_util.load_rank_piles()) if w]
    assert not bad, bad
