"""K24 on the MI355X (splice_kernel of msa_kernels.hip under DeviceAligner::run_splice, entry ndgpu_splice_batch): the directed cases,
the whole gate family (every length 1001..4096 with lq_total_len within 2 of len / 5), 2,000 fuzz jobs of up to 3,000 words and one job
of 100,000 words, in calls of 1,000; the same jobs shuffled, and a sample of them singly.  Every job against the host statement
(csrc/nd_splice.h), a part of them against the restatement of the reference's lines in splice_util.py.  One child process, shared by
the tests.  tests/test_simt_splice.py runs the smaller set on the interpreter."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import splice_util as su

pytestmark = pytest.mark.gpu

N_FUZZ, MAX_WORDS, N_LONG = 2000, 3000, 100000
N_DIRECTED, N_GATE = 82, 15480
RECORD = 48


@pytest.fixture(scope="module")
def run():
    return su.child("native", "gpu", N_FUZZ, MAX_WORDS, N_LONG, timeout=600)


def test_every_job_equals_the_host_statement(run):
    n = N_DIRECTED + N_GATE + N_FUZZ + 1
    assert run["n"] == n and run["n_dir"] == N_DIRECTED + N_GATE and run["longest"] == N_LONG
    assert run["bad_dev"] == [], run["bad_dev"]          # every field, the float's bits, the bytes


def test_a_part_equals_the_restatement(run):
    assert run["n_restate"] > N_DIRECTED + N_GATE // 16 + N_FUZZ // 3 and run["bad_restate"] == [], run["bad_restate"]


def test_shuffled_and_singly(run):
    assert run["bad_shuffled"] == [] and run["bad_singly"] == [] and run["n_singly"] > 40, run


def test_byte_accounting(run):
    """Down: the fixed record a job plus one byte a result base.  Up: more than the words.  Nothing declined."""
    st = run["stats"]
    n = run["n"]
    assert st["jobs"] == n and st["declined"] == 0 and st["launches"] >= (n + 999) // 1000, st
    assert st["d2h_bytes"] == RECORD * n + run["bytes"], (st, run["bytes"])
    assert st["h2d_bytes"] > 4 * 2500 * N_GATE and st["trimmed"] > N_GATE // 3 and st["ms"] > 0, st


def test_decline_hook():
    r = su.child("native", "batch", 60, 800, 0, "0", NDGPU_SPLICE_DECLINE="2")
    st = r["stats"]
    assert r["bad_host"] == [] and r["bad_dev"] == {str(r["n"]): []}, r
    assert st["declined"] == r["n"] // 2 and st["jobs"] == r["n"], st


def test_engine_five_ways():
    """The engine on the 180 fixture piles (committed fixtures only) under the five environments of tests/test_simt_splice.py."""
    with ThreadPoolExecutor(5) as ex:          # five processes side by side, each with a time limit of its own
        runs = list(ex.map(lambda e: su.child("native", "piles", "golden,edge,rank", timeout=300, **e), su.PILE_ENVS))
    su.check_pile_runs(runs, 180)
