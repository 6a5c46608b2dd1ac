"""The link counter's compact path and its deep path on a machine without a GPU: the library's own HIP sources under the
lane-accurate interpreter of tests/simt, on the piles of tests/golden/cover_piles.npz (tests/golden/make_cover_piles_golden.py:
staircases whose 32-column blocks are reached by 30 .. 90 reads, with blocks at exactly 64 and exactly 65, and flat piles at 65
and at 64 on every block), against the compiled reference's recorded answers.  Every comparison is equality of `len`,
`float32(identity)` and the bytes.  tests/test_gpu_k9_compact.py asks the same of the shipped library on the device;
tests/k9_cover_util.py holds what the two share."""
import functools
import os
import sys

import pytest

import k9_cover_util as K

sys.path.insert(0, os.path.join(K.HERE, "simt"))


@pytest.fixture(scope="module")
def simt_lib():
    import build_simt
    return build_simt.build()   # built once here, so that no child pays for it


@pytest.fixture(scope="module")
def piles():
    return K.load_cover_piles()


@functools.lru_cache(maxsize=None)
def each(limit):
    return K.run_child("simt", "each", limit, 1500)


@pytest.mark.parametrize("limit", K.LIMITS)
def test_every_pile_in_a_call_of_its_own(simt_lib, piles, limit):
    """NDGPU_K9_COMPACT unset, 0 (every block deep), 1, 32, 63, 64.  No case is left out."""
    r, trace = each(limit)
    K.check_each(r, trace, limit, piles)


def test_blocks_of_64_and_65_reads_land_on_their_sides(simt_lib):
    K.check_trace({limit: each(limit)[1] for limit in K.LIMITS})


def test_five_piles_in_one_batched_call(simt_lib, piles):
    K.check_batch(K.run_child("simt", "batch", None, 1500)[0], K.run_child("simt", "batch", 0, 1500)[0], piles)


def test_a_staircase_lanes_descending_schedule_one(simt_lib):
    r, trace = K.run_child("simt", "orders", None, 1500)
    assert r["bad"] == [] and r["tags"] == ["stair/ont"], r["bad"]
    assert trace["stair/ont"][0] > 0 and trace["stair/ont"][2] > 0, trace
