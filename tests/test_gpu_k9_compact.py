"""The link counter's compact path and its deep path on the device: the shipped library on the piles of
tests/golden/cover_piles.npz (tests/golden/make_cover_piles_golden.py), against the compiled reference's recorded answers --
equality of `len`, `float32(identity)` and the bytes.  Only the fixture is read.  tests/test_simt_k9_compact.py asks the same of
the interpreted kernels; tests/k9_cover_util.py holds what the two share."""
import functools

import pytest

import k9_cover_util as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def piles():
    return K.load_cover_piles()


@functools.lru_cache(maxsize=None)
def each(limit):
    return K.run_child("native", "each", limit, 600)


@pytest.mark.parametrize("limit", K.LIMITS)
def test_every_pile_in_a_call_of_its_own(piles, limit):
    """NDGPU_K9_COMPACT unset, 0 (every block deep), 1, 32, 63, 64.  No case is left out."""
    r, trace = each(limit)
    K.check_each(r, trace, limit, piles)


def test_blocks_of_64_and_65_reads_land_on_their_sides():
    K.check_trace({limit: each(limit)[1] for limit in K.LIMITS})


def test_five_piles_in_one_batched_call(piles):
    K.check_batch(K.run_child("native", "batch", None, 600)[0], K.run_child("native", "batch", 0, 600)[0], piles)
