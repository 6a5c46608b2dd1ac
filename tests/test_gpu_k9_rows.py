"""The row routine of the link counter's compact path on the device: the shipped library on the piles of
tests/golden/k9_rows.npz (tests/golden/make_k9_rows_golden.py), against the compiled reference's recorded answers -- equality of
`len`, `float32(identity)` and the bytes -- and against the deep path's tables (NDGPU_K9_DIGEST).  Only the fixture is read.
tests/test_simt_k9_rows.py asks the same of the interpreted kernels; tests/k9_rows_util.py holds what the two share."""
import functools

import pytest

import k9_rows_util as K

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(limit):
    return K.run_child("native", limit, 300)


@pytest.mark.parametrize("limit", (None, 0))
def test_every_pile_alone_and_all_in_one_call_answer_as_the_reference(limit):
    r, _ = run(limit)
    assert r["bad"] == [] and r["tags"] == list(K.TAGS), r


def test_compact_and_deep_path_leave_the_same_tables():
    K.check(run(None), run(0), K.load_piles())
