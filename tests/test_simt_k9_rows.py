"""The row routine of the link counter's compact path on a machine without a GPU: the library's own HIP sources under the
lane-accurate interpreter of tests/simt, on the piles of tests/golden/k9_rows.npz (tests/golden/make_k9_rows_golden.py: a cell
with more than 48 distinct links under 64 busy lanes, a column whose rows spread over the cells, a pile of two reads), against the
compiled reference's recorded answers -- equality of `len`, `float32(identity)` and the bytes -- and against the deep path's
tables (NDGPU_K9_DIGEST).  tests/test_gpu_k9_rows.py asks the same of the shipped library on the device; tests/k9_rows_util.py
holds what the two share."""
import functools
import os
import sys

import pytest

import k9_rows_util as K

sys.path.insert(0, os.path.join(K.HERE, "simt"))


@pytest.fixture(scope="module")
def simt_lib():
    import build_simt
    return build_simt.build()   # built once here, so that no child pays for it


@functools.lru_cache(maxsize=None)
def run(limit):
    return K.run_child("simt", limit, 1500)


@pytest.mark.parametrize("limit", (None, 0))
def test_every_pile_alone_and_all_in_one_call_answer_as_the_reference(simt_lib, limit):
    r, _ = run(limit)
    assert r["bad"] == [] and r["tags"] == list(K.TAGS), r


def test_compact_and_deep_path_leave_the_same_tables(simt_lib):
    K.check(run(None), run(0), K.load_piles())
