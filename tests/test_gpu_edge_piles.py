"""nextCorrect() of the shipped library on the device, on the hand-built edge piles of tests/golden/edge_piles.npz and away
from its default arguments: `len`, `float32(identity)` and the bytes equal the compiled reference's recorded answers.  Only the
fixture is read (tests/golden/make_edge_piles_golden.py made it; tests/test_simt_edge_piles.py asks the same of the interpreted
kernels).  The cases in which the reference itself dies are not run here."""
import json
import os
import subprocess
import sys

import pytest

import util
from util import EDGE_CAPACITY_FAMILIES, EDGE_TRACE_REPEAT, EDGE_TRACE_THIRD

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def piles():
    return util.load_edge_piles()


def test_every_pile_in_a_call_of_its_own(native_lib, piles):
    fn, fr = util.bind_correct(native_lib)
    assert len(piles) >= 120
    bad = [w for w in (util.edge_wrong(p, util.call_correct(fn, fr, p, **util.edge_args(p))) for p in piles) if w]
    assert not bad, bad


def test_piles_of_equal_arguments_in_one_batched_call(native_lib, piles):
    """The sub-batch that the link counter repeats (twice: the repeat and the links family are in it) also holds ordinary piles."""
    from nextdenovo_amd import api
    g = util.edge_groups(piles)
    big = max(g.values(), key=len)
    assert len(g) >= 20 and len(big) >= 30 and any(p["tag"].startswith("links/") for p in big)
    bad = []
    for key, members in g.items():
        bad += [w for w in (util.edge_wrong(p, r) for p, r in zip(members, util.edge_correct_group(api, key, members))) if w]
    assert not bad, bad


_CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
import util
from nextdenovo_amd import api
api.load()
mode = sys.argv[1]
key, big = max(util.edge_groups(util.load_edge_piles()).items(), key=lambda kv: len(kv[1]))
if mode == "capacity":            # the families built for the capacity paths between ordinary piles, one call
    special = [p for p in big if p["tag"].startswith(util.EDGE_CAPACITY_FAMILIES)]
    plain = [p for p in big if p["tag"].startswith("seedlen/")][:len(special) + 1]
    members = [q for pair in zip(plain, special) for q in pair] + plain[len(special):]
else:
    members = big
got = util.edge_correct_group(api, key, members)
bad = [w for w in (util.edge_wrong(p, r) for p, r in zip(members, got)) if w]
print(json.dumps(dict(bad=bad, n=len(members), tags=[p["tag"] for p in members], slow=api.stats()["score_slow_piles"])))
"""


def child(mode, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("NDGPU_K9", "NDGPU_K10"))}   # no force switch reaches the child
    e.update(env)
    out = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(HERE), HERE), mode], env=e, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


def test_capacity_paths_are_taken_without_a_switch():
    """The piles themselves overflow the link counter's first attempt (repeat), its second (links: the third attempt keeps its lists
    in device memory, and counts the 611 accepted reads of stack/600-deep with it) and the scoring kernels' column tables, by a wide
    column (int64) and by a deep one (stack) -- the trace says so, and the answers are the reference's."""
    r, err = child("capacity", NDGPU_TRACE="1")
    assert r["bad"] == [], r
    assert sum(t.startswith(EDGE_CAPACITY_FAMILIES) for t in r["tags"]) >= 8 and "stack/600-deep" in r["tags"] and sum(t.startswith("seedlen/") for t in r["tags"]) >= 8
    assert EDGE_TRACE_REPEAT in err, err[-2000:]
    assert EDGE_TRACE_THIRD in err, err[-2000:]
    assert r["slow"] >= 2, r
    assert "FATAL" not in err


def test_largest_group_in_sub_batches_of_two_on_two_contexts():
    r, _ = child("largest-group", NDGPU_SUBBATCH="2", NDGPU_CONTEXTS="2")
    assert r["bad"] == [] and r["n"] >= 30, r
