"""nextCorrect() on hand-built edge piles and away from its default arguments, on a machine without a GPU: the consensus library's
own HIP sources under the lane-accurate interpreter of tests/simt, against the compiled reference's answers recorded in
tests/golden/edge_piles.npz (tests/golden/make_edge_piles_golden.py says what every family is for).  Every comparison is equality
of `len`, `float32(identity)` and the bytes.  tests/test_gpu_edge_piles.py asks the same of the shipped library on the device.

Every call into the interpreted library is made in a child process that names the pile (or the group) before it starts: a kernel
that walks off its tables kills the interpreter, and the test then fails with the name of the pile instead of taking pytest along.

What the module catches, tried one change at a time on a copy of the kernels (none of them is in the tree):
  admission cut `>` -> `>=` (pile_accept_kernel)              per-pile and batched tests: args/*/max_cov_aln=*, cut/*/full, count/cut-at-*
  accepted alignment `>=` -> `>` min_len_aln                  per-pile, batched, sub-batches of two: seedlen/500-exact-copies, window/aln-len-500
  err word not cleared before the link counter's repeat       per-pile[repeat], [links]: the child aborts at repeat/63-insertions, links/192-insertions
  `rank < n_acc` -> `<=` in the register chunks               per-pile, eight families: the child dies (SIGSEGV) at count/63, seedlen/511, ...
  `rank < n_acc` -> `<=` in the later chunks                  per-pile[count], [links], [stack]: SIGSEGV at count/129, links/192-insertions, stack/cut-...
  last partial 32-column block dropped (`t_end`)              per-pile, eight families: SIGSEGV at seedlen/511, cut/ont/full, ...
  count of a known link not raised, count_links_global_kernel every test that runs links/192-insertions"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import refpipe
import util

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "simt"))

from util import EDGE_CAPACITY_FAMILIES as CAPACITY_FAMILIES, EDGE_TRACE_REPEAT as TRACE_REPEAT, EDGE_TRACE_THIRD as TRACE_THIRD
from util import edge_correct_group as correct_group, edge_groups as groups, edge_wrong as wrong


@pytest.fixture(scope="module")
def simt_lib():
    import build_simt
    os.environ.setdefault("NDGPU_CONTEXTS", "1")  # one device context: the interpreter brings its own host threads
    return C.CDLL(build_simt.build())


@pytest.fixture()
def simt_api(simt_lib, monkeypatch):
    from nextdenovo_amd import api
    monkeypatch.setattr(api, "_LIB", api._bind(simt_lib))
    return api


@pytest.fixture(scope="module")
def piles():
    return util.load_edge_piles()


def test_the_fixture_holds_every_family(piles):
    fams = {}
    for p in piles:
        fams[p["tag"].split("/")[0]] = fams.get(p["tag"].split("/")[0], 0) + 1
    assert set(fams) == set(util.EDGE_FAMILIES), fams
    assert len(piles) >= 120
    for rt in (1, 2, 3):   # the five frozen arguments, -s and -fast away from their defaults for every read type
        mine = [p for p in piles if p["read_type"] == rt]
        assert {p["max_cov_aln"] for p in mine} - {130} and {p["min_cov_base"] for p in mine} - {4}
        assert {p["min_len_aln"] for p in mine} - {500} and {np.float32(p["ratio"]) for p in mine} - {np.float32(0.8)}
        assert any(p["fast"] for p in mine) and any(p["split"] for p in mine)
        assert any(p["max_lq"] != min(len(p["seqs"][0]) // 2, 10000 if rt == 1 else 1000) for p in mine)


def run_child(code, args, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("NDGPU_")}   # no force switch reaches the child
    e.update(NDGPU_CONTEXTS="1")
    e.update(env)
    out = subprocess.run([sys.executable, "-c", code % (os.path.dirname(HERE), HERE, os.path.join(HERE, "simt"))] + list(args), env=e,
                         capture_output=True, text=True, timeout=1500)
    begun = [ln[6:] for ln in out.stdout.splitlines() if ln.startswith("BEGIN ")]
    assert out.returncode == 0, "the child ended with status %d in %s\n%s" % (out.returncode, begun[-1] if begun else "its start", out.stderr[-3000:])
    return out


_PILE_CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%r, %r, %r]
import util, build_simt
fn, fr = util.bind_correct(C.CDLL(build_simt.build()))
bad, n = [], 0
for p in util.load_edge_piles():
    if p["tag"].split("/")[0] == sys.argv[1]:
        print("BEGIN", p["tag"], flush=True)
        w = util.edge_wrong(p, util.call_correct(fn, fr, p, **util.edge_args(p)))
        bad += [w] if w else []
        n += 1
print(json.dumps(dict(bad=bad, n=n)))
"""


@pytest.mark.parametrize("family", util.EDGE_FAMILIES)
def test_every_pile_in_a_call_of_its_own(simt_lib, piles, family):
    """The drop-in entry point, one pile per call, with the arguments the fixture records.  No case is left out."""
    r = json.loads(run_child(_PILE_CHILD, [family]).stdout.strip().splitlines()[-1])
    assert r["bad"] == [], r["bad"]
    assert r["n"] == sum(p["tag"].split("/")[0] == family for p in piles) > 0


def test_piles_of_equal_arguments_in_one_batched_call(simt_lib, piles):
    """Every group of piles with the same arguments in ONE correct_batch call: the sub-batch that is repeated for the repeat
    and links families also holds ordinary piles, so whatever an overflowing attempt leaves in a neighbour's columns shows."""
    g = groups(piles)
    assert len(g) >= 20 and sum(len(m) for m in g.values()) == len(piles)
    big = max(g.values(), key=len)
    assert any(p["tag"].startswith("repeat/") for p in big) and any(p["tag"].startswith("links/") for p in big) and len(big) >= 30
    r, _ = child("all-groups")
    assert r["bad"] == [] and r["n"] == len(piles), r


_CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, build_simt
from nextdenovo_amd import api
lib = C.CDLL(build_simt.build())
api._LIB = api._bind(lib)
mode = sys.argv[1]
piles = util.load_edge_piles()
if mode == "all-groups":
    members, got = [], []
    for key, ms in util.edge_groups(piles).items():
        print("BEGIN the group of", ms[0]["tag"], flush=True)
        members += ms
        got += util.edge_correct_group(api, key, ms)
elif mode == "largest-group":
    key, members = max(util.edge_groups(piles).items(), key=lambda kv: len(kv[1]))
    got = util.edge_correct_group(api, key, members)
elif mode == "capacity":          # the families built for the capacity paths between ordinary piles, one call
    key, big = max(util.edge_groups(piles).items(), key=lambda kv: len(kv[1]))
    special = [p for p in big if p["tag"].startswith(util.EDGE_CAPACITY_FAMILIES)]
    plain = [p for p in big if p["tag"].startswith("seedlen/")][:len(special) + 1]
    members = [q for pair in zip(plain, special) for q in pair] + plain[len(special):]
    got = util.edge_correct_group(api, key, members)
elif mode == "orders":            # the same families one by one, lanes of a wavefront highest first, lowest wavefront runs ahead
    lib.simt_set_lane_order(1)
    lib.simt_set_schedule(1)
    fn, fr = util.bind_correct(lib)
    members = [p for p in piles if p["tag"].startswith(util.EDGE_CAPACITY_FAMILIES)]
    got = []
    for p in members:
        print("BEGIN", p["tag"], flush=True)
        got.append(util.call_correct(fn, fr, p, **util.edge_args(p)))
bad = [w for w in (util.edge_wrong(p, r) for p, r in zip(members, got)) if w]
print(json.dumps(dict(bad=bad, n=len(members), tags=[p["tag"] for p in members], slow=api.stats()["score_slow_piles"])))
"""


def child(mode, **env):
    out = run_child(_CHILD, [mode], **env)
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


def test_largest_group_in_sub_batches_of_two_on_two_contexts(simt_lib):
    r, _ = child("largest-group", NDGPU_SUBBATCH="2", NDGPU_CONTEXTS="2")
    assert r["bad"] == [] and r["n"] >= 30, r


def test_capacity_paths_are_taken_without_a_switch(simt_lib):
    """No NDGPU_K9_FORCE_RETRY, no NDGPU_K10_FORCE: the piles themselves overflow the link counter's first attempt (repeat), its
    second (links) and the scoring kernels' column tables, by a wide column (int64) and by a deep one (stack), in one sub-batch with
    ordinary piles around them.  The third attempt of the link counter then also counts the 611 accepted reads of stack/600-deep."""
    r, err = child("capacity", NDGPU_TRACE="1")
    assert r["bad"] == [], r
    assert sum(t.startswith(CAPACITY_FAMILIES) for t in r["tags"]) >= 8 and "stack/600-deep" in r["tags"] and sum(t.startswith("seedlen/") for t in r["tags"]) >= 8
    assert TRACE_REPEAT in err, err[-2000:]
    assert TRACE_THIRD in err, err[-2000:]
    assert r["slow"] >= 2, r
    assert "FATAL" not in err


def test_capacity_families_lanes_descending_schedule_one(simt_lib):
    r, _ = child("orders")
    assert r["bad"] == [] and r["n"] >= 9, r


_REF_CHILD = r"""
import json, os, signal, sys
sys.path[:0] = [%r, %r, %r]
import refpipe, util
lib = refpipe.ref_cns()


def ask(p):   # the live reference's answer, or the signal that killed it: one forked child per case, because it can die
    rd, wr = os.pipe()
    pid = os.fork()
    if pid == 0:
        try:
            ln, ide, seq = refpipe.call_nextcorrect(lib, p["seqs"], p["aln_start"], p["aln_end"], p["max_aln"], p["min_len_aln"],
                                                    p["max_cov_aln"], p["min_cov_base"], p["max_lq"], p["ratio"], p["split"],
                                                    p["fast"], p["read_type"])
            os.write(wr, json.dumps([ln, float(ide) if ln > 4 else 0.0, (seq or b"").decode()]).encode())
        finally:
            os._exit(0)
    os.close(wr)
    blob = b""
    while True:
        part = os.read(rd, 1 << 20)
        if not part:
            break
        blob += part
    os.close(rd)
    _, status = os.waitpid(pid, 0)
    if os.WIFSIGNALED(status):
        return signal.Signals(os.WTERMSIG(status)).name
    ln, ide, seq = json.loads(blob)
    return ln, ide, seq.encode()


bad = []
piles = util.load_edge_piles()
for p in piles:
    r = ask(p)
    w = "%%s: the reference died (%%s)" %% (p["tag"], r) if isinstance(r, str) else util.edge_wrong(p, r)
    bad += [w] if w else []
for p in util.load_edge_piles(died=True):
    r = ask(p)
    if r != p["signal"]:
        bad.append("%%s: the reference died of %%s when the fixture was made, now %%r" %% (p["tag"], p["signal"], r if isinstance(r, str) else r[0]))
print(json.dumps(dict(bad=bad, n=len(piles))))
"""


@pytest.mark.skipif(not refpipe.have_ref("nextcorrect.so"), reason="the reference is not built (make -C oracle ref)")
def test_fixture_equals_the_live_reference(piles):
    """The fixture cannot drift: where the reference is built, its answers are the recorded ones, and it still dies where it died.
    (In a process of its own: the forks per case start from one that has loaded neither the interpreter nor the device runtime.)"""
    r = json.loads(run_child(_REF_CHILD, []).stdout.strip().splitlines()[-1])
    assert r["bad"] == [] and r["n"] == len(piles), r


def test_where_the_reference_dies_the_product_answers_with_a_status():
    """min_len_aln larger than the seed: the seed is not in its own pile and the reference walks off its tables (SIGSEGV).  The
    product returns a status (len <= 4) and the process lives -- in a child, so that `lives` is something this test can see."""
    died = util.load_edge_piles(died=True)
    assert len(died) >= 2 and all(len(p["seqs"][0]) < p["min_len_aln"] for p in died)
    code = r"""
import ctypes as C, sys
sys.path[:0] = [%r, %r, %r]
import util, build_simt
fn, fr = util.bind_correct(C.CDLL(build_simt.build()))
for p in util.load_edge_piles(died=True):
    ln, _, _ = util.call_correct(fn, fr, p, **util.edge_args(p))
    print(p["tag"], ln)
""" % (os.path.dirname(HERE), HERE, os.path.join(HERE, "simt"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NDGPU_CONTEXTS="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(died) and all(int(ln.rsplit(" ", 1)[1]) <= 4 for ln in lines), lines
