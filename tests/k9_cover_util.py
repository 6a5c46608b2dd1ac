"""What tests/test_simt_k9_compact.py and tests/test_gpu_k9_compact.py share: the piles of tests/golden/cover_piles.npz
(tests/golden/make_cover_piles_golden.py made it and says what they are), the child program that runs them, and the checks on
what the child reports.  Every call into the library is made in a child process: NDGPU_K9_COMPACT is read once per process, and a
kernel that walks off its tables then fails the test with the pile's name instead of taking pytest along."""
import json
import os
import re
import subprocess
import sys

import numpy as np

import util

HERE = os.path.dirname(os.path.abspath(__file__))
LIMITS = (None, 0, 1, 32, 63, 64)          # NDGPU_K9_COMPACT: unset, and the values the limit is tested at
STAIRS = ("stair/ont", "stair/clr", "stair/hifi", "stair/clr,read_type=ont", "stair/hifi,read_type=ont")
ONE_CALL = ("stair/ont", "stair/clr,read_type=ont", "stair/hifi,read_type=ont", "flat/65", "flat/64")   # one read type: one batched call
TRACE = re.compile(r"\[ndgpu trace\] K9 blocks: compact (\d+) \(max cover (\d+)\), fallback (\d+) \(min cover (\d+)\)")


def load_cover_piles():
    """The piles of cover_piles.npz, as util.load_edge_piles() gives those of edge_piles.npz."""
    d = np.load(os.path.join(util.GOLD, "cover_piles.npz"))
    cache = {}

    def read(r):
        if r not in cache:
            cache[r] = util.ASC[util.unpack2(d["codes"][d["codes_off"][r]:d["codes_off"][r + 1]], int(d["lens"][r]))].tobytes()
        return cache[r]

    piles, off = [], d["pile_off"]
    for p in range(off.size - 1):
        a, b = int(off[p]), int(off[p + 1])
        piles.append(dict(tag=str(d["tag"][p]), seqs=[read(int(r)) for r in d["rec_read"][a:b]],
                          aln_start=[int(x) for x in d["aln_start"][a:b]], aln_end=[int(x) for x in d["aln_end"][a:b]],
                          max_aln=int(d["max_aln"][p]), max_lq=int(d["max_lq"][p]), read_type=int(d["read_type"][p]),
                          fast=int(d["fast"][p]), split=int(d["split"][p]), min_len_aln=int(d["min_len_aln"][p]),
                          max_cov_aln=int(d["max_cov_aln"][p]), min_cov_base=int(d["min_cov_base"][p]), ratio=float(d["ratio"][p]),
                          exp_len=int(d["exp_len"][p]), exp_ide=float(d["exp_ide"][p]),
                          exp_seq=d["exp_seq"][d["exp_seq_off"][p]:d["exp_seq_off"][p + 1]].tobytes()))
    return piles


# argv: simt | native, each | batch | orders.  stdout: BEGIN lines and one JSON line; stderr: "PILE <tag>" before every call, so that
# the trace lines that follow belong to it.
CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%r, %r, %r]
import util, k9_cover_util as K
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    lib = C.CDLL(build_simt.build())
    api._LIB = api._bind(lib)
else:
    lib = api.load()
fn, fr = util.bind_correct(lib)
piles = K.load_cover_piles()
mode = sys.argv[2]
if mode == "orders":              # lanes of a wavefront highest first, the lowest wavefront runs ahead
    lib.simt_set_lane_order(1)
    lib.simt_set_schedule(1)
    piles = [p for p in piles if p["tag"] == "stair/ont"]
if mode == "batch":
    members = [p for t in K.ONE_CALL for p in piles if p["tag"] == t]
    key = util.edge_group_key(members[0])
    assert all(util.edge_group_key(p) == key for p in members)
    print("BEGIN the batched call", flush=True)
    got = util.edge_correct_group(api, key, members)
else:
    members, got = piles, []
    for p in piles:
        print("BEGIN", p["tag"], flush=True)
        print("PILE", p["tag"], file=sys.stderr, flush=True)
        got.append(util.call_correct(fn, fr, p, **util.edge_args(p)))
bad = [w for w in (util.edge_wrong(p, r) for p, r in zip(members, got)) if w]
print(json.dumps(dict(bad=bad, tags=[p["tag"] for p in members], got=[[r[0], float(r[1]).hex(), r[2].decode()] for r in got])))
"""


def run_child(which, mode, limit, timeout, **env):
    """-> (the child's JSON, {tag: (compact, max cover, fallback, min cover) of the pile's first K9 attempt})"""
    keep = ("NDGPU_K9", "NDGPU_K10") if which == "native" else ("NDGPU_",)      # no force switch reaches the child
    e = {k: v for k, v in os.environ.items() if not k.startswith(keep)}
    e.update(NDGPU_TRACE="1")
    if which == "simt":
        e.update(NDGPU_CONTEXTS="1")
    if limit is not None:
        e.update(NDGPU_K9_COMPACT=str(limit))
    e.update(env)
    code = CHILD % (os.path.dirname(HERE), HERE, os.path.join(HERE, "simt"))
    out = subprocess.run([sys.executable, "-c", code, which, mode], env=e, capture_output=True, text=True, timeout=timeout)
    begun = [ln[6:] for ln in out.stdout.splitlines() if ln.startswith("BEGIN ")]
    assert out.returncode == 0, "the child ended with status %d in %s\n%s" % (out.returncode, begun[-1] if begun else "its start", out.stderr[-3000:])
    assert "FATAL" not in out.stderr
    trace, tag = {}, None
    for ln in out.stderr.splitlines():
        if ln.startswith("PILE "):
            tag = ln[5:]
        m = TRACE.search(ln)
        if m and tag is not None and tag not in trace:
            trace[tag] = tuple(int(x) for x in m.groups())
    return json.loads(out.stdout.strip().splitlines()[-1]), trace


def check_each(r, trace, limit, piles):
    """Every pile in a call of its own: the reference's answer, whatever the limit; and the counters add up."""
    assert r["bad"] == [], r["bad"]
    assert r["tags"] == [p["tag"] for p in piles] and len(piles) == 7
    for p in piles:
        compact, cmax, deep, dmin = trace[p["tag"]]
        assert compact + deep == (len(p["seqs"][0]) + 31) // 32, (p["tag"], trace[p["tag"]])      # every block took one of the two ways
        lim = 64 if limit is None else limit
        assert cmax <= lim and (deep == 0 or dmin > lim), (p["tag"], limit, trace[p["tag"]])


def check_trace(by_limit):
    """by_limit: {limit: trace}.  Blocks with exactly 64 and exactly 65 covering reads exist and land on the right side."""
    for tag in STAIRS:
        t = {lim: by_limit[lim][tag] for lim in LIMITS}
        assert t[0][0] == 0 and t[0][2] == 75, (tag, t[0])                        # T = 0: no block goes compact
        compact, cmax, deep, dmin = t[None]
        assert compact > 0 and deep > 0 and cmax == 64 and dmin == 65, (tag, t[None])
        assert t[64] == t[None], (tag, t[64], t[None])                            # the default IS 64
        assert t[64][0] > t[63][0] > t[32][0] > t[1][0] == 0, (tag, t)
    # the seed and 64 reads: 65 on every block, none compact; the seed and 63: every block compact, at exactly 64
    assert by_limit[None]["flat/65"] == (0, 0, 32, 65), by_limit[None]["flat/65"]
    assert by_limit[None]["flat/64"] == (32, 64, 0, 0), by_limit[None]["flat/64"]
    assert by_limit[63]["flat/64"] == (0, 0, 32, 64), by_limit[63]["flat/64"]


def check_batch(default, zero, piles):
    """The five piles of ONE_CALL in one batched call: default limit and limit 0 answer alike, and as the reference did."""
    assert default["bad"] == [] and zero["bad"] == [], (default["bad"], zero["bad"])
    assert default["tags"] == list(ONE_CALL) == zero["tags"]
    assert default["got"] == zero["got"]
