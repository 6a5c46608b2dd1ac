"""What tests/test_simt_k9_rows.py and tests/test_gpu_k9_rows.py share: the piles of tests/golden/k9_rows.npz
(tests/golden/make_k9_rows_golden.py made it and says what they are), the child program that runs them, and the checks on what
the child reports.  Every call into the library is made in a child process, as in tests/k9_cover_util.py: NDGPU_K9_COMPACT and
NDGPU_K9_DIGEST are read once per process."""
import json
import os
import re
import subprocess
import sys

import numpy as np

import util

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ("fan", "spread", "thin")
BLOCKS = re.compile(r"\[ndgpu trace\] K9 blocks: compact (\d+) \(max cover (\d+)\), fallback (\d+) \(min cover (\d+)\)")
TABLES = re.compile(r"\[ndgpu trace\] K9 tables: digest=([0-9a-f]{16}) cells=(\d+) links=(\d+) max_cell_len=(\d+)")


def load_piles():
    """The piles of k9_rows.npz, as util.load_edge_piles() gives those of edge_piles.npz."""
    d = np.load(os.path.join(util.GOLD, "k9_rows.npz"))
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


# argv: simt | native.  Every pile in a call of its own, then all of them in one batched call.  stderr: "PILE <tag>" before every
# call ("PILE batch" before the batched one), so that the trace lines that follow belong to it.  stdout: BEGIN lines and one JSON line.
CHILD = r"""
import ctypes as C, json, sys
sys.path[:0] = [%r, %r, %r]
import util, k9_rows_util as K
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    lib = C.CDLL(build_simt.build())
    api._LIB = api._bind(lib)
else:
    lib = api.load()
fn, fr = util.bind_correct(lib)
piles = K.load_piles()
bad = []
for p in piles:
    print("BEGIN", p["tag"], flush=True)
    print("PILE", p["tag"], file=sys.stderr, flush=True)
    bad.append(util.edge_wrong(p, util.call_correct(fn, fr, p, **util.edge_args(p))))
key = util.edge_group_key(piles[0])
assert all(util.edge_group_key(p) == key for p in piles)
print("BEGIN the batched call", flush=True)
print("PILE batch", file=sys.stderr, flush=True)
bad += [util.edge_wrong(p, r) for p, r in zip(piles, util.edge_correct_group(api, key, piles))]
print(json.dumps(dict(bad=[w for w in bad if w], tags=[p["tag"] for p in piles])))
"""


def run_child(which, limit, timeout):
    """-> (the child's JSON, {tag | "batch": ((compact, max cover, fallback, min cover), (digest, cells, links, max_cell_len)) of the
    call's first K9 attempt})"""
    keep = ("NDGPU_K9", "NDGPU_K10") if which == "native" else ("NDGPU_",)      # no force switch reaches the child
    e = {k: v for k, v in os.environ.items() if not k.startswith(keep)}
    e.update(NDGPU_TRACE="1", NDGPU_K9_DIGEST="1", NDGPU_CONTEXTS="1")      # (one context: the batched call is one sub-batch)
    if limit is not None:
        e.update(NDGPU_K9_COMPACT=str(limit))
    code = CHILD % (os.path.dirname(HERE), HERE, os.path.join(HERE, "simt"))
    out = subprocess.run([sys.executable, "-c", code, which], env=e, capture_output=True, text=True, timeout=timeout)
    begun = [ln[6:] for ln in out.stdout.splitlines() if ln.startswith("BEGIN ")]
    assert out.returncode == 0, "the child ended with status %d in %s\n%s" % (out.returncode, begun[-1] if begun else "its start", out.stderr[-3000:])
    assert "FATAL" not in out.stderr
    blocks, tables, tag = {}, {}, None
    for ln in out.stderr.splitlines():
        if ln.startswith("PILE "):
            tag = ln[5:]
        m = BLOCKS.search(ln)
        if m and tag is not None and tag not in blocks:
            blocks[tag] = tuple(int(x) for x in m.groups())
        m = TABLES.search(ln)
        if m and tag is not None and tag not in tables:
            tables[tag] = (m.group(1),) + tuple(int(x) for x in m.groups()[1:])
    return json.loads(out.stdout.strip().splitlines()[-1]), {t: (blocks[t], tables[t]) for t in TAGS + ("batch",)}


def check(default, zero, piles):
    """default, zero: run_child() with NDGPU_K9_COMPACT unset and 0.  The reference's answers either way, every block on the compact
    path when the switch is unset and none at 0, the same tables from both paths, and the fan's cell is as full as it was built."""
    assert [p["tag"] for p in piles] == list(TAGS)
    for r, _ in (default, zero):
        assert r["bad"] == [], r["bad"]
        assert r["tags"] == list(TAGS)
    n_blocks = {p["tag"]: (len(p["seqs"][0]) + 31) // 32 for p in piles}
    n_blocks["batch"] = sum(n_blocks.values())
    for tag in TAGS + ("batch",):
        (compact, cmax, deep, _), tab = default[1][tag]
        assert (compact, deep) == (n_blocks[tag], 0) and 1 <= cmax <= 64, (tag, default[1][tag])
        (compact0, _, deep0, _), tab0 = zero[1][tag]
        assert (compact0, deep0) == (0, n_blocks[tag]), (tag, zero[1][tag])
        assert tab == tab0, (tag, tab, tab0)
        assert tab[1] > 0 and tab[2] > 0
    assert default[1]["fan"][0][1] == 64                  # every lane of the wavefront holds a read
    assert default[1]["fan"][1][3] >= 48, default[1]["fan"]   # one cell with 48 or more distinct links
    assert default[1]["batch"][1][3] == default[1]["fan"][1][3]
    assert default[1]["thin"][0][1] == 2
    # the batched call's tables are the three piles' tables
    assert default[1]["batch"][1][1] == sum(default[1][t][1][1] for t in TAGS)
    assert default[1]["batch"][1][2] == sum(default[1][t][1][2] for t in TAGS)
