"""Shared by tests/test_simt_poa_resident.py and tests/test_zz_gpu_poa_resident.py: the fixture of the resident POA graphs
(tests/golden/poa_resident.npz from make_poa_resident_golden.py -- inputs and outputs of the compiled reference's poa_to_consensus, the
bytes stored as bytes), the 64-sequence problem the reference cannot take, and the child process that asks the flags entry."""
import json
import os
import subprocess
import sys

import numpy as np

import poa_util
import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_CACHE = {}
OVER_BOUND = 65535   # a problem whose sum(len + 1) exceeds this does not take the resident path


def load():
    """[(sequences as bytes, the reference's consensus)]; read once."""
    if "cases" not in _CACHE:
        d = np.load(os.path.join(util.GOLD, "poa_resident.npz"))
        cases, k = [], 0
        for i, n in enumerate(d["count"]):
            seqs = []
            for _ in range(int(n)):
                seqs.append(d["seq"][d["seq_off"][k]:d["seq_off"][k + 1]].tobytes())
                k += 1
            cases.append((seqs, d["res"][d["res_off"][i]:d["res_off"][i + 1]].tobytes()))
        _CACHE["cases"] = cases
    return _CACHE["cases"]


def bound(seqs):
    return sum(len(s) + 1 for s in seqs)


def cases(max_len=None, over_bound=False):
    """The fixture's cases; over_bound=False leaves out the ones beyond the node bound."""
    out = [c for c in load() if over_bound or bound(c[0]) <= OVER_BOUND]
    if max_len is not None:
        out = [c for c in out if max(len(s) for s in c[0]) <= max_len]
    return out


def many_sequences(n=64):
    """n light variants of one 40-base sequence over ACGTNR: label bit n - 1, and with 64 the nseq >= 64 mask.  The reference takes at
    most 50 sequences (lib/dag.c:17, 666), so this problem has no reference answer: the tests take the library's host routine."""
    rng = np.random.default_rng(6464)
    letters = b"ACGTNR"
    a = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, 40))
    out = [a]
    for j in range(n - 1):
        m = bytearray(a)
        for _ in range(j % 4):
            m[int(rng.integers(0, 40))] = letters[int(rng.integers(0, 6))]
        out.append(bytes(m))
    return out


# ---- child process: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, poa_util, poa_resident_util as pr
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
POA = ("poa_jobs", "poa_declined", "poa_rounds", "poa_launches", "poa_resident_jobs", "poa_resident_declined", "poa_graph_launches",
       "poa_h2d_bytes", "poa_d2h_bytes")
def leg(jobs, **kw):
    api.reset_stats()
    got = api.poa_batch(jobs, **kw)
    st = api.stats()
    return got, {k: st[k] for k in POA}
if what == "resident":          # the fixture's cases: the variable's choice in one call and singly, then every flag
    cases = pr.cases(int(sys.argv[3]))
    jobs, want = [c[0] for c in cases], [c[1] for c in cases]
    out = dict(n=len(cases))
    for name, kw in (("env", {}), ("resident", dict(resident=True)), ("rounds", dict(resident=False)), ("host", dict(host=True))):
        got, st = leg(jobs, **kw)
        out[name] = dict(bad=[i for i in range(len(cases)) if got[i] != want[i]], stats=st)
    api.reset_stats()
    one = [api.poa_batch([j])[0] for j in jobs]
    out["singly"] = dict(bad=[i for i in range(len(cases)) if one[i] != want[i]], stats={k: api.stats()[k] for k in POA})
    print(json.dumps(out))
elif what == "mixed":           # jobs of 2 and of 6 sequences in turn, and the 64-sequence problem: some leave the rounds early
    fx = [c for c in poa_util.fixtures(int(sys.argv[3])) + pr.cases(int(sys.argv[3]))]
    two, six = [c for c in fx if len(c[0]) == 2], [c for c in fx if len(c[0]) == 6]
    mix = [c for pair in zip(two, six) for c in pair]
    many = pr.many_sequences(64)
    jobs = [c[0] for c in mix] + [many]
    want = [c[1] for c in mix] + api.poa_batch([many], host=True)
    got, st = leg(jobs)
    print(json.dumps(dict(n_two=len(two), n_six=len(six), n=len(jobs), bad=[i for i in range(len(jobs)) if got[i] != want[i]], stats=st,
                          many_len=len(want[-1]))))
elif what == "args":            # the flags entry's argument errors: nothing written
    lib = api.load()
    cs = (C.c_char_p * 1)(b"ACGT")
    ln = (C.c_uint16 * 1)(4)
    arr = (api.PoaJob * 1)(api.PoaJob(C.cast(cs, C.POINTER(C.c_char_p)), C.cast(ln, C.POINTER(C.c_uint16)), 1))
    rcs = {}
    for flags in (6, 7, 8, 16, 1 << 20, -1, 0, 1, 2, 4):
        out = (C.c_void_p * 1)(0xdead)
        rc = lib.ndgpu_poa_batch_flags(arr, 1, flags, out)
        rcs[str(flags)] = [rc, out[0] == 0xdead, C.string_at(out[0]).decode() if rc == 0 else None]
    print(json.dumps(dict(rc=rcs, empty=lib.ndgpu_poa_batch_flags(None, 0, 2, None))))
"""


def child(lib, what, *args, timeout=1500, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("NDGPU_POA")}   # no switch of the caller's reaches the child
    e.update(env)
    if lib == "simt":
        e.setdefault("NDGPU_CONTEXTS", "1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE, os.path.join(HERE, "simt")), lib, what, *[str(a) for a in args]],
                         env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])
