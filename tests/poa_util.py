"""Shared by tests/test_simt_poa.py and tests/test_zz_gpu_poa.py: the POA fixtures (tests/golden/poa.npz from make_golden.py,
tests/golden/poa_device.npz from make_poa_device_golden.py -- inputs and outputs of the compiled reference's poa_to_consensus),
a fuzz generator, and the child processes that run the batched device POA (api.poa_batch) and the engine (api.correct_batch) under
the switches that are read once per process."""
import json
import os
import subprocess
import sys

import numpy as np

import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_CACHE = {}


def load(name):
    """[(sequences as bytes, the reference's consensus)] of one fixture; read once."""
    if name not in _CACHE:
        d = np.load(os.path.join(util.GOLD, name))
        cases, k = [], 0
        for i, n in enumerate(d["count"]):
            seqs = []
            for _ in range(int(n)):
                seqs.append(util.ASC[d["seq"][d["seq_off"][k]:d["seq_off"][k + 1]]].tobytes())
                k += 1
            cases.append((seqs, d["res"][d["res_off"][i]:d["res_off"][i + 1]].tobytes()))
        _CACHE[name] = cases
    return _CACHE[name]


def fixtures(max_len=None):
    cases = load("poa.npz") + load("poa_device.npz")
    if max_len is not None:
        cases = [c for c in cases if max(len(s) for s in c[0]) <= max_len]
    return cases


def fuzz_jobs(n, seed=2024, max_len=600):
    """2-6 sequences of 1..max_len bases per job, three error profiles, every ninth job over a two-letter alphabet."""
    from nextdenovo_amd import synth
    rng = np.random.default_rng(seed)
    jobs = []
    for it in range(n):
        L = int(rng.integers(1, max_len + 1))
        base = rng.integers(0, 2 if it % 9 == 8 else 4, L, dtype=np.uint8)
        prof = ("ont", "clr", "hifi")[it % 3]
        k = int(rng.integers(2, 7))
        seqs = [synth.mutate(base, np.random.default_rng([seed, it, j]), prof)[0][:max_len] for j in range(k)]
        seqs = [util.ASC[s].tobytes() for s in seqs if s.size > 0]
        while len(seqs) < 2:
            seqs.append(util.ASC[base].tobytes())
        jobs.append(seqs)
    return jobs


def host_poa(lib, seqs):
    """The library's own host poa_to_consensus (struct seq_ records, lib/nextcorrect.h:63-68)."""
    import ctypes as C
    stride = 6 + 10000
    lib.poa_to_consensus.argtypes = [C.c_void_p, C.c_int]
    lib.poa_to_consensus.restype = C.c_void_p
    buf = C.create_string_buffer(stride * len(seqs))
    for j, a in enumerate(seqs):
        C.memmove(C.addressof(buf) + j * stride + 4, np.uint16(len(a)).tobytes(), 2)
        C.memmove(C.addressof(buf) + j * stride + 6, a + b"\0", len(a) + 1)
    p = lib.poa_to_consensus(C.addressof(buf), len(seqs))
    res = C.string_at(p)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p)
    return res


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, poa_util
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
if what == "fixtures":          # every case in one call and one by one
    cases = poa_util.fixtures(int(sys.argv[3]) if len(sys.argv) > 3 else None)
    got = api.poa_batch([c[0] for c in cases])
    one = [api.poa_batch([c[0]])[0] for c in cases]
    bad = [i for i, c in enumerate(cases) if got[i] != c[1] or one[i] != c[1]]
    print(json.dumps(dict(bad=bad, n=len(cases), stats=api.stats())))
elif what == "piles":           # the golden piles through correct_batch, grouped by the arguments a call takes once
    piles = util.load_piles()
    groups = {}
    for i, p in enumerate(piles):
        groups.setdefault((p["read_type"], p["fast"], p["split"]), []).append(i)
    rec = [None] * len(piles)
    for (rt, fast, split), ids in groups.items():
        res = api.correct_batch([(piles[i]["seqs"], piles[i]["aln_start"], piles[i]["aln_end"], piles[i]["max_aln"], piles[i]["max_lq"]) for i in ids],
                                split=split, fast=fast, read_type=rt, host_threads=4)
        for i, (ln, ide, seq) in zip(ids, res):
            rec[i] = [int(ln), int(np.float32(ide).view(np.uint32)), seq.decode()]
    bad = [i for i, p in enumerate(piles) if rec[i][0] != p["exp_len"] or (rec[i][0] > 4 and (rec[i][2].encode() != p["exp_seq"] or
           rec[i][1] != int(np.float32(p["exp_ide"]).view(np.uint32))))]
    print(json.dumps(dict(rec=rec, bad=bad, groups=len(groups), stats=api.stats())))
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
