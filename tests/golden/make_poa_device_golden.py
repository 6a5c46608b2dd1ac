#!/usr/bin/env python
"""Generate tests/golden/poa_device.npz from the REAL reference's poa_to_consensus() (lib/dag.c:658-694): the cases that pin the
batched device POA (ndgpu_poa_batch) -- row lengths around the 64-lane chunk, identical sequences, head and tail chains, score
ties, rows of many chunks and the workgroup form.  Same record format as poa.npz (make_golden.py).

Run in the build container (needs the reference compiled into oracle/_ref by `make -C oracle ref`):

    python tests/golden/make_poa_device_golden.py

Seeded and deterministic; the GPU box reads only the fixture.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refpipe  # noqa: E402
from nextdenovo_amd import synth  # noqa: E402

ASC = np.frombuffer(b"ACGT", dtype=np.uint8)
LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)
PROFILES = ("ont", "clr", "hifi")


def jitter(base, rng, n_del, n_dup):
    """A copy with bases dropped and doubled, over the alphabet of `base` itself (synth.mutate substitutes from all four)."""
    s = list(base)
    for _ in range(n_del):
        if len(s) > 1:
            del s[int(rng.integers(0, len(s)))]
    for _ in range(n_dup):
        k = int(rng.integers(0, len(s)))
        s.insert(k, s[k])
    return np.asarray(s, dtype=np.uint8)


def cases():
    out = []
    ci = 0
    for L in LENGTHS:
        for prof in PROFILES:
            rng = np.random.default_rng(9000 + ci)
            base = rng.integers(0, 4, L, dtype=np.uint8)
            n = 2 + ci % 5
            seqs = [synth.mutate(base, np.random.default_rng(100000 + 100 * ci + j), prof)[0] for j in range(n)]
            seqs = [s for s in seqs if s.size > 0]
            while len(seqs) < 2:
                seqs.append(base.copy())
            out.append(seqs)
            ci += 1
    rng = np.random.default_rng(4242)
    a = rng.integers(0, 4, 120, dtype=np.uint8)
    out.append([a.copy() for _ in range(4)])                           # all sequences identical
    out.append([a, a[:40]])                                            # a later sequence that is only a prefix of the first
    out.append([a, a[-40:]])                                           # ... only a suffix
    out.append([a, a[:40], a[-40:], a, a[:1], a[-1:]])                 # head and tail chains together, the NUL-tail node
    out.append([a[:40], a, a[-40:]])                                   # the first is the short one
    h = np.zeros(30, dtype=np.uint8)
    out.append([h, np.zeros(33, dtype=np.uint8), np.zeros(28, dtype=np.uint8), h.copy(), np.zeros(64, dtype=np.uint8)])  # homopolymers
    two = rng.integers(0, 2, 90, dtype=np.uint8) * 3                   # two letters: score ties
    out.append([two] + [jitter(two, rng, 4, 4) for _ in range(4)])
    two = rng.integers(0, 2, 200, dtype=np.uint8) + 1
    out.append([jitter(two, rng, 9, 7) for _ in range(6)])
    base = rng.integers(0, 4, 1000, dtype=np.uint8)                    # rows of many chunks
    out.append([synth.mutate(base, np.random.default_rng(777 + j), "ont")[0] for j in range(6)])
    base = rng.integers(0, 4, 3100, dtype=np.uint8)                    # the workgroup form
    out.append([synth.mutate(base, np.random.default_rng(888 + j), "ont")[0] for j in range(2)])
    return out


def main():
    assert refpipe.have_ref("nextcorrect.so"), "build the reference first: make -C oracle ref"
    lib = refpipe.ref_cns()
    stride = 6 + 10000   # struct seq_ { u16 order, kscore, len; char seq[10000]; } (lib/nextcorrect.h:62-68)
    lib.poa_to_consensus.argtypes = [C.c_void_p, C.c_int]
    lib.poa_to_consensus.restype = C.c_void_p
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    flat, off, cnt, res, reso = [], [0], [], [], [0]
    for seqs in cases():
        buf = C.create_string_buffer(stride * len(seqs))
        for j, s in enumerate(seqs):
            a = ASC[s].tobytes()
            C.memmove(C.addressof(buf) + j * stride + 4, np.uint16(len(a)).tobytes(), 2)
            C.memmove(C.addressof(buf) + j * stride + 6, a + b"\0", len(a) + 1)
        p = lib.poa_to_consensus(C.addressof(buf), len(seqs))
        r = np.frombuffer(C.string_at(p), dtype=np.uint8)
        libc.free(p)
        cnt.append(len(seqs))
        for s in seqs:
            flat.append(np.asarray(s, dtype=np.uint8))
            off.append(off[-1] + s.size)
        res.append(r)
        reso.append(reso[-1] + r.size)
    np.savez_compressed(os.path.join(HERE, "poa_device.npz"), seq=np.concatenate(flat), seq_off=np.asarray(off),
                        count=np.asarray(cnt), res=np.concatenate(res), res_off=np.asarray(reso))
    print("poa_device: %d cases, %d bases" % (len(cnt), off[-1]))


if __name__ == "__main__":
    main()
