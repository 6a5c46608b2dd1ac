#!/usr/bin/env python
"""Generate tests/golden/poa_resident.npz from the REAL reference's poa_to_consensus() (lib/dag.c:658-694): the directed cases that
pin the resident POA graphs (K19, NDGPU_POA_RESIDENT=1 / ndgpu_poa_batch_flags) and that poa.npz and poa_device.npz lack -- letters
outside ACGT, columns of more than four nodes, start and tail chains, sequences that add no node, row counts around the wavefront,
50 sequences (the reference's limit), and a problem over the node bound.  Same arrays as poa.npz (make_golden.py), but `seq` holds the bytes themselves.

Run in the build container (needs the reference compiled into oracle/_ref by `make -C oracle ref`):

    python tests/golden/make_poa_resident_golden.py

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

LETTERS = b"ACGTNR"


def rand_seq(rng, n, letters=b"ACGT"):
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), n))


def cases():
    rng = np.random.default_rng(1919)
    out = []
    for n in range(2, 7):                                   # 2 to 6 sequences of 1, 2 and 3 bases
        for L in (1, 2, 3):
            a = rand_seq(rng, L)
            out.append([a] * n)                             # equal
            out.append([bytes(LETTERS[(j + k) % 6] for k in range(L)) for j in range(n)])   # different at every position
    out.append([bytes([c]) * 12 for c in LETTERS])          # six single-letter sequences: columns of six nodes
    for L, p in ((5, 3), (70, 40)):                         # a strict prefix / suffix of the first: start chain, tail chain + NUL node
        a = rand_seq(rng, L)
        out.append([a, a[:p]])
        out.append([a, a[-p:]])
        out.append([a, a[:p], a[-p:]])
    a = rand_seq(rng, 50)
    out.append([a] * 3)                                     # no new node, labels only
    out.append([a] * 6)
    for L in (63, 64, 65, 128, 129):                        # row counts around the wavefront: one substitution, one deletion, one insertion
        a = rand_seq(rng, L)
        m = bytearray(a)
        m[L // 3] = ord("N")
        del m[L // 2]
        m.insert(2 * L // 3, ord("R"))
        out.append([a, bytes(m)])
    a = rand_seq(rng, 80)
    out.append([a, rand_seq(rng, 20) + a])                  # a 20-base insertion at the front: the leading unmatched run
    out.append([a, b"N" * 20 + a, a])
    out.append([a, a[:-20]])                                # a 20-base deletion at the end
    out.append([a, a[:-20], a])
    a = rand_seq(rng, 40)                                   # 50 sequences, the most the reference takes (lib/dag.c:17, 666); the tests
    many = [a]                                              # build a 64-sequence problem themselves (tests/poa_resident_util.py)
    for j in range(49):
        m = bytearray(a)
        for _ in range(j % 4):
            m[int(rng.integers(0, 40))] = LETTERS[int(rng.integers(0, 6))]
        many.append(bytes(m))
    out.append(many)
    out.append([b"A" * 9999] * 7)                           # node bound 70,000 > 65,535
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
        for j, a in enumerate(seqs):
            C.memmove(C.addressof(buf) + j * stride + 4, np.uint16(len(a)).tobytes(), 2)
            C.memmove(C.addressof(buf) + j * stride + 6, a + b"\0", len(a) + 1)
        p = lib.poa_to_consensus(C.addressof(buf), len(seqs))
        r = np.frombuffer(C.string_at(p), dtype=np.uint8)
        libc.free(p)
        cnt.append(len(seqs))
        for a in seqs:
            flat.append(np.frombuffer(a, dtype=np.uint8))
            off.append(off[-1] + len(a))
        res.append(r)
        reso.append(reso[-1] + r.size)
    np.savez_compressed(os.path.join(HERE, "poa_resident.npz"), seq=np.concatenate(flat), seq_off=np.asarray(off),
                        count=np.asarray(cnt), res=np.concatenate(res), res_off=np.asarray(reso))
    print("poa_resident: %d cases, %d bases" % (len(cnt), off[-1]))


if __name__ == "__main__":
    main()
