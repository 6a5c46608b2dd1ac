#!/usr/bin/env python
"""Generate tests/golden/rank_piles.npz: piles whose low-quality regions take the TAIL pass of the 8-mer candidate ranking
(lib/nextcorrect.c:405-440), with the REAL reference's answers.

Run in the build container (needs the reference compiled into oracle/_ref by `make -C oracle ref` and the interpreted kernel
library of tests/simt):

    python tests/golden/make_rank_piles_golden.py            # writes the fixture, prints what the device ranking met
    python tests/golden/make_rank_piles_golden.py --check    # builds everything again and compares with the committed arrays

No other fixture reaches the tail pass: the ranking takes it only when the best candidate of a region is longer than 500 bases, or
longer than 200 and scores below 200, and the regions of piles.npz and edge_piles.npz are short.  The piles here give every read
an insertion the seed does not have: a random 3,000-base truth, the seed a noisy copy of it, every read a noisy copy of the truth
with `ins` extra bases -- the same for all reads, so that the candidates agree -- at column 1,500, over the full window.  ONT and
CLR, ins 30, 45, 210 and 320 with 6, 9 (two piles each) and 45 reads, default arguments.  A pile the reference answers with a
status is left out (a few of the shallow ones; from about 450 inserted bases on, all of them).

Layout and recipe: those of make_edge_piles_golden.py (2-bit packed reads stored once, `rec_read` per record, per pile the arguments
and the reference's len / identity / sequence; the reference runs in a forked child per case).  The file holds data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_edge_piles_golden as E  # noqa: E402
import refpipe  # noqa: E402

OUT = os.path.join(HERE, "rank_piles.npz")
INS = (30, 45, 210, 320)
READS = (6, 9, 45)


def rank_pile(prof, ins, n_reads, seed, rep=0):
    rng = np.random.default_rng(seed)
    L = 3000
    truth = rng.integers(0, 4, L, dtype=np.uint8)
    extra = rng.integers(0, 4, ins, dtype=np.uint8)
    s = E.noisy(truth, prof, seed + 1)
    with_ins = np.concatenate([truth[:1500], extra, truth[1500:]])
    seqs, st, en = [E.asc(s)], [0], [s.size - 1]
    for i in range(n_reads):
        seqs.append(E.asc(E.noisy(with_ins, prof, seed * 1000 + i)))
        st.append(0)
        en.append(s.size - 1)
    return E.make_case("rank/%s/ins%d/reads%d/%d" % (prof, ins, n_reads, rep), seqs, st, en, prof)


def cases():
    out = []
    for pi, prof in enumerate(("ont", "clr")):
        for ins in INS:
            for n in READS:
                for rep in range(1 if n > 9 else 2):   # (the small piles twice: they are what the interpreter can run)
                    out.append(rank_pile(prof, ins, n, 9000 + 1000 * rep + 100 * pi + ins + n, rep))
    return out


def build_arrays():
    code_of = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code_of[ch] = i
    pool, packed, lens = {}, [], []

    def read_index(s):
        if s not in pool:
            c = code_of[np.frombuffer(s, dtype=np.uint8)]
            assert c.max(initial=0) < 4
            pool[s] = len(packed)
            packed.append(E.pack2(c))
            lens.append(len(s))
        return pool[s]

    keys = ("pile_off", "rec_read", "aln_start", "aln_end", "max_aln", "max_lq", "read_type", "fast", "split", "min_len_aln",
            "max_cov_aln", "min_cov_base", "ratio", "tag")
    t = {k: [0] if k == "pile_off" else [] for k in keys}
    exp = {"exp_len": [], "exp_ide": [], "exp_seq": []}
    for c in cases():
        ref = E.answer(c)
        assert not isinstance(ref, str), "the reference died on %s: %s" % (c["tag"], ref)
        if ref[0] <= 4:   # (a few of the shallow piles: nothing of the seed is corrected)
            print("  %-28s reference: status %d -- left out" % (c["tag"], ref[0]), flush=True)
            continue
        for s in c["seqs"]:
            t["rec_read"].append(read_index(s))
        t["pile_off"].append(t["pile_off"][-1] + len(c["seqs"]))
        t["aln_start"] += c["aln_start"]
        t["aln_end"] += c["aln_end"]
        for k in keys[4:]:
            t[k].append(c[k])
        exp["exp_len"].append(ref[0])
        exp["exp_ide"].append(ref[1])
        exp["exp_seq"].append(np.frombuffer(ref[2], dtype=np.uint8))
        print("  %-28s reference: %d bases" % (c["tag"], ref[0]), flush=True)
    dt = dict(pile_off=np.int64, rec_read=np.int32, aln_start=np.uint32, aln_end=np.uint32, max_aln=np.uint32, max_lq=np.uint32,
              read_type=np.int32, fast=np.int32, split=np.int32, min_len_aln=np.uint32, max_cov_aln=np.uint32, min_cov_base=np.uint32,
              ratio=np.float32, tag=np.str_)
    arrays = {k: np.asarray(t[k], dtype=dt[k]) for k in keys}
    off = np.zeros(len(packed) + 1, dtype=np.int64)
    np.cumsum([a.size for a in packed], out=off[1:])
    eoff = np.zeros(len(exp["exp_seq"]) + 1, dtype=np.int64)
    np.cumsum([a.size for a in exp["exp_seq"]], out=eoff[1:])
    arrays.update(codes=np.concatenate(packed), codes_off=off, lens=np.asarray(lens, dtype=np.int32),
                  exp_len=np.asarray(exp["exp_len"], dtype=np.uint32), exp_ide=np.asarray(exp["exp_ide"], dtype=np.float32),
                  exp_seq=np.concatenate(exp["exp_seq"]), exp_seq_off=eoff)
    return arrays


def main():
    assert refpipe.have_ref("nextcorrect.so"), "build the reference first: make -C oracle ref"
    arrays = build_arrays()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(arrays), (sorted(old.files), sorted(arrays))
        for k, v in arrays.items():
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v), "array %s differs from the committed fixture" % k
        print("%s: the same %d arrays" % (os.path.basename(OUT), len(arrays)))
        return
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("%s: %d piles, %d reads, %d bytes" % (os.path.basename(OUT), arrays["tag"].size, arrays["lens"].size, size))
    assert size <= 1 << 20, "larger than a committed file may be"
    # what the device ranking meets on the small piles (the interpreted library; tests/test_zz_gpu_rank.py asserts the whole fixture)
    import rank_util
    r = rank_util.child("simt", "piles", "rank", 9, NDGPU_RANK_DEVICE="1")
    print("piles of <= 9 reads on the interpreted library: %d piles, wrong %s, regions ranked %d, tail passes %d"
          % (r["n"], r["bad"], r["stats"]["rank_jobs"], r["stats"]["rank_tail"]))
    assert r["bad"] == [] and r["stats"]["rank_tail"] > 0


if __name__ == "__main__":
    main()
