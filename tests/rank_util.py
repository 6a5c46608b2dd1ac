"""Shared by tests/test_simt_rank.py and tests/test_zz_gpu_rank.py: the 8-mer ranking of a low-quality region's candidates restated in
Python from the reference's lines (lib/nextcorrect.c:281-337 the histogram and the scores, :405-440 the program), not from the library;
directed cases and a seeded fuzz generator for the batched entry (api.lq_rank_batch); the fixture tests/golden/rank_piles.npz
(make_rank_piles_golden.py: piles whose regions take the tail pass, with the compiled reference's answers); and the child processes
that run the entry and the engine (api.correct_batch) under the switches that are read once per process."""
import json
import os
import subprocess
import sys

import numpy as np

import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KMER, RANGE, TOP, CAN_MAX = 8, 40, 10, 40          # KMER_LEN, KMER_RANGE, KMER_MAX_SEQ, LQ_CAN_MAX
_CODE = np.full(256, 4, dtype=np.uint32)           # the reference's base2int
for _ch, _v in ((b"Aa", 0), (b"Tt", 1), (b"Gg", 2), (b"Cc", 3), (b"N", 5), (b"M", 6)):
    for _c in _ch:
        _CODE[_c] = _v


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _kmers(seqs, from_tail):
    """count_kmers / count_kscore's k-mers of every sequence -> (K [n, 32] uint32, valid [n, 32]): min(len, KMER_RANGE) - KMER_LEN of
    them from offset 0, or from len - KMER_RANGE of a longer sequence's tail; km = km << 2 | code in 16 bits, as the reference rolls
    it (eight bytes to start with, one more per k-mer) -- here for all sequences of the job at once."""
    n = len(seqs)
    W = np.zeros((n, RANGE), dtype=np.uint8)
    cnt = np.zeros(n, dtype=np.int64)
    for i, s in enumerate(seqs):
        ln = len(s)
        if ln < KMER:
            continue
        off = ln - RANGE if from_tail and ln > RANGE else 0
        w = min(ln, RANGE)
        W[i, :w] = np.frombuffer(s, dtype=np.uint8, count=w, offset=off)
        cnt[i] = w - KMER
    C = _CODE[W]
    K = np.zeros((n, RANGE - KMER), dtype=np.uint32)
    km = np.zeros(n, dtype=np.uint32)
    for x in range(KMER):
        km = ((km << 2) | C[:, x]) & 0xffff
    K[:, 0] = km
    for k in range(1, RANGE - KMER):
        km = ((km << 2) | C[:, k + KMER - 1]) & 0xffff
        K[:, k] = km
    return K, np.arange(RANGE - KMER)[None, :] < cnt[:, None]


def _pass(pos, K, valid, c):
    """pos: input indices in the current order -> the scores in that order: the histogram of the first min(n, c) sequences' k-mers,
    every sequence scored with the sum of its own k-mers' bins (uint16)."""
    head = pos[:min(len(pos), c)]
    bins = np.bincount(K[head][valid[head]], minlength=65536)
    return ((bins[K[pos]] * valid[pos]).sum(axis=1) & 0xffff).astype(np.int64)


def _sort(pos, score):
    o = np.argsort(-score, kind="stable")      # glibc's qsort is a merge sort: ties keep the current order
    return pos[o], score[o]


def rank(seqs):
    """-> (order, kscore, tail, swapped): the program of lib/nextcorrect.c:405-440 on `seqs` in input order."""
    n = len(seqs)
    lens = np.asarray([len(s) for s in seqs], dtype=np.int64)
    pos = np.arange(n)
    K, valid = _kmers(seqs, 0)
    score = _pass(pos, K, valid, 1)
    pos, score = _sort(pos, score)
    score = _pass(pos, K, valid, TOP)
    kmaxlen, kmaxscore = int(lens[pos[0]]), int(score[0])
    tail = swapped = 0
    if kmaxlen > 500 or (kmaxlen > 200 and kmaxscore < 200):
        tail = 1
        if pos[0] != 0:                        # find_ref_lqseq: a swap, not a rotation
            j = int(np.nonzero(pos == 0)[0][0])
            pos[[0, j]] = pos[[j, 0]]
            score[[0, j]] = score[[j, 0]]
            swapped = 1
        saved = np.zeros(n, dtype=np.int64)
        saved[pos] = score
        K, valid = _kmers(seqs, 1)
        score = _pass(pos, K, valid, 1)
        pos, score = _sort(pos, score)
        score = _pass(pos, K, valid, TOP)
        score = (score + saved[pos]) & 0xffff
    pos, score = _sort(pos, score)
    return [int(x) for x in pos], [int(x) for x in score], tail, swapped


def want(jobs):
    return [rank(j)[:3] for j in jobs]


# ---- cases ----------------------------------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n, letters=b"ACGT"):
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes()


def _noisy(rng, base: bytes, rate=0.08):
    """A copy of base with substitutions, deletions and insertions, a third of `rate` each."""
    a = np.frombuffer(base, dtype=np.uint8).copy()
    m = rng.random(a.size) < rate / 3
    a[m] = _ACGT[rng.integers(0, 4, int(m.sum()))]
    a = np.delete(a, np.nonzero(rng.random(a.size) < rate / 3)[0])
    at = np.nonzero(rng.random(a.size) < rate / 3)[0]
    return np.insert(a, at, _ACGT[rng.integers(0, 4, at.size)]).tobytes()


def directed_cases():
    """[(name, [bytes])]; check_directed() asserts what each is for with the restatement."""
    rng = np.random.default_rng(77)
    cases = []
    for n in (1, 2, 5, 10, 11, 40):
        base = _rand(rng, 90)
        cases.append(("n=%d" % n, [_noisy(rng, base) for _ in range(n)]))
    one = _rand(rng, 60)
    cases.append(("identical", [one] * 12))
    cases.append(("homopolymer-600", [b"A" * 600] * 40))
    # input 0 unrelated to nine similar 600-base sequences.  Against input 0's own histogram input 0 scores 32 where its k-mers are
    # distinct and nothing else scores, so it stays in front; for find_ref_lqseq's swap another sequence must beat it there, which
    # takes a repeated k-mer: input 0 opens with 12 'A' (the k-mer AAAAAAAA five times: 5 x 5 + 27 = 52), the nine with 40 (32 x 5).
    base = b"A" * 40 + _rand(rng, 560)
    cases.append(("swap", [b"A" * 12 + _rand(rng, 588, b"CGT")] + [_noisy(rng, base, 0.02) for _ in range(9)]))
    # the tail condition: kmaxlen 200 | 201 and 500 | 501 with the best score on either side of 200.  Identical sequences of length
    # L score min(n, 10) x 32 each when no k-mer repeats inside a window: 6 copies 192, 7 copies 224.
    for L in (200, 201, 500, 501):
        s = _rand(rng, L)
        for n in (6, 7):
            cases.append(("tail-L%d-n%d" % (L, n), [s] * n))
    cases.append(("bytes-NM-lower", [b"ACGTNNMMacgtnm" * 5, b"acgtACGTNMNMNM" * 5, b"NNNNNNNNNNNNNNNNNNNN", b"MMMMMMMMMMMMNMNM", b"ACGTNNMMacgtnm" * 5]))
    cases.append(("bytes-noise", [bytes(rng.integers(0, 256, int(L), dtype=np.uint8)) for L in (50, 41, 40, 39, 300, 256, 8, 9, 600)]))
    cases.append(("bytes-every-value", [bytes(range(256)), bytes(range(255, -1, -1)), bytes(range(256)) * 3]))
    base = _rand(rng, 70)
    cases.append(("short-among-long", [_noisy(rng, base), b"", base[:7], base[:8], _noisy(rng, base), base[:9], b"", _noisy(rng, base)]))
    cases.append(("all-short", [b"", b"ACGTACG", b"ACGTACGT", b"A"]))
    return cases


def check_directed(cases=None):
    cases = dict(cases or directed_cases())
    got = {k: rank(v) for k, v in cases.items()}
    assert {len(cases["n=%d" % n]) for n in (1, 2, 5, 10, 11, 40)} == {1, 2, 5, 10, 11, 40}
    assert len(set(got["identical"][1])) == 1 and got["identical"][0] == list(range(12))          # every score tied: input order stays
    assert got["homopolymer-600"][1] == [20480] * 40 and got["homopolymer-600"][2] == 1             # 2 x 32 x 320, the maximum
    assert got["swap"][2] == 1 and got["swap"][3] == 1
    tails = {k: got[k][2] for k in cases if k.startswith("tail-")}
    assert tails == {"tail-L200-n6": 0, "tail-L200-n7": 0, "tail-L201-n6": 1, "tail-L201-n7": 0,      # > 200 with a score < 200 | >= 200
                     "tail-L500-n6": 1, "tail-L500-n7": 0, "tail-L501-n6": 1, "tail-L501-n7": 1}, tails   # > 500 whatever the score
    assert got["tail-L201-n6"][1][0] == 2 * 192 and got["tail-L201-n7"][1][0] == 224
    assert any(c > 3 for s in cases["bytes-NM-lower"] for c in _CODE[np.frombuffer(s, dtype=np.uint8)])
    assert {len(s) for s in cases["short-among-long"]} >= {0, 7, 8, 9}
    assert all(k == 0 for k in got["all-short"][1])
    return cases


FUZZ_LENS = (0, 1, 7, 8, 9, 39, 40, 41, 47, 48, 200, 201, 500, 501, 600, 9999)


def fuzz_jobs(n, seed=4242):
    """Per job n in 1..40 sequences; lengths from FUZZ_LENS or random; near-copies of one base string, unrelated strings, or a
    two-letter alphabet; every eighth job around a tandem repeat; every 16th job with stray bytes."""
    rng = np.random.default_rng(seed)
    jobs = []
    for it in range(n):
        k = int(rng.integers(1, CAN_MAX + 1))
        kind = it % 4
        letters = b"AC" if kind == 2 else b"ACGT"
        L0 = int(FUZZ_LENS[int(rng.integers(0, len(FUZZ_LENS)))]) if it % 3 else int(rng.integers(0, 700))
        base = _rand(rng, L0, letters)
        if it % 8 == 7:                     # a tandem repeat: k-mers repeat inside a window, scores pass 32, find_ref_lqseq swaps
            unit = _rand(rng, int(rng.integers(1, 6)), letters)
            base = (unit * (L0 // len(unit) + 1))[:L0]
        seqs = []
        for j in range(k):
            r = rng.random()
            if kind == 1 or r < 0.1:           # unrelated
                L = int(FUZZ_LENS[int(rng.integers(0, len(FUZZ_LENS) - (1 if rng.random() < 0.97 else 0)))]) if rng.random() < 0.5 else int(rng.integers(0, 700))
                s = _rand(rng, L, letters)
            elif r < 0.3:
                s = base                        # an exact copy: ties
            elif r < 0.4 and L0 > 60:           # the same ends, another middle
                s = base[:45] + _rand(rng, int(rng.integers(0, 300)), letters) + base[-45:]
            else:
                s = _noisy(rng, base, 0.01 if L0 > 1000 else 0.1)
            if it % 16 == 5 and len(s) and rng.random() < 0.5:
                b = bytearray(s)
                for p in rng.integers(0, len(b), 3):
                    b[int(p)] = int(rng.integers(0, 256))
                s = bytes(b)
            seqs.append(s[:9999])
        jobs.append(seqs)
    return jobs


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
_PILES = []


def load_rank_piles():
    """tests/golden/rank_piles.npz in the layout of edge_piles.npz (util.load_edge_piles); read once."""
    if not _PILES:
        d = np.load(os.path.join(util.GOLD, "rank_piles.npz"))
        cache = {}

        def read(r):
            if r not in cache:
                packed = d["codes"][d["codes_off"][r]:d["codes_off"][r + 1]]
                cache[r] = util.ASC[util.unpack2(packed, int(d["lens"][r]))].tobytes()
            return cache[r]

        off = d["pile_off"]
        for p in range(off.size - 1):
            a, b = int(off[p]), int(off[p + 1])
            _PILES.append(dict(tag=str(d["tag"][p]), seqs=[read(int(r)) for r in d["rec_read"][a:b]],
                               aln_start=[int(x) for x in d["aln_start"][a:b]], aln_end=[int(x) for x in d["aln_end"][a:b]],
                               max_aln=int(d["max_aln"][p]), max_lq=int(d["max_lq"][p]), read_type=int(d["read_type"][p]),
                               fast=int(d["fast"][p]), split=int(d["split"][p]), min_len_aln=int(d["min_len_aln"][p]),
                               max_cov_aln=int(d["max_cov_aln"][p]), min_cov_base=int(d["min_cov_base"][p]), ratio=float(d["ratio"][p]),
                               exp_len=int(d["exp_len"][p]), exp_ide=float(d["exp_ide"][p]),
                               exp_seq=d["exp_seq"][d["exp_seq_off"][p]:d["exp_seq_off"][p + 1]].tobytes()))
    return _PILES


def pile_sets(names, max_reads=None):
    """The piles of the named fixtures ('golden', 'edge', 'rank') in one list, each with the batched entry's arguments."""
    out = []
    for name in names:
        if name == "golden":
            for i, p in enumerate(util.load_piles()):
                q = dict(p, tag="golden/%d" % i, min_len_aln=500, max_cov_aln=130, min_cov_base=4, ratio=0.8)
                out.append(q)
        elif name == "edge":
            out += util.load_edge_piles()
        elif name == "rank":
            out += [p for p in load_rank_piles() if max_reads is None or len(p["seqs"]) - 1 <= max_reads]
    return out


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run --------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, rank_util
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
if what == "batch":             # directed cases + fuzz jobs: device, host flag and the restatement
    n_fuzz, call = int(sys.argv[3]), int(sys.argv[4])
    jobs = [c[1] for c in rank_util.directed_cases()] + rank_util.fuzz_jobs(n_fuzz)
    exp = rank_util.want(jobs)
    dev, host = [], []
    for a in range(0, len(jobs), call):
        dev += api.lq_rank_batch(jobs[a:a + call])
        host += api.lq_rank_batch(jobs[a:a + call], host=True)
    as_l = lambda r: [[list(o), list(k), int(t)] for o, k, t in r]
    dev, host, exp = as_l(dev), as_l(host), as_l(exp)
    bad_dev = [i for i in range(len(jobs)) if dev[i] != exp[i]]
    bad_host = [i for i in range(len(jobs)) if host[i] != exp[i]]
    print(json.dumps(dict(n=len(jobs), bad_dev=bad_dev[:20], bad_host=bad_host[:20], tails=sum(e[2] for e in exp), stats=api.stats())))
elif what == "piles":           # fixtures through correct_batch, grouped by the arguments a call takes once
    piles = rank_util.pile_sets(sys.argv[3].split(","), int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[4] != "all" else None)
    rec, bad = {}, []
    for key, members in util.edge_groups(piles).items():
        for p, got in zip(members, util.edge_correct_group(api, key, members)):
            w = util.edge_wrong(p, got)
            if w:
                bad.append(w)
            rec[p["tag"]] = [int(got[0]), int(np.float32(got[1]).view(np.uint32)) if got[0] > 4 else 0, got[2].decode() if got[0] > 4 else ""]
    print(json.dumps(dict(rec=rec, bad=bad, n=len(piles), stats=api.stats())))
"""


def child(lib, what, *args, timeout=1500, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("NDGPU_RANK", "NDGPU_POA", "NDGPU_TRACE", "NDGPU_EXTRACT"))}   # no switch of the caller's reaches the child
    e.update(env)
    if lib == "simt":
        e.setdefault("NDGPU_CONTEXTS", "1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE, os.path.join(HERE, "simt")), lib, what, *[str(a) for a in args]],
                         env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    lines = [ln for ln in out.stderr.splitlines() if ln.startswith("[ndgpu] extract: ")]   # (NDGPU_TRACE)
    r["extract_launches"] = len(lines)
    r["pool_retaken"] = sum(int(ln.rsplit(", pool retaken ", 1)[1]) for ln in lines if ", pool retaken " in ln)   # K11 launches that came back short
    return r


def check_pool_retake(short, plain):
    """Two runs of the same piles with the ranking behind K11, `short` under NDGPU_EXTRACT_POOL=1 (the first guess of K11's string
    pool is one byte: K11 writes nothing beyond it, K14 leaves the regions it cannot read, and DeviceAligner::run_extract takes both
    again with the size K11 reported), `plain` without: the same records and the same regions ranked, and only `short` retook."""
    assert short["n"] == plain["n"] >= 12 and short["bad"] == [] and plain["bad"] == [], (short["bad"], plain["bad"])
    assert short["rec"] == plain["rec"]    # length, float32 identity bits, bases
    assert short["pool_retaken"] >= 1 and plain["pool_retaken"] == 0, (short["pool_retaken"], plain["pool_retaken"])
    assert short["extract_launches"] == plain["extract_launches"] > 0
    for k in ("rank_jobs", "rank_tail"):
        assert short["stats"][k] == plain["stats"][k] > 0, (k, short["stats"], plain["stats"])
    assert short["stats"]["rank_launches"] == plain["stats"]["rank_launches"] + short["pool_retaken"]    # K14 runs again with K11
