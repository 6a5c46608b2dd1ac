"""Shared by tests/test_simt_phase.py and tests/test_zz_gpu_phase.py: the phasing and ranking of a HiFi pile's low-quality-region
candidates restated in Python from the reference's lines (lib/nextcorrect.c:512-737 the helpers, :787-948 the program up to the sort by
score), not from the library, with a counter on every branch; directed piles, one shape per branch, and a seeded fuzz generator for the
batched entry (api.hifi_phase_batch); and the child processes that run the entry and the engine (api.correct_batch) under the switches
that are read once per process.

Two of the program's statements cannot be reached, whatever the pile, and carry no counter:
  * the second `k == lqseq->len` exit (:928): after reverse_lqseq the lengths descend, so the loop in front of it stops at the latest
    when lqseq->len - 1 == k (seqs[k].len < seqs[k].len / 2 is false), and lqseq->len stays above k;
  * trim_endssr_is_same reads in front of the shorter string when the longer one has more than twice its bytes (:716-737); the
    library's rule and K22 count such a byte as a mismatch, and so does this restatement."""
import collections
import json
import os
import subprocess
import sys

import numpy as np

import rank_util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CAN_MAX = 40
EMPTY, DROPPED, SEED, RANKED = 0, 1, 2, 3
CNT = collections.Counter()
BRANCHES = ("most2_tie_taken", "most2_tie_kept", "most2_m2_same", "most2_m2_greater",
            "p1_s0", "p1_k0", "p1_neither", "p1_homo", "heter_by_length",
            "p2_s0", "p2_k0", "p2_homo_end", "p2_trim_endssr", "p2_prefixhomo", "p2_continue", "p2_same_s", "p2_same_k", "p2_homo",
            "mark_kk_ge2", "mark_kk_lt2", "compact_to_0", "compact_none", "compact_some",
            "spkp_swapped", "spkp_kept", "difflen_s_le3", "difflen_s_gt3", "difflen_compacts", "difflen_keeps",
            "seed_lower", "seed_upper", "trim1", "drop1", "reversal", "trim2", "sort_skipped", "rank_tail", "rank_no_tail")


def _hit(name):
    CNT[name] += 1


# ---- the restatement: a candidate is [order (source read), kscore, len, bytes, input index] ----------------------------------------
def _same(a, b):
    return a[2] == b[2] and a[3] == b[3]


def _select_most2(q, ln, count=True):       # :632-653
    used = [0] * CAN_MAX
    m1 = m2 = 0
    for j in range(ln):
        q[j][1] = 1
        if used[j]:
            continue
        for k in range(j + 1, ln):
            if _same(q[j], q[k]):
                used[k] = 1
                q[j][1] += 1
        if q[j][1] > q[m1][1] or (q[j][1] == q[m1][1] and q[j][0] < q[m1][0]):
            if count and q[j][1] == q[m1][1]:
                _hit("most2_tie_taken")
            m2, m1 = m1, j
        elif m2 == m1 or q[j][1] > q[m2][1]:
            if count and j:
                _hit("most2_m2_same" if m2 == m1 else "most2_m2_greater")
                if q[j][1] == q[m1][1]:
                    _hit("most2_tie_kept")
            m2 = j
    return m1, m2


def _select_most2_with_kscore(q, ln):       # :656-668
    m1 = m2 = 0
    for j in range(ln):
        if q[j][1] > q[m1][1] or (q[j][1] == q[m1][1] and q[j][0] < q[m1][0]):
            m2, m1 = m1, j
        elif m2 == m1 or q[j][1] > q[m2][1]:
            m2 = j
    return m1, m2


def _run_ends(s):                           # :678-683
    n = len(s)
    a = 0
    while a + 1 < n and s[a] == s[a + 1]:
        a += 1
    e = n - 1
    while e > 0 and s[e - 1] == s[e]:
        e -= 1
    return a, e


def _homo_end_same(a, b):                   # :684-697
    as_, ae = _run_ends(a)
    bs, be = _run_ends(b)
    if ae <= as_ and be <= bs:
        return 1
    if ae - as_ != be - bs:
        return 0
    return 1 if a[as_:ae + 1] == b[bs:be + 1] else 0


def _prefixhomo_same(a, b):                 # :699-714
    i = j = 0
    na, nb = len(a), len(b)
    while i < na and j < nb:
        if a[i] != b[j]:
            return 0
        while i + 1 < na and a[i] == a[i + 1]:
            i += 1
        while j + 1 < nb and b[j] == b[j + 1]:
            j += 1
        i += 1
        j += 1
    return 1


def _trim_endssr_same(a, b):                # :716-737
    if len(a) < len(b):
        a, b = b, a
    na, nb = len(a), len(b)
    if a[:nb] != b:
        return 0
    for j in range(na - 1, nb - 1, -1):
        at = nb - (na - j)
        if at < 0 or a[j] != b[at]:
            return 0
    return 1


def _like_first(x, first):
    if _homo_end_same(x, first):
        _hit("p2_homo_end")
        return 1
    if _trim_endssr_same(x, first):
        _hit("p2_trim_endssr")
        return 1
    if _prefixhomo_same(x, first):
        _hit("p2_prefixhomo")
        return 1
    return 0


def _compact(lq, dif):                      # :524-537, :599-609
    q = lq["q"]
    k = lq["len"]
    j = 0
    while j < lq["len"] and j < k:
        if dif[j]:
            k -= 1
            while k > j:
                if not dif[k]:
                    q[j], q[k] = q[k], q[j]
                    break
                k -= 1
        j += 1
    lq["len"] = k


def _remove_differ_len(lq):                 # :512-539
    q = lq["q"]
    k = lq["end"] - lq["start"] + 1
    offset = min(max(30, k // 10), k // 3)
    dif = [0] * CAN_MAX
    s = 0
    for j in range(lq["len"]):
        if q[j][2] + offset >= k and q[j][2] <= k + offset:
            s += 1
        else:
            dif[j] = 1
    n = lq["len"]
    if s != n and (s >= n // 2 or (s >= n // 3 and s >= 3)):
        _hit("difflen_compacts")
        _compact(lq, dif)
    else:
        _hit("difflen_keeps")
    return s


def _scores(q, ln, from_tail):              # count_kmers with c = LQ_CAN_MAX, count_kscore (:281-337)
    K, valid = rank_util._kmers([x[3] for x in q[:ln]], from_tail)
    return [int(v) for v in rank_util._pass(np.arange(ln), K, valid, CAN_MAX)]


def _record(lq, kind, n, **kw):
    q = lq["q"]
    r = dict(kind=kind, lower=0, indexs=lq["indexs"], tail=0, n=n, seed=0, seed_pos=0, perm=[x[4] for x in q], kscore=[x[1] for x in q])
    r.update(kw)
    return r


def restate(n_aligned, regions):
    """(n_aligned, [(start, end, [bytes], [source read])]) -> dict(has_heter, pass2, regions=[record]) in api.hifi_phase_batch's form."""
    R = [dict(start=st, end=en, len=len(seqs), indexs=0, q=[[src[i], 0, len(seqs[i]), seqs[i], i] for i in range(len(seqs))])
         for st, en, seqs, src in regions]
    ps, pd, pdel = ([0] * max(1, n_aligned) for _ in range(3))
    has_heter = 0
    for lq in R:                            # :789-810
        if not lq["len"]:
            continue
        q = lq["q"]
        s, k = _select_most2(q, lq["len"])
        if s != k and q[k][1] >= 3 and q[s][2] == q[k][2]:
            if s == 0 or k == 0:
                _hit("p1_s0" if s == 0 else "p1_k0")
                heter = k if s == 0 else s
                for j in range(lq["len"]):
                    i = q[j][0]
                    if _same(q[0], q[j]):
                        ps[i] = (ps[i] + 1) & 0xffff
                    elif _same(q[heter], q[j]):
                        pd[i] = (pd[i] + 1) & 0xffff
            else:
                _hit("p1_neither")
            lq["indexs"] = 1
        else:
            _hit("p1_homo")
            lq["indexs"] = 0
        if not has_heter:
            if lq["indexs"] == 1:
                has_heter = 1
            elif s != k and q[k][1] >= 5 and q[s][1] + q[k][1] >= lq["len"] * 0.8 and not _prefixhomo_same(q[s][3], q[k][3]):
                _hit("heter_by_length")
                has_heter = 1
    pass2 = 1 if has_heter and not ps[0] else 0
    if pass2:                               # :812-854
        for lq in R:
            if not lq["len"]:
                continue
            q = lq["q"]
            s, k = _select_most2_with_kscore(q, lq["len"])
            if s != k and q[k][1] >= 5 and q[s][1] + q[k][1] >= lq["len"] * 0.8 and \
                    (q[s][2] >= q[k][2] + 5 or q[k][2] >= q[s][2] + 5 or not _prefixhomo_same(q[s][3], q[k][3])):
                if s == 0:
                    _hit("p2_s0")
                    s_, k_ = 1, 0
                elif k == 0:
                    _hit("p2_k0")
                    s_, k_ = 0, 1
                else:
                    s_ = _like_first(q[s][3], q[0][3])
                    k_ = _like_first(q[k][3], q[0][3])
                if s_ and not k_:
                    _hit("p2_same_s")
                    same, heter = s, k
                elif k_ and not s_:
                    _hit("p2_same_k")
                    same, heter = k, s
                else:
                    _hit("p2_continue")
                    continue
                for j in range(lq["len"]):
                    i = q[j][0]
                    if _same(q[same], q[j]):
                        ps[i] = (ps[i] + 1) & 0xffff
                    elif _same(q[heter], q[j]):
                        pd[i] = (pd[i] + 1) & 0xffff
                lq["indexs"] = 2
            else:
                _hit("p2_homo")
                lq["indexs"] = 0
    for lq in R:                            # mark_del_lqseq, :570-588
        if not lq["len"]:
            continue
        q = lq["q"]
        kk = sum(1 for j in range(1, lq["len"]) if ps[q[j][0]] >= 3 and not pd[q[j][0]])
        _hit("mark_kk_ge2" if kk >= 2 else "mark_kk_lt2")
        for j in range(lq["len"]):
            i = q[j][0]
            if kk >= 2:
                if pd[i]:
                    pdel[i] = 1
            elif ps[i] < pd[i] or pd[i] >= 3:
                pdel[i] = 1
    for lq in R:                            # remove_differ_phase_lqseq, :590-610
        if not lq["len"]:
            continue
        dif = [1 if pdel[x[0]] else 0 for x in lq["q"][:lq["len"]]] + [0] * CAN_MAX
        _compact(lq, dif)
        _hit("compact_none" if not any(dif) else "compact_to_0" if not lq["len"] else "compact_some")
    out = []
    for lq in R:                            # :874-948
        q = lq["q"]
        if not q:
            out.append(dict(kind=EMPTY, lower=0, indexs=0, tail=0, n=0, seed=0, seed_pos=0, perm=[], kscore=[]))
            continue
        if not lq["len"]:
            out.append(_record(lq, DROPPED, 0))
            continue
        s, k = _select_most2(q, lq["len"], count=False)
        i = q[s][0]
        if lq["indexs"] and s != k and s != 0 and q[k][1] >= 3 and ps[i] >= pd[i] + 3:
            sp = kp = 0
            for j in range(1, lq["len"]):
                i = q[j][0]
                if pd[i] >= 3:
                    continue
                if _same(q[s], q[j]):
                    sp += ps[i] - pd[i]
                elif _same(q[k], q[j]):
                    kp += ps[i] - pd[i]
            _hit("spkp_swapped" if sp < kp else "spkp_kept")
            if sp < kp:
                s = k
        elif q[0][2] > 50 and q[s][1] < lq["len"] // 3 and q[s][1] < 3:
            sl = _remove_differ_len(lq)
            _hit("difflen_s_le3" if sl <= 3 else "difflen_s_gt3")
            if sl <= 3:
                s = 0
                q[s][1] = 65534
        if q[s][1] > 2 or q[s][1] >= lq["len"] // 2:
            lower = 1 if q[s][1] < lq["len"] // 2 else 0
            _hit("seed_lower" if lower else "seed_upper")
            out.append(_record(lq, SEED, -2, lower=lower, seed=q[s][4], seed_pos=s))
            continue
        _remove_differ_len(lq)
        if lq["len"] > 4:
            n = lq["len"]
            q[:n] = sorted(q[:n], key=lambda x: x[2])          # qsort(compare_seq_by_len): glibc's is a stable merge sort
            k = n // 2
            trimmed = 0
            while n > k and (q[n - 1][2] > 2 * q[k][2] or q[n - 1][2] >= 1.4 * q[n - 2][2]):
                n -= 1
                trimmed = 1
            if trimmed:
                _hit("trim1")
            lq["len"] = n
            if k == n:
                _hit("drop1")
                out.append(_record(lq, DROPPED, 0))
                continue
            k = n // 2
            if q[0][2] < q[k][2] // 2:
                _hit("reversal")
                q[:n] = q[:n][::-1]
                trimmed = 0
                while q[n - 1][2] < q[k][2] // 2:
                    n -= 1
                    trimmed = 1
                if trimmed:
                    _hit("trim2")
                lq["len"] = n
                assert k != n                                  # (:928, see the module's text)
        else:
            _hit("sort_skipped")
        n = lq["len"]
        for j, v in enumerate(_scores(q, n, 0)):
            q[j][1] = v
        tail = 1 if q[0][2] > 100 else 0
        _hit("rank_tail" if tail else "rank_no_tail")
        if tail:
            saved = {}
            for j in range(n):
                saved[q[j][0]] = q[j][1]                       # save_kscore: by source read
            for j, v in enumerate(_scores(q, n, 1)):
                q[j][1] = (v + saved[q[j][0]]) & 0xffff
        q[:n] = sorted(q[:n], key=lambda x: -x[1])             # qsort(compare_seq_by_kscore)
        out.append(_record(lq, RANKED, n, tail=tail))
    return dict(has_heter=has_heter, pass2=pass2, regions=out)


def strip(res):
    """What the entry returns without `declined`, to compare with restate()."""
    return [dict(has_heter=r["has_heter"], pass2=r["pass2"], regions=r["regions"]) for r in res]


# ---- directed piles: name -> (n_aligned, regions, the counters the pile must reach) -----------------------------------------------
def _reg(cands, span=None, start=100):
    seqs = [c[0] for c in cands]
    span = span if span is not None else max(1, len(seqs[0]) if seqs else 1)
    return (start, start + span - 1, seqs, [c[1] for c in cands])


def _rand(rng, n, letters=b"ACGT"):
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes()


def directed_piles():
    rng = np.random.default_rng(77)
    X, Y, Z = b"ACGTTGCAAC", b"ACGTAGCAAC", b"ACGTCGCAAC"            # SNP alleles, equal lengths
    XL = b"ACGTTCATCAGCAAC"                                          # five bases longer than X, another run-compressed string
    out = {}
    two_hap = lambda n_a, n_b, first_b=False: ([(Y if first_b else X, 0)] + [(X, i) for i in range(1, n_a)] +
                                                 [(Y, n_a + i) for i in range(n_b)])
    out["tie-lower-order-wins"] = (8, [_reg([(X, 5), (X, 6), (Y, 1), (Y, 2), (Z, 7)])], ["most2_tie_taken"])
    out["tie-higher-order-loses"] = (8, [_reg([(X, 1), (X, 2), (Y, 5), (Y, 6), (Z, 7), (Z, 3), (Z, 4)])], ["most2_tie_kept", "most2_m2_same"])
    out["m2-greater"] = (9, [_reg([(X, 0), (X, 1), (X, 2), (Z, 3), (Y, 4), (Y, 5)])], ["most2_m2_greater"])
    out["pass1-s0"] = (9, [_reg(two_hap(6, 3))], ["p1_s0", "mark_kk_lt2"])
    out["pass1-k0"] = (9, [_reg([(Y, 0)] + [(X, i) for i in range(1, 7)] + [(Y, 7), (Y, 8)])], ["p1_k0"])
    out["pass1-neither"] = (10, [_reg([(Z, 0)] + [(X, i) for i in range(1, 6)] + [(Y, i) for i in range(6, 9)])], ["p1_neither"])
    out["heter-by-length"] = (12, [_reg([(X, i) for i in range(6)] + [(XL, i) for i in range(6, 11)])], ["heter_by_length", "p2_s0", "p2_same_s"])
    out["pass2-k0"] = (12, [_reg([(XL, 0)] + [(X, i) for i in range(1, 7)] + [(XL, i) for i in range(7, 11)])], ["p2_k0", "p2_same_k"])
    mid = b"CGTTGCA"
    U = b"GGATTACAGGATTACA"                                          # unrelated to the first candidate by every predicate
    first = b"A" + mid + b"T"
    out["pass2-homo-end"] = (13, [_reg([(first, 0)] + [(b"AAA" + mid + b"TTTTTT", i) for i in range(1, 7)] + [(U, i) for i in range(7, 12)])],
                             ["p2_homo_end", "p2_same_s"])
    ssr = b"ACTGAGAGA"
    out["pass2-trim-endssr"] = (13, [_reg([(ssr, 0)] + [(U, i) for i in range(1, 7)] + [(ssr + b"GAGAGA", i) for i in range(7, 12)])],
                                ["p2_trim_endssr", "p2_same_k"])
    out["pass2-prefixhomo"] = (13, [_reg([(b"ACGTGCA", 0)] + [(b"AACCGGTTGGCCAA", i) for i in range(1, 7)] + [(U, i) for i in range(7, 12)])],
                               ["p2_prefixhomo", "p2_same_s"])
    out["pass2-continue"] = (13, [_reg([(b"TTTTGGGG", 0)] + [(U, i) for i in range(1, 7)] + [(U[::-1] + b"ACACA", i) for i in range(7, 12)])],
                             ["p2_continue"])
    # four SNP sites phase the reads: 0..5 with the seed, 6..8 against it; then regions of one haplotype each
    sites = [_reg(two_hap(6, 3), start=100 + 50 * i) for i in range(4)]
    out["mark-kk-ge2-compaction"] = (9, sites + [_reg([(X, i) for i in range(6)], start=400),          # nothing flagged
                                                 _reg([(Y, 6), (Y, 7), (Y, 8)], start=450)],           # every candidate flagged
                                     ["mark_kk_ge2", "compact_some", "compact_none", "compact_to_0", "seed_upper"])
    # reads 5..7 agree with the seed at ten sites, reads 1..4 at three: the region's larger class loses to the better phased one
    many = [_reg([(X, 0), (X, 5), (X, 6), (X, 7), (Y, 8), (Y, 9), (Y, 10)], start=100 + 20 * i) for i in range(7)]
    three = [_reg([(X, i) for i in range(8)] + [(Y, 8), (Y, 9), (Y, 10)], start=300 + 20 * i) for i in range(3)]
    out["sp-less-than-kp"] = (11, many + three + [_reg([(Z, 0)] + [(X, i) for i in range(1, 5)] + [(Y, i) for i in range(5, 8)], start=500)],
                              ["spkp_swapped"])
    out["sp-not-less"] = (11, three + [_reg([(Z, 0)] + [(X, i) for i in range(1, 5)] + [(Y, i) for i in range(5, 8)], start=500)], ["spkp_kept"])
    # no string three times, a first candidate beyond 50 bases
    base = _rand(rng, 60)
    own = lambda L, i: (_rand(np.random.default_rng(1000 + i), L), i)
    out["difflen-s-le3"] = (12, [_reg([(base, 0)] + [own(60, 1), own(61, 2)] + [own(200, i) for i in range(3, 10)], span=60)],
                            ["difflen_s_le3", "seed_upper"])
    out["difflen-s-gt3"] = (12, [_reg([(base, 0)] + [own(58 + i, i) for i in range(1, 8)] + [own(400, 8), own(410, 9)], span=60)],
                            ["difflen_s_gt3", "difflen_compacts", "rank_no_tail"])
    out["seed-lower"] = (12, [_reg([(X, 0), (X, 1), (X, 2)] + [own(10, i) for i in range(3, 11)])], ["seed_lower"])
    own_l = lambda L, i: (_rand(np.random.default_rng(2000 + i + L), L), i)
    out["trim1"] = (12, [_reg([own_l(20 + i, i) for i in range(8)] + [own_l(31, 8), own_l(46, 9)], span=3000)], ["trim1", "rank_no_tail"])
    out["drop1"] = (12, [_reg([own_l(L, i) for i, L in enumerate((10, 11, 12, 13, 20, 30, 45, 70, 100, 150))], span=3000)], ["trim1", "drop1"])
    out["reversal-trim2"] = (12, [_reg([own_l(L, i) for i, L in enumerate((4, 5, 30, 31, 32, 33, 34, 35, 36, 37))], span=3000)],
                             ["reversal", "trim2"])
    out["sort-skipped"] = (12, [_reg([own_l(20 + i, i) for i in range(4)], span=3000)], ["sort_skipped"])
    long_ = _rand(rng, 140)
    noisy = lambda i: (rank_util._noisy(np.random.default_rng(3000 + i), long_, 0.1), i)
    out["rank-tail"] = (12, [_reg([noisy(i) for i in range(9)], span=140)], ["rank_tail"])
    seed10k = _rand(rng, 10000)
    out["seed-of-10000"] = (12, [_reg([(seed10k, 0)] + [(rank_util._noisy(np.random.default_rng(4000 + i), seed10k[:900], 0.02), i) for i in range(1, 9)],
                                      span=9000),
                                 _reg([(seed10k, 0), (seed10k, 1), (seed10k[:-1] + b"A", 2), (seed10k, 3)], span=10000, start=20000)], [])
    out["zero-length"] = (12, [_reg([(b"", 0), (b"", 1), (b"", 2), (X, 3), (b"", 4)], span=3),
                               _reg([(b"", 0)] + [own_l(L, i + 1) for i, L in enumerate((0, 9, 10, 11, 12, 13))], span=10, start=300)], [])
    out["no-candidates"] = (5, [_reg([], span=10), _reg([(X, 0), (X, 1)]), _reg([], span=5, start=300)], [])
    out["one-source-read-twice"] = (6, [_reg([(rank_util._noisy(np.random.default_rng(5000 + i), long_, 0.1), i % 3) for i in range(9)], span=140)],
                                    ["rank_tail"])
    return out


def check_directed():
    """Every directed pile reaches the branches it is there for (the restatement's own counters)."""
    piles = directed_piles()
    for name, (n_aligned, regions, want) in piles.items():
        CNT.clear()
        restate(n_aligned, regions)
        missing = [w for w in want if not CNT[w]]
        assert not missing, (name, missing, dict(CNT))
    assert len(piles["seed-of-10000"][1][0][2][0]) == 10000
    return piles


# ---- the fuzz generator -----------------------------------------------------------------------------------------------------------
def _mutate(rng, s, letters):
    """One edit of s: a substitution, a deletion, an insertion or a longer homopolymer run."""
    if not s:
        return _rand(rng, 1, letters)
    p = int(rng.integers(0, len(s)))
    what = int(rng.integers(0, 4))
    if what == 0:
        return s[:p] + _rand(rng, 1, letters) + s[p + 1:]
    if what == 1:
        return s[:p] + s[p + 1:]
    if what == 2:
        return s[:p] + _rand(rng, int(rng.integers(1, 8)), letters) + s[p:]
    return s[:p] + s[p:p + 1] * int(rng.integers(1, 7)) + s[p:]


def _snp(a, letters, at):
    return a[:at] + bytes([letters[(letters.index(a[at]) + 1) % len(letters)]]) + a[at + 1:]


def fuzz_piles(n, seed=2222):
    """Piles of 1..12 regions, 1..40 candidates of 0..160 bases over an alphabet of 2..4 letters, up to 64 reads.  The reads carry one
    of up to three haplotypes; a region gives every haplotype an allele (the same, a substitution apart, an insertion or a repeat
    expansion apart, or unrelated) and every read its haplotype's allele, its own edit of it, or a string of its own -- so that
    strings repeat, phase, and fail to.  Piles by style (pile number mod 6): 0..2 mostly SNP sites, among them sites split by another
    rule than the haplotypes and sites that only one haplotype's reads cover; 3: alleles of different lengths and no SNP, the first
    candidate a relative of one allele (the second pass and its predicates); 4: every read its own string, some regions with lengths in
    a geometric row; 5: a mix."""
    rng = np.random.default_rng(seed)
    piles = []
    for it in range(n):
        style = it % 6
        n_reads = int(rng.integers(1, 65))
        if style == 3:
            n_reads = max(n_reads, 14)
        if style <= 2 and it % 2 == 0:
            n_reads = max(n_reads, 24)
        letters = (b"AC", b"ACG", b"ACGT")[int(rng.integers(0, 3))]
        frac = 0.42 if style == 3 else 0.3 if style <= 2 and it % 2 == 0 else (0.0, 0.25, 0.4, 0.5, 0.7)[it % 5]
        hap = (rng.random(n_reads) < frac).astype(np.int64)
        if it % 7 == 3 and style != 3:
            hap[rng.random(n_reads) < 0.3] = 2
        if style == 3:
            hap[0] = int(rng.random() < 0.5)
        elif it % 4:
            hap[0] = 0
        n_reg = int(rng.integers(9, 13)) if style <= 2 and it % 2 == 0 else int(rng.integers(1, 13))
        regions = []
        for r in range(n_reg):
            kind = int(rng.integers(0, 6)) if style == 5 else (style if style >= 3 else (0 if rng.random() < 0.8 else int(rng.integers(0, 6))))
            L = int(rng.integers(0, 161)) if rng.random() < 0.5 else int(rng.integers(4, 30))
            u = rng.random()
            special = None
            phased = style <= 2 and it % 2 == 0        # six SNP sites, then sites of other kinds
            if phased and r < 6:
                pass
            elif phased and u < 0.6:
                special = "local"
            elif style <= 2 and u < (0.8 if phased else 0.15) and (hap == 1).sum() >= 1:
                special = "minority"
            elif style == 4 and u < 0.35:
                special = "geometric"
            if style == 3 or special == "local":
                L = max(L, 12)
            clean = style <= 2 and it % 2 == 0 and special is None and rng.random() < 0.9     # a plain SNP site
            if clean:
                kind, L = 0, max(L, 4)
            a0 = _rand(rng, L, letters)
            first = _mutate(rng, a0, letters) if rng.random() < 0.2 and not clean else None      # the first candidate as a third string
            if style == 3:
                w = int(rng.integers(0, 5))
                tails = [_rand(rng, int(rng.integers(2, 4)), letters) * 2 for _ in range(2)]     # each allele ends in a unit twice
                a0 = a0[:150] + tails[0]
                a1 = (_rand(rng, min(150, L + int(rng.integers(5, 11))), letters) + tails[1]) if w >= 2 else \
                    (a0 + _rand(rng, int(rng.integers(5, 9)), letters)) if w == 0 else a0 + a0[-1:] * int(rng.integers(1, 9))
                first = None
                if rng.random() < 0.6:
                    x = (a0, a1)[int(rng.integers(0, 2))]
                    v = (0, 1, 1, 2, 3)[int(rng.integers(0, 5))]
                    if v == 0:
                        first = x[:1] * 2 + x + x[-1:] * 3
                    elif v == 1:
                        first = x[:-(len(tails[0]) // 2)] if x is a0 else x[:-(len(tails[1]) // 2)] if w >= 2 else x[:-1]
                    elif v == 2:
                        p = len(x) // 2
                        first = x[:p] + x[p:p + 1] * 2 + x[p:]
                    else:
                        first = _rand(rng, len(x), letters)
            elif kind == 3:        # an insertion, a run or a repeat at the end
                w = int(rng.integers(0, 3))
                a1 = a0 + (_rand(rng, int(rng.integers(5, 12)), letters) if w == 0 else a0[-1:] * int(rng.integers(1, 9)) if w == 1 else a0[-2:] * int(rng.integers(1, 5)))
                if rng.random() < 0.5:
                    a0, a1 = a1, a0
            else:                # a substitution (kinds 0..2), or another string altogether
                a1 = _rand(rng, L, letters) if kind == 5 or not L else _snp(a0, letters, L // 2)
            a2 = _mutate(rng, a1, letters)
            alleles = (a0, a1, a2)
            k = int(rng.integers(1, min(CAN_MAX, n_reads) + 1)) if rng.random() < 0.7 and style != 3 else min(CAN_MAX, n_reads)
            reads = np.sort(rng.choice(n_reads, k, replace=False))
            if style <= 2 and it % 2 == 0 and special is None:      # every third read covers every site, the others a third of them
                reads = np.nonzero((np.arange(n_reads) % 3 == 0) | (rng.random(n_reads) < 0.5))[0][:CAN_MAX]
            if special == "minority":
                reads = np.nonzero(hap == 1)[0][:CAN_MAX]
            elif special == "local":
                reads = np.arange(min(CAN_MAX, n_reads))
            elif rng.random() < 0.15 and k > 1:
                reads = rng.permutation(reads)
            p_own = (0.0, 0.05)[int(rng.integers(0, 2))] if clean else 1.0 if kind == 4 else (0.0, 0.05)[int(rng.integers(0, 2))] if style == 3 else (0.0, 0.05, 0.3, 1.0)[int(rng.integers(0, 4))]
            span = max(1, len(a0) + int(rng.integers(-3, 4)))
            seqs = []
            if special == "geometric":
                lens = [min(160, int(3 * 1.5 ** i)) for i in range(min(len(reads), 11))]
                reads = reads[:len(lens)]
                seqs = [_rand(rng, int(x), letters) for x in rng.permutation(lens)]
                span = 3000
            elif special == "local":        # the split follows the reads' numbers, the first candidate is a third string
                a1 = _snp(a0, letters, L // 2)
                by_two = rng.random() < 0.3
                seqs = [_snp(a0, letters, 1) if x == 0 else (a0, a1)[int(rd) % 2 if by_two else int(rd) % 3 == 0] for x, rd in enumerate(reads)]
            else:
                for x, rd in enumerate(reads):
                    s = alleles[int(hap[rd])]
                    if x == 0 and first is not None:
                        s = first
                    elif rng.random() < p_own:
                        s = _rand(rng, int(rng.integers(0, 161)), letters) if (kind == 4 and rng.random() < 0.7) else _mutate(rng, s, letters)
                    seqs.append(s[:160])
            start = 100 + 4000 * r
            regions.append((start, start + span - 1, seqs, [int(x) for x in reads]))
        piles.append((n_reads, regions))
    return piles


def fuzz_counters(piles):
    CNT.clear()
    want = [restate(*p) for p in piles]
    return want, dict(CNT)


def case_piles():
    return [(v[0], v[1]) for v in directed_piles().values()]


def capacity_piles():
    """Three piles, the second with 2,049 aligned reads (one over K22's table, kPhaseReads of nd_device.h) and its candidates from
    the last of them."""
    a, b, c = fuzz_piles(3, seed=9)
    return [a, (2049, [(s, e, seqs, [2048 - x for x in src]) for s, e, seqs, src in b[1]]), c]


def big_pile(n_regions=3000, seed=31):
    """One pile of n_regions regions and 2,000 reads: the regions of fuzz piles with 40 reads or fewer, one behind the other, the
    reads of the k-th of them numbered from 40 * (k mod 50) on."""
    regions = []
    for k, (n_reads, regs) in enumerate(p for p in fuzz_piles(1500, seed=seed) if p[0] <= 40):
        at = len(regions)
        regions += [(100 + 4000 * (at + i), 100 + 4000 * (at + i) + e - s, seqs, [40 * (k % 50) + x for x in src])
                    for i, (s, e, seqs, src) in enumerate(regs)]
        if len(regions) >= n_regions:
            break
    assert len(regions) >= n_regions
    return (2000, regions[:n_regions])


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
_PILES = []


def load_phase_piles():
    """tests/golden/hifi_phase_piles.npz (make_hifi_phase_golden.py: HiFi piles of two haplotypes and piles where every read carries
    its own repeat length, with the compiled reference's answers) in the layout of rank_piles.npz; read once."""
    import util
    if not _PILES:
        d = np.load(os.path.join(util.GOLD, "hifi_phase_piles.npz"))
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
    """The HiFi piles of the named fixtures ('golden', 'edge': rank_util.pile_sets; 'phase': the fixture above, its piles of at most
    max_reads reads)."""
    out = [p for p in rank_util.pile_sets([n for n in names if n != "phase"]) if p["read_type"] == 3]
    if "phase" in names:
        out += [p for p in load_phase_piles() if max_reads is None or len(p["seqs"]) - 1 <= max_reads]
    return out


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run --------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, rank_util, phase_util
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
if what == "batch":             # directed piles + fuzz piles: device, host flag and the restatement, in calls of `call`
    n_fuzz, call = int(sys.argv[3]), int(sys.argv[4])
    piles = phase_util.case_piles() + phase_util.fuzz_piles(n_fuzz)
    exp = [phase_util.restate(*p) for p in piles]
    dev, host = [], []
    for a in range(0, len(piles), call):
        dev += api.hifi_phase_batch(piles[a:a + call])
        host += api.hifi_phase_batch(piles[a:a + call], host=True)
    declined = sum(r["declined"] for r in dev)
    dev, host = phase_util.strip(dev), phase_util.strip(host)
    bad_dev = [i for i in range(len(piles)) if dev[i] != exp[i]]
    bad_host = [i for i in range(len(piles)) if host[i] != exp[i]]
    first = [dev[bad_dev[0]], exp[bad_dev[0]]] if bad_dev else []
    print(json.dumps(dict(n=len(piles), bad_dev=bad_dev[:20], bad_host=bad_host[:20], first=first, declined=declined,
                          regions=sum(len(p[1]) for p in piles), kinds=[sum(1 for e in exp for g in e["regions"] if g["kind"] == k) for k in range(4)],
                          pass2=sum(e["pass2"] for e in exp), tails=sum(g["tail"] for e in exp for g in e["regions"]),
                          stats=api.phase_stats())))
elif what == "capacity":        # a pile of 2,049 aligned reads between two small ones
    piles = phase_util.capacity_piles()
    dev, host = api.hifi_phase_batch(piles), api.hifi_phase_batch(piles, host=True)
    exp = [phase_util.restate(*p) for p in piles]
    print(json.dumps(dict(declined=[r["declined"] for r in dev], same=phase_util.strip(dev) == phase_util.strip(host) == exp,
                          stats=api.phase_stats())))
elif what == "piles":           # fixtures through correct_batch, grouped by the arguments a call takes once
    piles = phase_util.pile_sets(sys.argv[3].split(","), int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[4] != "all" else None)
    rec, bad = {}, []
    for key, members in util.edge_groups(piles).items():
        for p, got in zip(members, util.edge_correct_group(api, key, members)):
            w = util.edge_wrong(p, got)
            if w:
                bad.append(w)
            rec[p["tag"]] = [int(got[0]), int(np.float32(got[1]).view(np.uint32)) if got[0] > 4 else 0, got[2].decode() if got[0] > 4 else ""]
    print(json.dumps(dict(rec=rec, bad=bad, n=len(piles), stats=api.stats(), phase=api.phase_stats())))
elif what == "piles_each":      # the same pile by pile, with each pile's own counters
    piles = phase_util.pile_sets(sys.argv[3].split(","), int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[4] != "all" else None)
    each, bad = [], []
    for p in piles:
        api.reset_stats()
        key = next(iter(util.edge_groups([p])))
        w = util.edge_wrong(p, util.edge_correct_group(api, key, [p])[0])
        if w:
            bad.append(w)
        each.append([p["tag"], api.phase_stats()])
    print(json.dumps(dict(each=each, bad=bad, n=len(piles))))
"""


def child(lib, what, *args, timeout=1500, **env):
    e = {k: v for k, v in os.environ.items()
         if not k.startswith(("NDGPU_RANK", "NDGPU_POA", "NDGPU_TRACE", "NDGPU_EXTRACT", "NDGPU_PHASE"))}   # no switch of the caller's reaches the child
    e.update(env)
    if lib == "simt":
        e.setdefault("NDGPU_CONTEXTS", "1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE, os.path.join(HERE, "simt")), lib, what, *[str(a) for a in args]],
                         env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    r["trace_lines"] = sum(1 for ln in out.stderr.splitlines() if ln.startswith("[ndgpu trace] hifi_phase "))
    return r
