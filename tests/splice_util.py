"""Shared by tests/test_simt_splice.py and tests/test_zz_gpu_splice.py: the end of a pile -- update_lqreg, update_consensus_trimed and
trim_terminal_ssr with its two helpers -- restated in Python from the reference's lines (lib/nextcorrect.c:1340-1482 and :2008-2128),
not from the library, with a count of how often each branch was taken; directed jobs, each the smallest shape at which K24
(splice_kernel, msa_kernels.hip: 64 items a chunk, a prefix maximum for the region index, an automaton that jumps along ballots) can
go wrong, and check_directed(), which asserts from the restatement that each reaches its shape; a seeded fuzz generator; and the child
processes that run the batched entry (api.splice_batch) under the switches that are read once per process.

A job here is (words, lstrip, rstrip, regions, read_type): words a uint32 array of pos << 8 | char in ascending positions, regions
[(start, end, len, sudoseed bytes)] in the engine's order (the index counts down while the positions go up), read_type 3 for HiFi.

One place where the restatement cannot follow the reference: at :1399 the `break` leaves the pseudo-seed's loop alone and the outer
loop goes on, writing lq[10] of a table of ten.  The engine ends the string there, as the base branch (:1408) does; so does this."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_CODE = [4] * 256                                   # base_to_int, lib/nextcorrect.c:42-50
for _ch, _v in ((b"Aa", 0), (b"Tt", 1), (b"Gg", 2), (b"Cc", 3), (b"N", 5), (b"M", 6)):
    for _c in _ch:
        _CODE[_c] = _v

BRANCHES = ("lower_open", "lower_extend", "lq_m_resets_hq", "close_start0", "gap_close", "gap_reset", "short_reset", "hold",
            "seed_emitted", "seed_empty", "region_skipped", "inside_silent", "base", "lagging_base", "bump",
            "raw_first", "raw_middle", "raw_tail", "raw_none", "raw_none_lead", "hifi_plain", "hifi_ends", "hifi_empty",
            "gate_len", "gate_identity", "trim_ran", "head_count_low", "tail_count_low", "clip_head", "clip_tail", "ssr_break", "ssr_reset",
            "ssr_p_short", "skip_lower", "len4")
U32 = 0xffffffff


def _update_lqreg(lq, seq, p, i, st, br):
    """:1340-1363; st = [hq_m, lq_m]"""
    s = lq[i]
    if seq[p] >= 97:
        if not s[2]:
            s[0] = p
            br["lower_open"] += 1
        else:
            br["lower_extend"] += 1
        if st[1] > 2:
            if st[0]:
                br["lq_m_resets_hq"] += 1
            st[0] = 0
        st[1] += 1
        s[1] = p
        s[2] += 1
        s[3] += 1
    else:
        if s[2] and s[0] == 0:
            i += 1
            st[0] = 0
            br["close_start0"] += 1
        else:
            c = st[0] + s[0] > s[1]
            if not c:
                c = st[0] > 10
                st[0] += 1
            if c:
                if s[1] > s[0] + 100:
                    i += 1
                    br["gap_close"] += 1
                else:
                    if s[2]:
                        br["gap_reset"] += 1
                    s[2] = s[1] = 0
                st[0] = 0
            elif st[0] >= s[2]:
                if s[2]:
                    br["short_reset"] += 1
                s[2] = s[1] = 0
                st[0] = 0
            else:
                br["hold"] += 1
        st[1] = 0
    return i


def _terminal_ssr(seq, s):
    """:2008-2032 with ssr_range 24, ssr_len 4 -> (kmer, its count)"""
    bins = [0] * 256
    km = 0
    for i in range(24):
        if i:
            km = (km << 2 | _CODE[seq[s + i + 3]]) & 0xff
        else:
            for k in range(4):
                km = (km << 2 | _CODE[seq[s + k]]) & 0xff
        bins[km] += 1
    best = 0
    for i in range(256):
        if bins[i] > best:
            best = bins[i]
            km = i
    return km, bins[km]


def _clip_ssr(seq, seq_len, kmer, dire, br):
    """:2034-2098"""
    gap = 20
    p = p1 = p2 = kt = 0
    if dire:
        for i in range(0, 8, 2):
            kt = (kt << 2 | (kmer >> i & 3)) & 0xff
        seq_len -= 1
        kmer, kt = kt, 0
    for i in range(max(0, seq_len - 4)):
        if dire:
            if i:
                kt = (kt << 2 | _CODE[seq[seq_len - i - 4 + 1]]) & 0xff
            else:
                for k in range(4):
                    kt = (kt << 2 | _CODE[seq[seq_len - k]]) & 0xff
        else:
            if i:
                kt = (kt << 2 | _CODE[seq[i + 3]]) & 0xff
            else:
                for k in range(4):
                    kt = (kt << 2 | _CODE[seq[k]]) & 0xff
        if kt != kmer:
            if i - p > gap:
                if not p1:
                    p1 = p
                elif p2:
                    if i - p2 < 100:
                        p = p1
                        br["ssr_break"] += 1
                        break
                    p1 = p2 = 0
                    br["ssr_reset"] += 1
        else:
            p = i
            if p1 and p2 == 0:
                p2 = p
    if p <= 100:
        br["ssr_p_short"] += 1
    return p + 4 if p > 100 else 0


def restate(job):
    """-> dict: len, identity (numpy.float32), lq_total_len, out_len, lq_m, hq_m, lq_i, clip_s, clip_e, seq (bytes), br, truncated
    ('seed', 'base' or None), trimmed, table (the ten slots and the guard slot as the loop left them)"""
    words, lstrip, rstrip, regions, read_type = job
    w = [int(x) for x in words]
    n = len(w)
    br = dict.fromkeys(BRANCHES, 0)
    out = bytearray()
    lq = [[0, 0, 0, 0] for _ in range(11)]           # start, end, lqlen, lq_total_len; [10]: the engine's guard slot
    st = [0, 0]
    lq_i = 0
    update = 1
    idx = len(regions) - 1
    usable = lambda k: regions[k][2] > 0 or regions[k][2] == -2
    truncated = None
    i = lstrip
    while i < n - rstrip and truncated is None:
        p = w[i] >> 8
        if idx >= 0 and (not usable(idx) or p > regions[idx][1]):          # :1387
            idx -= 1
            update = 1
            br["region_skipped"] += 1
        if idx >= 0 and usable(idx) and regions[idx][0] <= p <= regions[idx][1]:      # :1391
            if update:
                seed = regions[idx][3]
                br["seed_emitted" if seed else "seed_empty"] += 1
                for ch in seed:
                    out.append(ch)
                    lq_i = _update_lqreg(lq, out, len(out) - 1, lq_i, st, br)
                    if lq_i >= 10:
                        truncated = "seed"
                        break
                update = 0
            else:
                br["inside_silent"] += 1
        else:
            out.append(w[i] & 0xff)
            update = 1
            br["base"] += 1
            if any(usable(k) and regions[k][0] <= p <= regions[k][1] for k in range(max(idx, 0))):
                br["lagging_base"] += 1              # a region below the index holds p: the index has not caught up
            lq_i = _update_lqreg(lq, out, len(out) - 1, lq_i, st, br)
            if lq_i >= 10:
                truncated = "base"
        i += 1
    olen = len(out)
    table = [list(s) for s in lq]
    if lq[lq_i][1] == (olen - 1) & U32:                                    # :1412
        lq_i += 1
        br["bump"] += 1
    code = 0
    if read_type == 3:                                                     # :1420-1444
        a = 0
        while a < olen and out[a] >= 97:
            a += 1
        z = 0
        while z < olen and out[olen - 1 - z] >= 97:
            z += 1
        if a + z < olen:
            br["hifi_ends" if a or z else "hifi_plain"] += 1
            lq_m, hq_m = a, olen - z
            total = (sum(lq[q][3] for q in range(min(lq_i, 11))) - (a + z)) & U32
        else:
            br["hifi_empty"] += 1
            lq_m = hq_m = total = 0
            code = 2
    elif lq_i:                                                             # :1445-1468
        lq_m, hq_m, p = 0, lq[0][0], lq[0][0]
        total = (lq[0][3] - lq[0][2]) & U32
        took = "raw_first"
        i = 1
        while i < 10 and lq[i][1]:
            if (lq[i][0] - lq[i - 1][1]) & U32 > p:
                lq_m, hq_m = lq[i - 1][1] + 1, lq[i][0]
                total = (lq[i][3] - lq[i][2]) & U32
                p = (lq[i][0] - lq[i - 1][1]) & U32
                took = "raw_middle"
            i += 1
        if i < 10 and (olen - lq[i - 1][1]) & U32 > p:
            lq_m, hq_m = lq[i - 1][1] + 1, olen
            total = lq[i][3]
            took = "raw_tail"
        br[took] += 1
    else:                                                                  # :1469-1480
        k = 0
        while k < olen and out[k] >= 97:
            k += 1
        br["raw_none_lead" if k else "raw_none"] += 1
        lq_m, hq_m = k, olen
        total = (lq[0][3] - k) & U32
    ln = 2 if code == 2 else (hq_m - lq_m) & U32
    seq = bytes(out[lq_m:hq_m]) if code != 2 else b""
    with np.errstate(all="ignore"):
        identity = np.float32(0) if code == 2 else np.float32(1) - np.float32(total) / np.float32(ln)
    clip_s = clip_e = 0
    trimmed = False
    if ln > 1000:                                                          # get_cns_from_align_tags' gate, then :2100-2128
        br["gate_len"] += 1
        if float(identity) > 0.8:
            br["gate_identity"] += 1
            br["trim_ran"] += 1
            trimmed = True
            km, cnt = _terminal_ssr(seq, 0)
            if cnt >= 4:
                clip_s = _clip_ssr(seq, ln, km, 0, br)
                br["clip_head"] += clip_s > 0
                while clip_s < ln and seq[clip_s] >= 97:
                    clip_s += 1
                    br["skip_lower"] += 1
            else:
                br["head_count_low"] += 1
            km, cnt = _terminal_ssr(seq, ln - 24 - 4 + 1)
            if cnt >= 4:
                clip_e = _clip_ssr(seq, ln, km, 1, br)
                br["clip_tail"] += clip_e > 0
                while clip_e < ln and seq[ln - clip_e - 1] >= 97:
                    clip_e += 1
                    br["skip_lower"] += 1
            else:
                br["tail_count_low"] += 1
            if clip_s + clip_e < ln - 10:
                seq = seq[clip_s:ln - clip_e]
                ln = ln - clip_s - clip_e
            else:
                br["len4"] += 1
                ln = 4
                seq = seq[:4]                       # the record the engine builds for a length of 4 carries the string's first four bytes
    return dict(len=ln, identity=identity, lq_total_len=total, out_len=olen, lq_m=lq_m, hq_m=hq_m, lq_i=lq_i, clip_s=clip_s, clip_e=clip_e,
                seq=seq, br=br, truncated=truncated, trimmed=trimmed, table=table, out=bytes(out))


FIELDS = ("len", "lq_total_len", "out_len", "lq_m", "hq_m", "lq_i", "clip_s", "clip_e")


def as_record(d):
    """A result of restate() or api.splice_batch() as one comparable list: every field, the float's bits, the bytes."""
    idn = np.float32(d["identity"])
    return [int(d[k]) for k in FIELDS] + ["nan" if np.isnan(idn) else int(idn.view(np.uint32)), bytes(d["seq"]).decode("latin-1")]


# ---- building jobs --------------------------------------------------------------------------------------------------------------
def job(text, regions=(), lstrip=0, rstrip=0, read_type=0, pos=None):
    """text: the consensus characters; positions 0, 1, 2 ... unless given"""
    t = np.frombuffer(text if isinstance(text, bytes) else text.encode(), dtype=np.uint8).astype(np.uint32)
    p = np.arange(t.shape[0], dtype=np.uint32) if pos is None else np.asarray(pos, dtype=np.uint32)
    return ((p << 8 | t).astype(np.uint32), lstrip, rstrip, [(int(a), int(b), int(c), bytes(d)) for a, b, c, d in regions], read_type)


def filler(n, seed=1, alphabet=b"ACGT"):
    """n upper-case bases without a repeat structure"""
    r = np.random.default_rng(seed)
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[r.integers(0, len(alphabet), n)])


def distinct27(seed=3):
    """27 bases whose 24 4-mers are all different (no terminal repeat: terminal_ssr's count is 1)"""
    r = np.random.default_rng(seed)
    while True:
        s = filler(27, int(r.integers(1 << 30)))
        if len({s[i:i + 4] for i in range(24)}) == 24:
            return s


def body(n, seed=1):
    """n >= 54 upper-case bases that begin and end without a terminal repeat"""
    return distinct27(seed) + filler(n - 54, seed + 1) + distinct27(seed + 2)


def closing(k, gap=14):
    """k lower-case runs of 102 bases, each behind `gap` upper-case ones: the twelfth upper-case base behind a run closes its slot"""
    return ("G" * gap + "a" * 102) * k


def directed_cases():
    c = []
    add = lambda name, *a, **kw: c.append((name, job(*a, **kw)))
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        add("n=%d" % n, filler(n, 5 + n))
    # the branches of update_lqreg
    add("lqreg/lower-only", "GGGG" + "a" * 5)
    add("lqreg/close-start0", "aaa" + "G" * 20)                              # a slot closed at index 0
    add("lqreg/gap-close", "GGG" + "a" * 102 + "G" * 30)
    add("lqreg/gap-close-at-101", "GGG" + "a" * 101 + "G" * 30)              # end == start + 100: emptied, not closed
    add("lqreg/gap-reset", "GGG" + "a" * 30 + "G" * 30)
    add("lqreg/short-reset", "GGG" + "aa" + "G" * 30)                        # hq_m reaches lqlen first
    add("lqreg/hold-then-extend", "GGG" + "a" * 30 + "GG" + "a" * 80 + "G" * 30)     # two runs joined over a short gap into one slot
    add("lqreg/hq-over-10", "GGG" + "a" * 40 + "G" * 5 + "aaa" + "G" * 9 + "a" * 70 + "G" * 40)   # three lower-case chars do not reset hq_m
    add("lqreg/lq_m-resets-hq", "GGG" + "a" * 40 + "G" * 5 + "aaaa" + "G" * 9 + "a" * 70 + "G" * 40)   # four do
    add("lqreg/run-over-chunk-edge", "G" * 40 + "a" * 102 + "G" * 50)
    add("lqreg/upper-run-steps-over-chunk-edge", "G" * 10 + "a" * 50 + "G" * 30 + "a" * 110 + "G" * 20)   # hq_m counts on from lane 60 into the next chunk
    add("lqreg/run-ends-on-lane-63", "G" * 4 + "a" * 60 + "G" * 70)
    add("lqreg/run-starts-on-lane-0", "G" * 64 + "a" * 102 + "G" * 70)
    # the tenth slot and the bump
    add("tenth/on-a-base", closing(10) + "G" * 50)
    add("tenth/nine-closed", closing(9) + "G" * 50)
    seed10 = ("G" * 3 + "a" * 102 + "G" * 20 + "TTT").encode()
    add("tenth/inside-a-seed", closing(9) + "G" * 14 + "C" * 10 + "G" * 40, regions=[(9 * 116 + 14, 9 * 116 + 23, 5, seed10)])
    add("bump/lq_i-0", "GGG" + "a" * 5)                                      # the string ends inside the first run
    add("bump/lq_i-0-long", "GGG" + "a" * 120)
    add("bump/lq_i-9", closing(9) + "G" * 14 + "a" * 7)
    add("bump/guard-slot", closing(10) + "G" * 12)                            # cut at the tenth slot with its last base: the guard slot is read
    add("bump/one-char", "a")                                                # end == 0 == len - 1 with lqlen 1
    add("bump/empty-string", "")                                             # len - 1 wraps
    # the raw choice
    add("raw/first", "G" * 300 + "a" * 102 + "G" * 50 + "a" * 102 + "G" * 20)
    add("raw/middle", "G" * 30 + "a" * 102 + "G" * 300 + "a" * 102 + "G" * 20)
    add("raw/tail", "G" * 30 + "a" * 102 + "G" * 50 + "a" * 102 + "G" * 300)
    add("raw/tail-open-slot-counted", "G" * 30 + "a" * 102 + "G" * 300 + "aaa" + "G" * 5)     # lq[i].lq_total_len of an emptied slot
    add("raw/none", "G" * 100)
    add("raw/none-leading-lower", "aaaa")                                    # all lower case without an upper one: lq_i is bumped
    add("raw/none-short-runs", "G" * 10 + "aa" + "G" * 30 + "aaa" + "G" * 30)
    add("raw/len-0", "aaa" + "G", rstrip=1)                                  # bumped slot at start 0: the first stretch [0, 0)
    # HiFi
    add("hifi/plain", "G" * 50 + "a" * 5 + "G" * 50, read_type=3)
    add("hifi/both-ends", "aaa" + "G" * 50 + "a" * 120 + "G" * 50 + "aa", read_type=3)
    add("hifi/all-lower", "a" * 70, read_type=3)
    add("hifi/empty", "", read_type=3)
    add("hifi/ends-over-chunks", "a" * 70 + "G" * 3 + "a" * 130, read_type=3)
    # regions (engine order: descending positions)
    t = filler(200, 9)
    sd = b"ttGGGGcc"
    for ln in (0, -1, -2, 7):
        add("region/len=%d" % ln, t, regions=[(50, 60, ln, sd)])
    add("region/seed-len-0", t, regions=[(50, 60, 5, b"")])
    add("region/two-adjacent", t, regions=[(61, 70, 5, b"CCCC"), (50, 60, 5, b"TTTT")])
    add("region/adjacent-second-unusable", t, regions=[(61, 70, 0, b"CCCC"), (50, 60, 5, b"TTTT")])
    # the index steps down one region a word: three regions lie between two neighbouring positions, the word behind them is inside
    # the lowest of the three and still comes out as a base
    pos = list(range(40)) + list(range(100, 160))
    add("region/lagging-index", filler(100, 10), pos=pos,
        regions=[(150, 155, 5, b"AAAA"), (100, 104, 5, b"CC"), (60, 70, 5, b"TT"), (50, 55, 5, b"GG"), (45, 48, 5, b"AA")])
    add("region/under-lstrip", t, regions=[(0, 12, 5, b"TTTT")], lstrip=8)
    add("region/past-rstrip", t, regions=[(190, 250, 5, b"TTTT")], rstrip=5)
    pos = list(range(50)) + [50] * 5 + list(range(51, 60)) + [60] * 4 + list(range(61, 150))
    add("region/insertions-on-the-edges", filler(len(pos), 11), pos=pos, regions=[(50, 60, 5, b"ggTT")])
    add("region/none-usable", t, regions=[(150, 160, 0, b"A"), (100, 110, -1, b"C"), (50, 60, 0, b"G")])
    add("region/seed-over-chunk-edge", filler(130, 12), regions=[(60, 62, 5, filler(150, 13) + b"acgt" * 30)])
    add("region/many-small", filler(300, 14), regions=[(k, k, 5, b"t") for k in range(290, 5, -3)])
    add("region/whole-string", filler(100, 15), regions=[(0, 1000, 5, b"GGaaGG")])
    add("region/hifi", "aa" + filler(100, 16).decode() + "aa", regions=[(50, 60, -2, b"ccGGGGcc")], read_type=3)
    # the trim
    B = lambda n, s=1: body(n, s).decode()
    add("ssr/len-1000", "AC" * 60 + B(880))
    add("ssr/len-1001", "AC" * 60 + B(881))
    add("ssr/count-3", "ACACACAC" + distinct27(1).decode() + B(1100))
    add("ssr/count-4", "ACACACACAC" + distinct27(1).decode() + B(1100))
    add("ssr/head", "AC" * 60 + B(1100))
    add("ssr/tail", B(1100) + "GT" * 70)
    add("ssr/both", "AC" * 60 + B(1100) + "GT" * 70)
    add("ssr/p-100", "AC" * 52 + B(1100))
    add("ssr/p-101", "G" + "AC" * 52 + B(1100))
    add("ssr/tail-p-100", B(1100) + "AC" * 52)
    add("ssr/tail-p-101", B(1100) + "AC" * 52 + "G")
    add("ssr/break", "AC" * 60 + "G" * 30 + "AC" * 20 + "G" * 40 + B(1100))          # a second block near the first: p = p1
    add("ssr/reset", "AC" * 60 + "G" * 30 + "AC" * 60 + "G" * 40 + B(1100))          # a long second block: p1 = p2 = 0, then p1 again
    add("ssr/reset-then-break", "AC" * 60 + "G" * 30 + "AC" * 60 + "G" * 30 + "AC" * 10 + "G" * 40 + B(1100))
    add("ssr/lower-after-clip", "AC" * 60 + "acgtacgt" + B(1100))
    add("ssr/lower-before-tail-clip", B(1100) + "tgca" * 20 + "TG" * 70)
    add("ssr/leaves-10", "AC" * 520)                                         # both clips run through the string: len 4
    add("ssr/n-in-window", "ACAN" * 40 + B(1100))
    add("ssr/m-tail", B(1100) + "GTGM" * 40)
    add("ssr/period-3", "ACG" * 50 + B(1100))
    add("ssr/hifi", "aa" + "AC" * 60 + B(1100) + "GT" * 70 + "a", read_type=3)
    add("ssr/after-the-choice", "G" * 5 + "a" * 102 + "AC" * 60 + B(1100) + "GT" * 70 + "a" * 102 + "G" * 8)
    return c


def gate_family(full=False):
    """For len in 1001..4096 and lq_total_len within 2 of len / 5 (identity about 0.8, a float compared as a double), with an SSR head
    so that trimming changes the answer: the lower-case characters are single ones 4 apart, which no slot keeps.  full: every length
    (15,480 jobs); otherwise every length below 1100, every 37th above and the powers of two with their neighbours (925 jobs)."""
    lens = range(1001, 4097) if full else list(range(1001, 1100)) + list(range(1100, 4097, 37)) + [2047, 2048, 2049, 4095, 4096]
    out = []
    for ln in lens:
        base = np.frombuffer(("AC" * 60 + "GT" * ((ln - 120) // 2 + 1))[:ln].encode(), dtype=np.uint8)
        for d in (-2, -1, 0, 1, 2):
            t = ln // 5 + d
            s = base.copy()
            s[130:130 + 4 * t:4] |= 0x20
            assert 130 + 4 * (t - 1) < ln
            out.append(("gate/%d/%d" % (ln, t), job(s.tobytes())))
    return out


def check_directed():
    """Asserts, from the restatement alone, that every directed case reaches the shape it is named for."""
    cases = dict(directed_cases())
    r = {k: restate(w) for k, w in cases.items()}
    b = lambda k: r[k]["br"]
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        assert r["n=%d" % n]["out_len"] == n and r["n=%d" % n]["len"] == (n if n != 1 else 0)    # (one base: bumped, the tail [1, 1))
    assert b("lqreg/lower-only")["lower_open"] == 1 and b("lqreg/lower-only")["lower_extend"] == 4
    assert b("lqreg/close-start0")["close_start0"] == 1 and r["lqreg/close-start0"]["table"][0][:3] == [0, 2, 3]
    assert b("lqreg/gap-close")["gap_close"] == 1 and b("lqreg/gap-close-at-101")["gap_close"] == 0 and b("lqreg/gap-close-at-101")["gap_reset"] == 1
    assert b("lqreg/gap-reset")["gap_reset"] == 1 and b("lqreg/gap-reset")["short_reset"] == 0 and b("lqreg/gap-reset")["hold"] == 11
    assert b("lqreg/short-reset")["short_reset"] == 1 and b("lqreg/short-reset")["gap_reset"] == 0 and b("lqreg/short-reset")["hold"] == 1
    h = r["lqreg/hold-then-extend"]
    assert h["br"]["hold"] >= 2 and h["br"]["gap_close"] == 1 and h["table"][0] == [3, 114, 110, 110] and h["lq_i"] == 1
    assert b("lqreg/hq-over-10")["lq_m_resets_hq"] == 0 and b("lqreg/lq_m-resets-hq")["lq_m_resets_hq"] == 2
    assert b("lqreg/hq-over-10")["gap_close"] == 0 and b("lqreg/lq_m-resets-hq")["gap_close"] == 1
    assert r["lqreg/hq-over-10"]["table"] != r["lqreg/lq_m-resets-hq"]["table"]
    for k in ("lqreg/run-over-chunk-edge", "lqreg/run-ends-on-lane-63", "lqreg/run-starts-on-lane-0"):
        assert b(k)["gap_close"] == (0 if "63" in k else 1), k
    u = cases["lqreg/upper-run-steps-over-chunk-edge"]
    assert chr(u[0][60] & 0xff) == "G" and chr(u[0][59] & 0xff) == "a" and b("lqreg/upper-run-steps-over-chunk-edge")["hold"] >= 10
    assert r["tenth/on-a-base"]["truncated"] == "base" and r["tenth/on-a-base"]["out_len"] == 10 * 116 + 12 and r["tenth/on-a-base"]["lq_i"] == 10
    assert r["tenth/nine-closed"]["truncated"] is None and r["tenth/nine-closed"]["lq_i"] == 9
    s = r["tenth/inside-a-seed"]
    assert s["truncated"] == "seed" and s["out_len"] == 9 * 116 + 14 + 3 + 102 + 12 and s["out"].endswith(b"a" + b"G" * 12)
    assert r["bump/lq_i-0"]["lq_i"] == 1 and r["bump/lq_i-0-long"]["lq_i"] == 1 and r["bump/lq_i-9"]["lq_i"] == 10
    assert r["bump/guard-slot"]["truncated"] == "base" and r["bump/guard-slot"]["br"]["bump"] == 0 and r["bump/guard-slot"]["lq_i"] == 10
    assert r["bump/guard-slot"]["out_len"] == 10 * 116 + 12
    assert r["bump/one-char"]["br"]["bump"] == 1 and r["bump/empty-string"]["br"]["bump"] == 0 and r["bump/empty-string"]["len"] == 0
    assert r["bump/lq_i-9"]["br"]["gap_close"] == 9
    assert b("raw/first")["raw_first"] == 1 and r["raw/first"]["len"] == 300
    assert b("raw/middle")["raw_middle"] == 1 and r["raw/middle"]["len"] == 300 and r["raw/middle"]["lq_m"] == 132
    assert b("raw/tail")["raw_tail"] == 1 and r["raw/tail"]["len"] == 300
    assert b("raw/tail-open-slot-counted")["raw_tail"] == 1 and r["raw/tail-open-slot-counted"]["lq_total_len"] == 3
    assert b("raw/none")["raw_none"] == 1 and r["raw/none"]["len"] == 100
    assert r["raw/none-leading-lower"]["lq_i"] == 1 and r["raw/none-leading-lower"]["len"] == 0
    assert b("raw/none-short-runs")["raw_none"] == 1 and r["raw/none-short-runs"]["lq_total_len"] == 5
    assert r["raw/len-0"]["len"] == 0 and r["raw/len-0"]["lq_i"] == 1 and np.isnan(r["raw/len-0"]["identity"])
    assert b("hifi/plain")["hifi_plain"] == 1 and r["hifi/plain"]["lq_total_len"] == 0     # no slot closed: lq_i 0, nothing summed
    e = r["hifi/both-ends"]
    assert e["br"]["hifi_ends"] == 1 and e["lq_m"] == 3 and e["hq_m"] == e["out_len"] - 2 and e["lq_total_len"] == 120
    assert r["hifi/all-lower"]["len"] == 2 and r["hifi/all-lower"]["seq"] == b"" and r["hifi/empty"]["len"] == 2
    assert r["hifi/ends-over-chunks"]["lq_m"] == 70 and r["hifi/ends-over-chunks"]["len"] == 3
    for ln in (0, -1):
        assert b("region/len=%d" % ln)["seed_emitted"] == 0 and r["region/len=%d" % ln]["out_len"] == 200
    for ln in (-2, 7):
        assert b("region/len=%d" % ln)["seed_emitted"] == 1 and r["region/len=%d" % ln]["out_len"] == 200 - 11 + 8
    assert b("region/seed-len-0")["seed_empty"] == 1 and r["region/seed-len-0"]["out_len"] == 189
    assert b("region/two-adjacent")["seed_emitted"] == 2 and b"TTTTCCCC" in r["region/two-adjacent"]["out"]
    assert b("region/adjacent-second-unusable")["seed_emitted"] == 1 and r["region/adjacent-second-unusable"]["out_len"] == 200 - 11 + 4
    g = r["region/lagging-index"]
    assert g["br"]["lagging_base"] >= 1 and g["br"]["seed_emitted"] == 2, g["br"]
    assert b("region/under-lstrip")["seed_emitted"] == 1 and r["region/under-lstrip"]["out"].startswith(b"TTTT")
    assert b("region/past-rstrip")["seed_emitted"] == 1 and r["region/past-rstrip"]["out"].endswith(b"TTTT")
    assert b("region/insertions-on-the-edges")["seed_emitted"] == 1 and b("region/insertions-on-the-edges")["inside_silent"] == 5 + 9 + 4 - 1
    assert b("region/none-usable")["seed_emitted"] == 0 and b("region/none-usable")["region_skipped"] == 3
    assert r["region/seed-over-chunk-edge"]["out_len"] == 130 - 3 + 270
    assert b("region/many-small")["seed_emitted"] == 95 and b("region/whole-string")["seed_emitted"] == 1 and r["region/whole-string"]["out_len"] == 6
    assert r["region/hifi"]["lq_m"] == 2 and b"ccGGGGcc" in r["region/hifi"]["seq"]
    assert r["ssr/len-1000"]["len"] == 1000 and not r["ssr/len-1000"]["trimmed"] and r["ssr/len-1001"]["trimmed"] and r["ssr/len-1001"]["clip_s"] > 0
    assert b("ssr/count-3")["head_count_low"] == 1 and b("ssr/count-4")["head_count_low"] == 0 and r["ssr/count-4"]["clip_s"] == 0
    assert r["ssr/head"]["clip_s"] == 120 and r["ssr/head"]["clip_e"] == 0 and r["ssr/tail"]["clip_s"] == 0 and r["ssr/tail"]["clip_e"] == 139
    assert r["ssr/both"]["clip_s"] == 120 and r["ssr/both"]["clip_e"] == 139 and r["ssr/both"]["len"] == 1101     # (the tail walk is one index short)
    assert r["ssr/p-100"]["clip_s"] == 0 and r["ssr/p-101"]["clip_s"] == 105
    assert r["ssr/tail-p-100"]["clip_e"] == 0 and r["ssr/tail-p-101"]["clip_e"] == 105
    assert b("ssr/break")["ssr_break"] == 1 and r["ssr/break"]["clip_s"] == 120
    assert b("ssr/reset")["ssr_reset"] == 1 and r["ssr/reset"]["clip_s"] == 270
    assert b("ssr/reset-then-break")["ssr_reset"] == 1 and b("ssr/reset-then-break")["ssr_break"] == 1
    assert r["ssr/lower-after-clip"]["clip_s"] == 128 and r["ssr/lower-before-tail-clip"]["clip_e"] == 220 and b("ssr/lower-before-tail-clip")["skip_lower"] == 80
    assert r["ssr/leaves-10"]["len"] == 4 and r["ssr/leaves-10"]["seq"] == b"ACAC" and b("ssr/leaves-10")["len4"] == 1
    assert r["ssr/n-in-window"]["clip_s"] == 160 and r["ssr/m-tail"]["clip_e"] > 150 and r["ssr/period-3"]["clip_s"] > 150
    assert r["ssr/hifi"]["clip_s"] == 120 and r["ssr/hifi"]["clip_e"] == 139 and r["ssr/hifi"]["lq_m"] == 2
    a = r["ssr/after-the-choice"]
    assert a["lq_m"] == 107 and a["clip_s"] == 120 and a["clip_e"] == 139 and a["len"] == 1101
    return cases


def check_gate_family(fam):
    """Both sides of the gate occur, and where it opens the trim changes the answer."""
    res = [restate(w) for k, w in fam]
    opened = [x for x in res if x["trimmed"]]
    assert len(opened) > 100 and len(res) - len(opened) > 100, (len(opened), len(res))
    assert all(x["clip_s"] == 120 for x in opened) and all(x["clip_s"] == 0 and x["len"] > 1000 for x in res if not x["trimmed"])
    return res


# ---- fuzz -----------------------------------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bases(rng, n):
    return bytes(_ACGT[rng.integers(0, 4, n)])


def fuzz_jobs(n, max_words, seed=2424, exact=False, first=0):
    """Six styles, by job index modulo 6.  0, 3: strings of upper-case runs and lower-case runs of four kinds (1..3, 4..40, 101..130 --
    these close a slot -- and single characters behind short gaps; every other job of style 0 ends in upper case alone), regions with pseudo-seeds of mixed case, positions with insertions
    and jumps.  1: long strings whose table fills -- lower-case runs of 101..130 behind 12..40 upper-case bases, or (every other job of the style) an
    upper-case string whose regions' pseudo-seeds each hold such a run, so that the tenth slot opens inside a pseudo-seed.  2: three
    small regions at every jump of the positions, two inside the jump and one around the word behind it: the lagging index.  4, 5:
    long strings with few lower-case characters that begin and / or end with a short-period repeat (a second block behind a gap: the
    break and the reset; a twelfth: nothing but the repeat), so that the trim runs.  A third of the jobs is HiFi, three in fifteen
    of lower case alone; strips on two thirds."""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(first, first + n):
        style = it % 6
        lo_total = 1 if style in (0, 2, 3) else min(max_words, 1300 if style >= 4 else 1700)
        total = max_words if exact else int(rng.integers(lo_total, max_words + 1))
        seeds_close = style == 1 and (it // 6) % 2 == 1
        kinds = rng.choice(5, total // 3 + 2, p=[0.45, 0.2, 0.15, 0.12, 0.08] if style < 4 else [0.9, 0.06, 0.03, 0.0, 0.01])
        if style == 1:
            kinds = np.where(np.arange(kinds.shape[0]) % 2 == 0, 0, 0 if seeds_close else 3)
        parts = []
        for k in kinds.tolist():
            if k == 0:
                parts.append(_bases(rng, int(rng.integers(12, 41) if style == 1 else rng.integers(1, 60 if style != 4 else 400))))
            elif k == 1:
                parts.append(_bases(rng, int(rng.integers(1, 4))).lower())
            elif k == 2:
                parts.append(_bases(rng, int(rng.integers(4, 41))).lower())
            elif k == 3:
                parts.append(_bases(rng, int(rng.integers(101, 131))).lower())
            else:
                parts.append(b"".join(b"a" + _bases(rng, int(rng.integers(1, 12))) for _ in range(int(rng.integers(2, 6)))))
        text = bytearray(b"".join(parts)[:total])
        if style == 0 and (it // 6) % 2 and len(text) > 30:
            text[-(len(text) // 3):] = _bases(rng, len(text) // 3)          # a long upper-case tail: the tail stretch wins
        if it % 7 == 3 and len(text) > 8:
            text[:int(rng.integers(1, 5))] = b"a"                            # a slot that opens at index 0
        if it % 3 == 2 and it % 2 == 0 and len(text) > 8:
            text[-3:] = b"acg"                                                # HiFi: a lower-case run at the end
        if it % 15 in (2, 8, 11):
            text = bytearray(bytes(text).lower())                            # (HiFi jobs: it % 3 == 2) nothing but lower case
        if style >= 4 and len(text) > 1200:
            unit = [b"AC", b"GT", b"ACG", b"ACAN", b"A", b"GTGM", b"TTG", b"CA"][(it // 6) % 8]
            def block(at, k, back):
                rep = (unit * k)[:k]
                if back:
                    text[len(text) - at - k:len(text) - at] = rep
                else:
                    text[at:at + k] = rep
            if it % 12 == 11:
                block(0, len(text), False)
            if it % 3 != 0:
                k = int(rng.integers(40, 200))
                block(0, k, False)
                if (it // 6) % 2 == 1:
                    text[k:k + 6] = b"acgtac"
                if it % 5 in (0, 2, 4):                                      # a second block behind a gap: the break or the reset
                    block(k + int(rng.integers(25, 60)), int(rng.integers(20, 60) if (it // 6) % 5 == 0 else rng.integers(110, 200)), False)
            if it % 3 != 1:
                k = int(rng.integers(40, 200))
                block(0, k, True)
                if (it // 6) % 2 == 0:
                    text[-k - 5:-k] = b"tgcat"
                if it % 5 in (1, 3):
                    block(k + int(rng.integers(25, 60)), int(rng.integers(20, 60) if (it // 6) % 5 == 0 else rng.integers(110, 200)), True)
        m = len(text)
        step = np.ones(m, dtype=np.int64)
        step[rng.random(m) < 0.05] = 0                                       # insertion columns keep the position
        jumps = rng.random(m) < 0.01
        step[jumps] = rng.integers(2, 40, int(jumps.sum()))
        pos = np.cumsum(step)
        top = int(pos[-1]) if m else 0
        regions = []
        if style == 2:
            for j in np.nonzero(step >= 8)[0].tolist()[::-1]:
                if j == 0 or j + 6 >= m or (regions and regions[-1][0] <= int(pos[j]) + 3):
                    continue
                a = int(pos[j - 1])
                regions += [(int(pos[j]) - 1, int(pos[j]) + 3, 5, _bases(rng, 4).lower()), (a + 3, a + 4, 5, b"TT"), (a + 1, a + 2, 5, b"GG")]
        elif style != 5:
            at = top + 5
            for _ in range(int(rng.integers(12, 16)) if seeds_close else int(rng.integers(0, 2 + m // 150))):
                end = at - int(rng.integers(1, 2 + max(1, top // (20 if seeds_close else 8)))) if rng.random() > 0.15 else at - 1     # (a sixth: adjacent)
                start = end - int(rng.integers(0, 30))
                if start < 0:
                    break
                ln = 5 if seeds_close else int(rng.choice([5, 5, 5, -2, 0, -1]))
                sl = 130 if seeds_close else int(rng.choice([0, 1, 5, 20, 60, 130]))
                sd = bytearray(_bases(rng, sl))
                if seeds_close:
                    sd[3:113] = bytes(sd[3:113]).lower()
                elif sl and rng.random() < 0.5:
                    a = int(rng.integers(0, sl))
                    z = a + int(rng.integers(1, 1 + (110 if rng.random() < 0.3 else 6)))
                    sd[a:z] = bytes(sd[a:z]).lower()
                regions.append((start, end, ln, bytes(sd)))
                at = start
        lstrip = int(rng.integers(0, 1 + min(m, 6))) if it % 3 == 0 else 0
        rstrip = int(rng.integers(0, 1 + min(m - lstrip, 6))) if it % 3 == 1 else 0
        out.append(job(bytes(text), regions=regions, lstrip=lstrip, rstrip=rstrip, read_type=3 if it % 3 == 2 else 0, pos=pos))
    return out


def long_job(n=100000):
    return fuzz_jobs(1, n, seed=77, exact=True, first=4)[0]      # (a style whose table does not fill: the whole string is walked)


def branch_totals(jobs):
    tot = dict.fromkeys(BRANCHES, 0)
    extra = dict(truncated_seed=0, truncated_base=0, trimmed_head=0, trimmed_tail=0)
    for w in jobs:
        r = restate(w)
        for k, v in r["br"].items():
            tot[k] += v
        extra["truncated_seed"] += r["truncated"] == "seed"
        extra["truncated_base"] += r["truncated"] == "base"
        extra["trimmed_head"] += r["clip_s"] > 0
        extra["trimmed_tail"] += r["clip_e"] > 0
    return tot, extra


def job_set(n_fuzz, max_words, gate=False, n_long=0, full_gate=False):
    jobs = [w for k, w in directed_cases()] + ([w for k, w in gate_family(full_gate)] if gate else []) + fuzz_jobs(n_fuzz, max_words)
    if n_long:
        jobs.append(long_job(n_long))
    return jobs


def result_bytes(recs):
    return sum(len(r[-1]) for r in recs)


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run --------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, splice_util as su
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
if what == "batch":             # directed + fuzz jobs: device, host flag and the restatement, in calls of `call` jobs
    n_fuzz, max_words, gate = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    calls = [int(x) for x in sys.argv[6].split(",")]
    jobs = su.job_set(n_fuzz, max_words, gate=bool(gate))
    exp = [su.as_record(su.restate(w)) for w in jobs]
    out = dict(n=len(jobs), bytes=su.result_bytes(exp), bad_dev={})
    host = [su.as_record(r) for r in api.splice_batch(jobs, host=True)]
    out["bad_host"] = [i for i in range(len(jobs)) if host[i] != exp[i]][:20]
    api.reset_stats()
    for call in calls:
        call = call or len(jobs)
        dev = {}
        for a in range(0, len(jobs), call):
            for k, r in enumerate(api.splice_batch(jobs[a:a + call])):
                dev[a + k] = su.as_record(r)
        out["bad_dev"][str(call)] = [i for i in dev if dev[i] != exp[i]][:20]
    out["stats"] = api.splice_stats()
    print(json.dumps(out))
elif what == "gpu":             # the big set: all jobs against the host statement, a part against the restatement; shuffled; singly
    n_fuzz, max_words, n_long = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    jobs = su.job_set(n_fuzz, max_words, gate=True, n_long=n_long, full_gate=True)
    n_dir = len(jobs) - n_fuzz - 1
    host = [su.as_record(r) for r in api.splice_batch(jobs, host=True)]
    api.reset_stats()
    dev = []
    for a in range(0, len(jobs), 1000):
        dev += [su.as_record(r) for r in api.splice_batch(jobs[a:a + 1000])]
    st = api.splice_stats()
    out = dict(n=len(jobs), n_dir=n_dir, longest=max(w[0].shape[0] for w in jobs), bytes=su.result_bytes(host), stats=st)
    out["bad_dev"] = [i for i in range(len(jobs)) if dev[i] != host[i]][:20]
    some = list(range(82)) + list(range(82, n_dir, 16)) + list(range(n_dir, len(jobs) - 1, 3)) + [len(jobs) - 1]
    out["bad_restate"] = [i for i in some if su.as_record(su.restate(jobs[i])) != dev[i]][:20]
    out["n_restate"] = len(some)
    perm = np.random.default_rng(5).permutation(len(jobs))
    got = []
    for a in range(0, len(jobs), 1000):
        got += [su.as_record(r) for r in api.splice_batch([jobs[i] for i in perm[a:a + 1000]])]
    out["bad_shuffled"] = [int(i) for k, i in enumerate(perm) if got[k] != host[int(i)]][:20]
    singly = list(range(0, 82, 7)) + list(range(82, n_dir, 997)) + list(range(n_dir + 50, len(jobs), 97)) + [len(jobs) - 1]
    out["bad_singly"] = [i for i in singly if su.as_record(api.splice_batch([jobs[i]])[0]) != host[i]][:20]
    out["n_singly"] = len(singly)
    print(json.dumps(out))
elif what == "piles":           # fixtures through correct_batch, grouped by the arguments a call takes once
    import util, rank_util
    piles = rank_util.pile_sets(sys.argv[3].split(","), None)
    rec, bad = {}, []
    api.reset_stats()
    for key, members in util.edge_groups(piles).items():
        for p, got in zip(members, util.edge_correct_group(api, key, members)):
            w = util.edge_wrong(p, got)
            if w:
                bad.append(w)
            rec[p["tag"]] = [int(got[0]), int(np.float32(got[1]).view(np.uint32)) if got[0] > 4 else 0, got[2].decode() if got[0] > 4 else ""]
    print(json.dumps(dict(rec=rec, bad=bad, n=len(piles), stats=api.splice_stats(), all_stats=api.stats(), phase=api.phase_stats(),
                          modes=api.cns_mode_stats())))
elif what == "args":
    lib = api.load() if sys.argv[1] != "simt" else api._LIB
    out = {}
    def call(words, lstrip=0, rstrip=0, regions=(), flags=0, null_words=False, null_regions=False, null_res=False, null_seqs=False, n_words=None):
        w = np.ascontiguousarray(words, dtype=np.uint32)
        rg = (api.SpliceRegion * max(1, len(regions)))(*[api.SpliceRegion(a, b, c, len(d) if e is None else e, d) for a, b, c, d, e in regions])
        job = (api.SpliceJob * 1)(api.SpliceJob(None if null_words else w.ctypes.data, w.size if n_words is None else n_words, lstrip, rstrip,
                                                len(regions), None if null_regions else rg, 0, 0))
        res = (api.SpliceResult * 1)()
        C.memset(res, 0x55, C.sizeof(res))
        sw = C.c_void_p(0x55)
        rc = lib.ndgpu_splice_batch(job, 1, flags, None if null_res else res, None if null_seqs else C.byref(sw))
        return [rc, bytes(res) == b"\x55" * C.sizeof(res) and sw.value == 0x55]
    ok = (np.arange(10, 20, dtype=np.uint32) << 8) | 71
    for flags in (0, 1):
        f = "/%%d" %% flags
        out["ok" + f] = call(ok, flags=flags)
        out["ok-regions" + f] = call(ok, regions=[(12, 13, 5, b"TT", None)], flags=flags)
        out["strips-meet" + f] = call(ok, lstrip=4, rstrip=6, flags=flags)
        out["strips-cross" + f] = call(ok, lstrip=5, rstrip=6, flags=flags)
        out["descending" + f] = call(ok[::-1].copy(), flags=flags)
        out["descending-under-strip" + f] = call(np.concatenate([ok[:2][::-1], ok[2:]]), lstrip=1, flags=flags)
        out["equal-positions" + f] = call(np.repeat(ok, 2), flags=flags)
        out["start-above-end" + f] = call(ok, regions=[(14, 13, 5, b"TT", None)], flags=flags)
        out["null-words" + f] = call(ok, null_words=True, flags=flags)
        out["null-words-empty" + f] = call(ok, null_words=True, n_words=0, flags=flags)
        out["null-regions" + f] = call(ok, regions=[(12, 13, 5, b"TT", None)], null_regions=True, flags=flags)
        out["null-seed" + f] = call(ok, regions=[(12, 13, 5, None, 3)], flags=flags)
        out["null-seed-empty" + f] = call(ok, regions=[(12, 13, 5, None, 0)], flags=flags)
        out["null-res" + f] = call(ok, null_res=True, flags=flags)
        out["null-seqs" + f] = call(ok, null_seqs=True, flags=flags)
        out["n0" + f] = lib.ndgpu_splice_batch(None, 0, flags, None, None)
        out["n-neg" + f] = lib.ndgpu_splice_batch(None, -1, flags, None, None)
    out["py-empty"] = api.splice_batch([]) == [] and api.splice_batch([], host=True) == []
    big = su.job("G" * 40, pos=list(range(40)))
    far = (big[0].copy(), 0, 0, [], 0)
    far[0][-1] = ((1 << 21) - 1) << 8 | 71           # a position outside the words' range: answered by the host statement
    api.reset_stats()
    got = api.splice_batch([big, far])
    out["far"] = [su.as_record(g) == su.as_record(su.restate(w)) for g, w in zip(got, (big, far))]
    out["far-stats"] = api.splice_stats()
    print(json.dumps(out))
"""


def child(lib, what, *args, timeout=1500, **env):
    # no switch of the caller's reaches the child
    e = {k: v for k, v in os.environ.items() if not k.startswith(("NDGPU_SPLICE", "NDGPU_CNS", "NDGPU_RANK", "NDGPU_POA", "NDGPU_TRACE", "NDGPU_EXTRACT"))}
    e.update(env)
    if lib == "simt":
        e.setdefault("NDGPU_CONTEXTS", "1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE, os.path.join(HERE, "simt")), lib, what, *[str(a) for a in args]],
                         env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    r["trace"] = [ln for ln in out.stderr.splitlines() if ln.startswith("[ndgpu trace] splice")]
    return r


# every other opt-in of the engine, for the runs beside them
OTHER_OPT_INS = dict(NDGPU_CNS_DEVICE="1", NDGPU_CNS_HIFI="1", NDGPU_CNS_FAST="1", NDGPU_RANK_DEVICE="1", NDGPU_POA_DEVICE="1",
                     NDGPU_POA_RESIDENT="1", NDGPU_PHASE_DEVICE="1")
PILE_ENVS = [dict(NDGPU_SPLICE_DEVICE="1", NDGPU_TRACE="1"), dict(OTHER_OPT_INS, NDGPU_SPLICE_DEVICE="1"),
             dict(NDGPU_SPLICE_DEVICE="1", NDGPU_SPLICE_DECLINE="2"), dict(NDGPU_SPLICE_DEVICE="1", NDGPU_SPLICE_HOST="1"), {}]


def check_pile_runs(runs, n_piles):
    """The five runs of the engine over the fixture piles: the switch alone, beside every other opt-in, with every second job declined,
    on a backend that does not offer the entry, and unset."""
    alone, beside, declined, no_entry, unset = runs
    for r in runs:
        assert r["n"] == n_piles and r["bad"] == [], r["bad"]                 # the compiled reference's recorded answers
        assert r["rec"] == unset["rec"]                                       # length, float32 identity bits, bases
    for r in (alone, beside):
        st = r["stats"]
        assert 0 < st["jobs"] <= n_piles and st["declined"] == 0 and st["launches"] > 0, st
        assert st["h2d_bytes"] > 0 and st["d2h_bytes"] >= 48 * st["jobs"] and st["ms"] > 0, st
    assert alone["stats"]["jobs"] == declined["stats"]["jobs"] and len(alone["trace"]) == alone["stats"]["launches"]
    assert declined["stats"]["declined"] == declined["stats"]["jobs"] // 2 > 0, declined["stats"]
    assert 0 < declined["stats"]["d2h_bytes"] < alone["stats"]["d2h_bytes"]
    assert beside["modes"]["hifi_jobs"] > 0 and beside["phase"]["piles"] > 0 and beside["all_stats"]["cns_jobs"] > 0      # the others ran too
    for r in (no_entry, unset):
        assert all(v == 0 for v in r["stats"].values()), r["stats"]
