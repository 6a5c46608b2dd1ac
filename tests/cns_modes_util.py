"""Shared by tests/test_simt_cns_modes.py and tests/test_zz_gpu_cns_modes.py: the HiFi and -fast forms of the loop behind the main
walk restated in Python from the reference's lines (lib/nextcorrect.c:1807-1860 with the verdict :1864-1865, and :1724-1777), not from
the library, with a count of how often each branch was taken; directed walks per mode, each the smallest shape at which K21
(cns_walk_kernel, msa_kernels.hip: 64 items a chunk, a wave-uniform automaton that jumps along ballots) can go wrong, and
check_directed(), which asserts from the restatements that each reaches its shape; a seeded fuzz generator per mode; and the child
processes that run the batched entry (api.cns_walk_batch) and the engine (api.correct_batch) under the switches that are read once
per process.

A walk here is (steps, min_cov, lq_max_len, ratio, mode, seed): steps an int array [n, 4] of t_pos, link, cov, base (A0 T1 G2 C3, 4 a
gap, 5 N), mode 1 HiFi (seed: ASCII bytes) or 2 -fast (seed None)."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

INT_TO_BASE = b"ATGC-N"
_CODE = np.full(256, 4, dtype=np.int64)            # base_to_int, lib/nextcorrect.c:42-50
for _ch, _v in ((b"Aa", 0), (b"Tt", 1), (b"Gg", 2), (b"Cc", 3), (b"N", 5), (b"M", 6)):
    for _c in _ch:
        _CODE[_c] = _v

K_BRANCHES = ("cov4", "cov4_open", "bad_open", "bad_extend", "held_near", "held_pos", "push", "merge", "clamp", "upper", "lower")
F_BRANCHES = ("lower_open", "lower_extend", "lower_index0", "close_len", "close_slot0", "empty", "truncate", "scan_take", "scan_skip",
              "tail_take", "tail_skip", "no_closed")


# ---- the restatements -----------------------------------------------------------------------------------------------------------
def restate_kmer(steps, seed, min_cov, ratio=0.8):
    """:1807-1860 -> dict: bases (pos << 8 | char at index p, before reverse_consensus_base), regions [(start, end)], len,
    lqseq_total_length, ok (:1864-1865), br."""
    ref = _CODE[np.frombuffer(seed, dtype=np.uint8)].tolist()    # ref_tag->align_tags[t].q_base
    lq_min_length, dag_min_qv = 2, 80
    p = lq = 0
    lq_s = lq_e = -1
    total = 0
    pos, chars, regions = [], [], []
    br = dict.fromkeys(K_BRANCHES, 0)
    for t_pos, link, cov, base in steps.tolist():
        if base == 4:                                            # :1808
            continue
        pos.append(t_pos)                                        # :1814
        qv = 100 * link // cov                                   # :1816
        if cov < 4:                                              # :1818-1821
            br["cov4_open" if lq else "cov4"] += 1
            lq = 0
            lq_s = -1
            total += 1
        elif qv < dag_min_qv or base != ref[t_pos]:              # :1822-1828
            br["bad_open" if lq_s == -1 else "bad_extend"] += 1
            if lq_s == -1:
                lq_s = p
            lq_e = p
            lq = 1
            total += 1
        elif lq and p - lq_e > 2 * lq_min_length and pos[p] != pos[p - 1]:      # :1829
            lq_e = p - lq_min_length - 1
            if lq_s > lq_min_length:
                lq_s -= lq_min_length
            else:
                lq_s = 1
                br["clamp"] += 1
            if regions and pos[lq_s] >= regions[-1][0]:          # :1833-1834
                regions[-1] = (pos[lq_e], regions[-1][1])
                br["merge"] += 1
            else:
                regions.append((pos[lq_e], pos[lq_s]))           # (start, end)
                br["push"] += 1
            lq = 0
            lq_s = -1
        elif lq:
            br["held_near" if p - lq_e <= 2 * lq_min_length else "held_pos"] += 1
        if cov > min_cov:                                        # :1848-1852
            chars.append(INT_TO_BASE[base])
            br["upper"] += 1
        else:
            chars.append(INT_TO_BASE[base] | 0x20)
            br["lower"] += 1
        p += 1
    ok = p > 2 and total < p * 0.8 and np.float32(0) < np.float32(p) * (np.float32(1) - np.float32(ratio))
    return dict(mode=1, len=p, lqseq_total_length=total, ok=bool(ok), bases=[(a << 8) | c for a, c in zip(pos, chars)], regions=regions,
                br=br)


def restate_fast(steps, min_cov):
    """:1724-1777 -> dict: len, identity (numpy.float32), lq_total_len, seq (bytes), br, truncated, closed (slots the scan visited)."""
    u32 = lambda v: v & 0xffffffff
    lq = [dict(start=0, end=0, lqlen=0, total=0) for _ in range(10)]
    lq_i = 0
    out = bytearray()
    br = dict.fromkeys(F_BRANCHES, 0)
    truncated = False
    for t_pos, link, cov, base in steps.tolist():
        if base == 4:                                            # :1729
            continue
        s = lq[lq_i]
        if cov > min_cov:                                        # :1730-1734
            out.append(INT_TO_BASE[base])
            if s["end"] >= s["start"] + 50 or not lq_i:
                br["close_len" if lq_i else "close_slot0"] += 1
                lq_i += 1
                if lq_i >= 10:
                    br["truncate"] += 1
                    truncated = True
                    break
            else:
                s["end"] = 0
                br["empty"] += 1
        else:                                                    # :1735-1744
            out.append(INT_TO_BASE[base] | 0x20)
            if not s["end"]:
                s["start"] = len(out) - 1
                s["lqlen"] = 0
                br["lower_index0" if len(out) == 1 else "lower_open"] += 1
            else:
                br["lower_extend"] += 1
            s["end"] = len(out) - 1
            s["total"] += 1
            s["lqlen"] += 1
    lq_m, hq_m = 0, lq[0]["start"]                               # :1756-1771
    l = hq_m
    lq_total_len = u32(lq[0]["total"] - lq[0]["lqlen"])
    i = 1
    while i < 10 and lq[i]["end"]:
        if u32(lq[i]["start"] - lq[i - 1]["end"]) > u32(l):
            lq_m, hq_m = lq[i - 1]["end"] + 1, lq[i]["start"]
            lq_total_len = u32(lq[i]["total"] - lq[i]["lqlen"])
            l = hq_m - lq_m
            br["scan_take"] += 1
        else:
            br["scan_skip"] += 1
        i += 1
    if i == 1:
        br["no_closed"] += 1
    if i < 10:
        if u32(len(out) - lq[i - 1]["end"]) > u32(l):
            lq_m, hq_m = lq[i - 1]["end"] + 1, len(out)
            lq_total_len = lq[i]["total"]
            br["tail_take"] += 1
        else:
            br["tail_skip"] += 1
    ln = u32(hq_m - lq_m)                                        # :1773-1776
    with np.errstate(all="ignore"):
        identity = np.float32(1) - np.float32(lq_total_len) / np.float32(ln)
    return dict(mode=2, len=ln, identity=identity, lq_total_len=lq_total_len, ok=True, seq=bytes(out[lq_m:hq_m][::-1]), br=br,
                truncated=truncated, closed=i - 1, out_len=len(out))


def restate(w):
    steps, min_cov, lq_max_len, ratio, mode, seed = w
    return restate_kmer(steps, seed, min_cov, ratio) if mode == 1 else restate_fast(steps, min_cov)


def as_record(d):
    """A result of restate() or api.cns_walk_batch() as one comparable list."""
    if d["mode"] == 2:
        idn = np.float32(d["identity"])
        return [2, int(d["len"]), "nan" if np.isnan(idn) else int(idn.view(np.uint32)), int(d["lq_total_len"]), bool(d["ok"]), bytes(d["seq"]).decode()]
    return [1, int(d["len"]), int(d["lqseq_total_length"]), bool(d["ok"]), [int(x) for x in d["bases"]], [[int(a), int(b)] for a, b in d["regions"]]]


# ---- building walks -------------------------------------------------------------------------------------------------------------
TOP = 5000


def seed_for(top=TOP):
    """The seed whose code at position t is t % 4."""
    return (b"ATGC" * (top // 4 + 2))[:top + 1]


class Walk:
    """Items appended origin first; positions descend by one per item unless `ins` (an insertion column keeps the position).  A
    good item carries the seed's base (t % 4) and qv 90 at coverage 100."""

    def __init__(self, top=TOP):
        self.rows = []
        self.pos = top

    def add(self, n=1, qv=90, cov=100, ins=False, gap=False, mism=False):
        for _ in range(n):
            if not ins:
                self.pos -= 1
            b = 4 if gap else (self.pos + (1 if mism else 0)) % 4
            self.rows.append((self.pos, qv * cov // 100, cov, b))
        return self

    def bad(self, n=1):
        return self.add(n, qv=50)

    def lower(self, n=1):                         # (-fast: coverage at min_cov)
        return self.add(n, cov=4)

    def hifi(self, min_cov=4, ratio=0.8):
        return (np.asarray(self.rows, dtype=np.int64).reshape(-1, 4), min_cov, 10000, ratio, 1, seed_for())

    def fast(self, min_cov=4):
        return (np.asarray(self.rows, dtype=np.int64).reshape(-1, 4), min_cov, 10000, 0.8, 2, None)


LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)


def directed_hifi():
    c = []
    for n in LENGTHS:
        w = Walk()
        if n >= 63:
            w.add(5).bad(2).add(n - 7)
        else:
            w.add(n)
        c.append(("n=%d" % n, w.hifi()))
    c.append(("all-gap", Walk().add(70, gap=True).hifi()))
    # gap items on both sides of the chunk edges 63 | 64 and 127 | 128; a window whose emission lies behind the first edge
    w = Walk().add(58).bad(2).add(2).add(4, gap=True).add(60).add(4, gap=True).bad(1).add(20)
    c.append(("gaps-at-chunk-edges", w.hifi()))
    for k in (4, 5):                               # the walk ends k items behind the bad one: p - lq_e == k at the last item
        c.append(("tail-%d" % k, Walk().add(10).bad(1).add(k).hifi()))
    for b in (1, 2, 3):                            # lq_s <= 2: the clamp to 1 (3: lq_s - 2 = 1 without it)
        c.append(("bad-at-%d" % b, Walk().add(b).bad(1).add(10).hifi()))
    # the first window's start is pos[p1 - 3], a run of insertion columns carries that position on; the second bad item lies two
    # behind an index of that run (merge) or three (miss by one position)
    c.append(("merge", Walk().add(10).bad(1).add(2).add(8, ins=True).add(1).bad(1).add(8).hifi()))
    c.append(("merge-miss", Walk().add(10).bad(1).add(2).add(8, ins=True).add(2).bad(1).add(8).hifi()))
    c.append(("cov4-inside", Walk().add(10).bad(2).add(2).add(1, cov=3).add(10).hifi()))
    c.append(("cov4-idle", Walk().add(10).add(3, cov=3).add(10).hifi()))
    c.append(("insertions-at-emission", Walk().add(10).bad(1).add(3).add(4, ins=True).add(6).hifi()))
    c.append(("open-across-three-chunks", Walk().add(10).bad(1).add(2).add(150, ins=True).add(10).hifi()))
    c.append(("seed-differs", Walk().add(10).add(1, mism=True).add(10).hifi()))
    c.append(("bad-run-extends", Walk().add(10).bad(3).add(2).bad(1).add(10).hifi()))
    c.append(("ratio-below", Walk().bad(7).add(3).hifi()))
    c.append(("ratio-at", Walk().bad(8).add(2).hifi()))
    for lane in (0, 63):
        c.append(("idle-3-chunks-lane-%d" % lane, Walk().add(256 if lane == 0 else 255).bad(1).add(20).hifi()))
    w = Walk().add(6, cov=4).add(6, cov=5).add(6, cov=4)
    c.append(("cov-at-min-cov", w.hifi()))
    return c


def _runs(n_runs, first_lower=False, tail=7):
    w = Walk()
    if first_lower:
        w.lower(51)
        n_runs -= 1
    w.add(3)
    for _ in range(n_runs):
        w.lower(51).add(3)
    return w.add(tail)


def directed_fast():
    c = []
    for n in LENGTHS:
        w = Walk()
        if n >= 63:
            w.add(5).lower(51).add(n - 56)
        else:
            w.add(n)
        c.append(("n=%d" % n, w.fast()))
    c.append(("all-gap", Walk().add(70, gap=True).fast()))
    w = Walk().add(58).lower(4).add(1).add(4, gap=True).add(58).lower(2).add(4, gap=True).lower(3).add(20)
    c.append(("gaps-at-chunk-edges", w.fast()))
    c.append(("no-lower", Walk().add(40).fast()))
    c.append(("all-lower", Walk().lower(40).fast()))
    c.append(("lower-at-0", Walk().lower(1).add(20).fast()))
    c.append(("lower-run-from-0", Walk().lower(3).add(20).fast()))
    c.append(("lower-0-alone-at-chunk-end", Walk().lower(1).add(63, gap=True).lower(2).add(20).fast()))
    for k in (50, 51):
        c.append(("run-%d" % k, Walk().add(5).lower(k).add(5).fast()))
    c.append(("run-over-chunk-edge", Walk().add(40).lower(60).add(10).fast()))
    c.append(("run-ends-on-lane-63", Walk().add(4).lower(60).add(10).fast()))
    c.append(("run-starts-on-lane-0", Walk().add(64).lower(60).add(10).fast()))
    for k in (8, 9, 10):
        c.append(("closing-runs-%d" % k, _runs(k).fast()))
        c.append(("closing-runs-%d-first-lower" % k, _runs(k, first_lower=True).fast()))
    c.append(("ends-inside-run", Walk().add(10).lower(20).fast()))
    c.append(("ends-inside-long-run", Walk().add(10).lower(51).add(2).lower(60).fast()))
    c.append(("tail-taken", Walk().add(1).lower(51).add(100).fast()))
    c.append(("tail-not-taken", Walk().add(100).lower(51).add(3).fast()))
    c.append(("short-runs-leave-their-count", Walk().add(3).lower(5).add(3).lower(7).add(30).fast()))
    c.append(("cov-at-min-cov", Walk().add(6, cov=4).add(6, cov=5).add(6, cov=4).fast()))
    return c


def directed_cases():
    return [("hifi/" + k, w) for k, w in directed_hifi()] + [("fast/" + k, w) for k, w in directed_fast()]


def check_directed():
    """Asserts, from the restatements alone, that every directed case reaches the shape it is named for."""
    cases = dict(directed_cases())
    r = {k: restate(w) for k, w in cases.items()}
    h = lambda k: r["hifi/" + k]
    f = lambda k: r["fast/" + k]
    for n in LENGTHS:
        assert cases["hifi/n=%d" % n][0].shape[0] == n and h("n=%d" % n)["len"] == n
        assert cases["fast/n=%d" % n][0].shape[0] == n and f("n=%d" % n)["out_len"] == n
        if n >= 63:
            assert h("n=%d" % n)["br"]["push"] == 1 and f("n=%d" % n)["br"]["close_len"] == 1
    assert h("all-gap")["len"] == 0 and not h("all-gap")["ok"] and f("all-gap")["len"] == 0
    for k in ("hifi/gaps-at-chunk-edges", "fast/gaps-at-chunk-edges"):
        g = cases[k][0]
        assert g[63, 3] == 4 and g[64, 3] == 4 and g[127, 3] == 4 and g[128, 3] == 4 and g[61, 3] != 4 and g[67, 3] != 4, k
    assert h("gaps-at-chunk-edges")["br"]["push"] == 2 and f("gaps-at-chunk-edges")["br"]["empty"] >= 2
    assert h("tail-4")["br"]["push"] == 0 and h("tail-4")["br"]["held_near"] == 4 and h("tail-5")["br"]["push"] == 1
    assert h("bad-at-1")["br"]["clamp"] == 1 and h("bad-at-2")["br"]["clamp"] == 1 and h("bad-at-3")["br"]["clamp"] == 0
    assert all(h("bad-at-%d" % b)["regions"][0][1] == cases["hifi/bad-at-%d" % b][0][1, 0] for b in (1, 2, 3))     # end = pos[1]
    m, mm = h("merge"), h("merge-miss")
    assert m["br"]["push"] == 1 and m["br"]["merge"] == 1 and len(m["regions"]) == 1
    assert mm["br"]["push"] == 2 and mm["br"]["merge"] == 0 and mm["regions"][1][1] == mm["regions"][0][0] - 1
    assert h("cov4-inside")["br"] == dict(h("cov4-inside")["br"], cov4_open=1, push=0, merge=0) and h("cov4-inside")["lqseq_total_length"] == 3
    assert h("cov4-idle")["br"]["cov4"] == 3 and h("cov4-idle")["regions"] == []
    e = h("insertions-at-emission")
    assert e["br"]["held_pos"] == 3 and e["br"]["push"] == 1          # p - lq_e is 5, 6, 7 on insertion columns, emitted at 8
    o = h("open-across-three-chunks")
    assert o["br"]["held_pos"] > 128 and o["br"]["push"] == 1
    assert h("seed-differs")["br"]["bad_open"] == 1 and h("seed-differs")["br"]["push"] == 1 and h("seed-differs")["lqseq_total_length"] == 1
    assert h("bad-run-extends")["br"]["bad_extend"] == 3 and h("bad-run-extends")["br"]["push"] == 1
    assert h("ratio-below")["ok"] and not h("ratio-at")["ok"] and h("ratio-at")["len"] == 10 and h("ratio-at")["lqseq_total_length"] == 8
    for lane in (0, 63):
        k = "idle-3-chunks-lane-%d" % lane
        first_bad = int(np.nonzero(cases["hifi/" + k][0][:, 1] < 80)[0][0])
        assert first_bad % 64 == lane and first_bad // 64 >= 3 and h(k)["br"]["push"] == 1
    assert [chr(b & 0xff).islower() for b in h("cov-at-min-cov")["bases"]] == [True] * 6 + [False] * 6 + [True] * 6
    assert f("cov-at-min-cov")["len"] == 6 and f("cov-at-min-cov")["seq"].isupper() and f("cov-at-min-cov")["lq_total_len"] == 0
    # -fast
    n = f("no-lower")
    assert n["len"] == 39 and n["br"]["no_closed"] == 1 and n["br"]["tail_take"] == 1 and n["lq_total_len"] == 0      # one character dropped
    assert f("all-lower")["br"]["lower_index0"] == 1 and f("all-lower")["br"]["close_slot0"] == 0
    assert f("lower-at-0")["br"]["lower_index0"] == 1 and f("lower-at-0")["br"]["lower_open"] == 0
    assert f("lower-run-from-0")["br"] == dict(f("lower-run-from-0")["br"], lower_index0=1, lower_open=1, lower_extend=1)
    assert f("lower-0-alone-at-chunk-end")["br"] == dict(f("lower-0-alone-at-chunk-end")["br"], lower_index0=1, lower_open=1, lower_extend=1)
    assert f("run-50")["br"]["close_len"] == 0 and f("run-50")["br"]["empty"] >= 1 and f("run-51")["br"]["close_len"] == 1
    for k in ("run-over-chunk-edge", "run-ends-on-lane-63", "run-starts-on-lane-0"):
        assert f(k)["br"]["close_len"] == 1 and f(k)["closed"] == 1, k
    assert not f("closing-runs-8")["truncated"] and f("closing-runs-8")["closed"] == 8
    assert f("closing-runs-9")["truncated"] and f("closing-runs-10")["truncated"] and f("closing-runs-9")["closed"] == 9
    assert f("closing-runs-10")["out_len"] == f("closing-runs-9")["out_len"] < cases["fast/closing-runs-10"][0].shape[0] - 50
    assert not f("closing-runs-9-first-lower")["truncated"] and f("closing-runs-10-first-lower")["truncated"]
    assert f("ends-inside-run")["closed"] == 1 and f("ends-inside-run")["br"]["close_len"] == 0 and f("ends-inside-long-run")["closed"] == 2
    assert f("tail-taken")["br"]["tail_take"] == 1 and f("tail-not-taken")["br"]["tail_skip"] == 1 and f("tail-not-taken")["len"] == 99
    s = f("short-runs-leave-their-count")
    assert s["br"]["empty"] >= 2 and s["lq_total_len"] == 12 and s["br"]["tail_take"] == 1
    return cases


# ---- fuzz -----------------------------------------------------------------------------------------------------------------------
def _from_segments(rng, kinds, lens, total, top):
    kind = np.repeat(kinds, lens)[:total]
    return kind, top - np.cumsum(kind != 4)          # (kind 4: an insertion column keeps the position)


def fuzz_hifi(n, max_items, seed=2121, exact=False):
    """Segments of item kinds -- 0 good (1..40 items), 1 low qv, 2 a base that is not the seed's, 3 cov < 4, 4 good insertion columns,
    5 gaps -- and, a sixth of the segments, the pattern that merges two windows: a bad item, two good ones, six to ten insertion
    columns, one good item, a bad one, six good ones.  Coverage 4..60 where not low; a seed with an N every 97 bases and lower-case
    letters; min_cov 0..7."""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        total = max_items if exact else int(rng.integers(1, max_items + 1))
        top = 3 * max_items + 10
        k = total // 4 + 2
        kd = rng.choice(7, k, p=[0.38, 0.12, 0.08, 0.05, 0.1, 0.1, 0.17])
        kinds, lens = [], []
        for a, ln in zip(kd.tolist(), rng.integers(1, 41, k).tolist()):
            if a == 6:
                kinds += [1, 0, 4, 0, 1, 0]
                lens += [1, 2, 6 + ln % 5, 1, 1, 6]
            else:
                kinds.append(a)
                lens.append(ln if a in (0, 4) else 1 + ln % 3)
        kind, pos = _from_segments(rng, np.asarray(kinds), np.asarray(lens), total, top)
        m = kind.shape[0]
        cov = np.where(kind == 3, rng.integers(1, 4, m), rng.integers(4, 61, m))
        need = (80 * cov + 99) // 100                 # the smallest link with 100 * link / cov >= 80
        link = np.where(kind == 1, (rng.random(m) * need).astype(np.int64), need + (rng.random(m) * (cov - need + 1)).astype(np.int64))
        base = np.where(kind == 5, 4, np.where(kind == 2, (pos + 1 + rng.integers(0, 3, m)) % 4, pos % 4))
        sd = bytearray(seed_for(top))
        for t in range(it % 97, top + 1, 97):
            sd[t] = ord("N")
        for t in range(it % 13, top + 1, 13):
            sd[t] = sd[t] | 0x20 if sd[t] != ord("N") else sd[t]
        out.append((np.stack([pos, link, cov, base], axis=1).astype(np.int64), int(rng.integers(0, 8)), 10000, 0.8, 1, bytes(sd)))
    return out


def fuzz_fast(n, max_items, seed=2222, exact=False):
    """Runs of upper-case items (1..80), lower-case runs (a third of the walks: 50..70 items mostly, so that slots close and the
    table fills; a third: below 50, so that none closes; the rest mixed) and gaps; min_cov 1..7."""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        total = max_items if exact else int(rng.integers(1, max_items + 1))
        style = (it // 3 + it) % 3                                    # (every third walk of the set still meets all three)
        k = total // 3 + 2
        kinds = rng.choice(3, k, p=[0.45, 0.45, 0.1])                   # 0 upper, 1 lower, 2 gap
        if style == 0:
            kinds = np.arange(k) % 2                                    # strictly alternating: every lower-case run closes its slot
        up = rng.integers(1, 11 if style == 0 else 81, k)
        lo = rng.integers(50, 57, k) if style == 0 else rng.integers(1, 50, k) if style == 1 else rng.integers(30, 71, k)
        lens = np.where(kinds == 0, up, np.where(kinds == 1, lo, rng.integers(1, 6, k)))
        kind = np.repeat(kinds, lens)[:total]
        m = kind.shape[0]
        min_cov = int(rng.integers(1, 8))
        cov = np.where(kind == 1, rng.integers(1, min_cov + 1, m), rng.integers(min_cov + 1, 61, m))
        pos = 3 * max_items - np.cumsum(kind != 2)
        base = np.where(kind == 2, 4, rng.integers(0, 6, m))
        base[base == 4] = np.where(kind[base == 4] == 2, 4, 5)
        link = (rng.random(m) * (cov + 1)).astype(np.int64)
        out.append((np.stack([pos, link, cov, base], axis=1).astype(np.int64), min_cov, 10000, 0.8, 2, None))
    return out


def fuzz_walks(mode, n, max_items, **kw):
    return fuzz_hifi(n, max_items, **kw) if mode == 1 else fuzz_fast(n, max_items, **kw)


def long_walk(mode, n=100000):
    return fuzz_walks(mode, 1, n, seed=5 + mode, exact=True)[0]


def branch_totals(walks):
    tot = dict.fromkeys(K_BRANCHES + F_BRANCHES, 0)
    extra = dict(truncated=0, no_closed=0, merged=0)
    for w in walks:
        r = restate(w)
        for k, v in r["br"].items():
            tot[k] += v
        if w[4] == 2:
            extra["truncated"] += bool(r["truncated"])
            extra["no_closed"] += r["closed"] == 0
        else:
            extra["merged"] += r["br"]["merge"] > 0
    return tot, extra


def to_jobs(api, walks):
    return [(api.walk_steps(s[:, 0], s[:, 1], s[:, 2], s[:, 3]), mc, ml, ratio, mode, seed) for s, mc, ml, ratio, mode, seed in walks]


def walk_set(mode, n_fuzz, max_items, n_long=0):
    walks = [w for k, w in directed_cases() if w[4] == mode] + fuzz_walks(mode, n_fuzz, max_items)
    if n_long:
        walks.append(long_walk(mode, n_long))
    return walks


# ---- the engine's fixtures ------------------------------------------------------------------------------------------------------
def group_kind(key):
    """A group key of util.edge_groups -> 'fast', 'hifi' or 'raw': the loop its piles take behind the walk."""
    return "fast" if key[5] else "hifi" if key[6] == 3 else "raw"


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run --------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, cns_util, cns_modes_util as cm
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
if what == "batch":             # a mode's directed + fuzz walks: device, host flag and the restatement, in calls of `call` walks
    mode, n_fuzz, max_items = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    calls = [int(x) for x in sys.argv[6].split(",")]
    walks = cm.walk_set(mode, n_fuzz, max_items)
    exp = [cm.as_record(cm.restate(w)) for w in walks]
    jobs = cm.to_jobs(api, walks)
    out = dict(n=len(walks), regions=sum(len(e[5]) for e in exp) if mode == 1 else 0, bad_dev={})
    host = [cm.as_record(r) for r in api.cns_walk_batch(jobs, host=True)]
    out["bad_host"] = [i for i in range(len(walks)) if host[i] != exp[i]][:20]
    api.reset_stats()
    for call in calls:
        call = call or len(jobs)
        dev = {}
        for a in range(0, len(jobs), call):
            for k, r in enumerate(api.cns_walk_batch(jobs[a:a + call])):
                dev[a + k] = cm.as_record(r)
        out["bad_dev"][str(call)] = [i for i in dev if dev[i] != exp[i]][:20]
    out["stats"], out["mode_stats"] = api.stats(), api.cns_mode_stats()
    print(json.dumps(out))
elif what == "gpu":             # a mode's big set: all walks against the host routine, a part against the restatement; shuffled; singly
    mode, n_fuzz, max_items, n_long = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
    walks = cm.walk_set(mode, n_fuzz, max_items, n_long)
    n_dir = len(walks) - n_fuzz - 1
    jobs = cm.to_jobs(api, walks)
    host = [cm.as_record(r) for r in api.cns_walk_batch(jobs, host=True)]
    api.reset_stats()
    dev = []
    for a in range(0, len(jobs), 1000):
        dev += [cm.as_record(r) for r in api.cns_walk_batch(jobs[a:a + 1000])]
    st, ms = api.stats(), api.cns_mode_stats()
    out = dict(n=len(walks), n_dir=n_dir, longest=max(w[0].shape[0] for w in walks), longest_fuzz=max(w[0].shape[0] for w in walks[:-1]))
    out["bad_dev"] = [i for i in range(len(jobs)) if dev[i] != host[i]][:20]
    some = list(range(n_dir)) + list(range(n_dir, len(walks) - 1, 3)) + [len(walks) - 1]
    tot = dict.fromkeys(cm.K_BRANCHES + cm.F_BRANCHES, 0)
    bad = []
    for i in some:
        e = cm.restate(walks[i])
        for k, v in e["br"].items():
            tot[k] += v
        if cm.as_record(e) != dev[i]:
            bad.append(i)
    out["bad_restate"], out["n_restate"], out["br"] = bad[:20], len(some), tot
    out["sum_len"] = sum(h[1] for h in host) if mode == 1 else sum(len(h[5]) for h in host)
    out["regions"] = sum(len(h[5]) for h in host) if mode == 1 else 0
    out["stats"], out["mode_stats"] = st, ms
    perm = np.random.default_rng(5).permutation(len(jobs))
    got = []
    for a in range(0, len(jobs), 1000):
        got += [cm.as_record(r) for r in api.cns_walk_batch([jobs[i] for i in perm[a:a + 1000]])]
    out["bad_shuffled"] = [int(i) for k, i in enumerate(perm) if got[k] != host[int(i)]][:20]
    singly = list(range(n_dir)) + list(range(n_dir + 50, len(jobs), 97)) + [len(jobs) - 1]
    out["bad_singly"] = [i for i in singly if cm.as_record(api.cns_walk_batch([jobs[i]])[0]) != host[i]][:20]
    out["n_singly"] = len(singly)
    print(json.dumps(out))
elif what == "mode0":           # mode 0 of the new entry == the existing entry, on K20's directed cases (and mixed with the other modes)
    walks = [c[1] for c in cns_util.directed_cases()]
    old = [cns_util.as_record(r) for r in api.cns_windows_batch(cns_util.to_jobs(api, walks))]
    jobs = [(j[0], j[1], j[2], j[3], 0, None) for j in cns_util.to_jobs(api, walks)]
    other = cm.to_jobs(api, [w for k, w in cm.directed_cases()])
    mixed = []
    for i, j in enumerate(jobs):
        mixed += [j, other[i %% len(other)]]
    exp_other = [cm.as_record(cm.restate(w)) for k, w in cm.directed_cases()]
    res = {}
    for host in (False, True):
        new = [cns_util.as_record(r) for r in api.cns_walk_batch(jobs, host=host)]
        mx = api.cns_walk_batch(mixed, host=host)
        res[str(host)] = dict(same=new == old, mixed_raw=[cns_util.as_record(r) for r in mx[0::2]] == old,
                              mixed_other=all(cm.as_record(r) == exp_other[i %% len(other)] for i, r in enumerate(mx[1::2])))
    print(json.dumps(dict(n=len(walks), res=res)))
elif what == "piles":           # fixtures through correct_batch, grouped by the arguments a call takes once; counters per kind of group
    import rank_util
    piles = rank_util.pile_sets(sys.argv[3].split(","), None)
    rec, bad = {}, []
    names = ("cns_jobs", "cns_declined", "cns_launches", "cns_d2h_bytes", "walk_d2h_bytes")
    kinds = {k: dict(dict.fromkeys(names + tuple(api.cns_mode_stats()), 0), piles=0, after_main=0.0) for k in ("raw", "hifi", "fast")}
    for key, members in util.edge_groups(piles).items():
        b0, m0 = api.stats(), api.cns_mode_stats()
        for p, got in zip(members, util.edge_correct_group(api, key, members)):
            w = util.edge_wrong(p, got)
            if w:
                bad.append(w)
            rec[p["tag"]] = [int(got[0]), int(np.float32(got[1]).view(np.uint32)) if got[0] > 4 else 0, got[2].decode() if got[0] > 4 else ""]
        b1, m1 = api.stats(), api.cns_mode_stats()
        g = kinds[cm.group_kind(key)]
        for k in names:
            g[k] += b1[k] - b0[k]
        for k in m1:
            g[k] += m1[k] - m0[k]
        g["piles"] += len(members)
    print(json.dumps(dict(rec=rec, bad=bad, n=len(piles), kinds=kinds, stats=api.stats(), mode_stats=api.cns_mode_stats())))
elif what == "seed-n":          # one golden HiFi pile with a seed base replaced by N, in the ASCII form
    import rank_util
    piles = rank_util.pile_sets(["golden"], None)
    out = []
    for key, members in util.edge_groups(piles).items():
        if cm.group_kind(key) != "hifi":
            continue
        p = dict(members[0])
        s = bytearray(p["seqs"][0])
        s[len(s) // 2] = ord("N")
        p["seqs"] = [bytes(s)] + list(p["seqs"][1:])
        got = util.edge_correct_group(api, key, [p])[0]
        plain = util.edge_correct_group(api, key, [members[0]])[0]
        out.append([[int(g[0]), int(np.float32(g[1]).view(np.uint32)) if g[0] > 4 else 0, g[2].decode() if g[0] > 4 else ""] for g in (got, plain)])
        break
    print(json.dumps(dict(out=out, mode_stats=api.cns_mode_stats())))
elif what == "args":
    lib = api.load() if sys.argv[1] != "simt" else api._LIB
    ok = api.walk_steps([10, 9, 8], [50, 50, 50], [60, 60, 60], [0, 1, 2])
    out = {}
    def call(steps, mode, seed, seed_len=None, flags=0, n=None):
        st = np.ascontiguousarray(steps)
        job = (api.CnsWalkJob * 1)(api.CnsWalkJob(st.ctypes.data, st.size if n is None else n, 4, 10000, 0.8, mode,
                                                  (len(seed) if seed else 0) if seed_len is None else seed_len, seed))
        res = (api.CnsWalkResult * 1)()
        C.memset(res, 0x55, C.sizeof(res))
        bw, rw, sw = C.c_void_p(0x55), C.c_void_p(0x55), C.c_void_p(0x55)
        rc = lib.ndgpu_cns_walk_batch(job, 1, flags, res, C.byref(bw), C.byref(rw), C.byref(sw))
        untouched = bytes(res) == b"\x55" * C.sizeof(res) and bw.value == 0x55 and rw.value == 0x55 and sw.value == 0x55
        return [rc, untouched]
    seed = b"ACGTACGTACGT"
    for flags in (0, 1):
        out["mode3/%%d" %% flags] = call(ok, 3, seed, flags=flags)
        out["mode-neg/%%d" %% flags] = call(ok, -1, seed, flags=flags)
        out["hifi-null-seed/%%d" %% flags] = call(ok, 1, None, flags=flags)
        out["hifi-short-seed/%%d" %% flags] = call(ok, 1, seed, seed_len=10, flags=flags)       # t_pos 10 >= seed_len 10
        out["hifi-seed-just-fits/%%d" %% flags] = call(ok, 1, seed, seed_len=11, flags=flags)
        gap = ok.copy(); gap["base"][0] = 4
        out["hifi-gap-outside-seed/%%d" %% flags] = call(gap, 1, seed, seed_len=10, flags=flags)   # a gap step's t_pos is not looked at
        for mode in (0, 1, 2):
            bad = ok.copy(); bad["cov"][1] = 0
            out["cov0-%%d/%%d" %% (mode, flags)] = call(bad, mode, seed, flags=flags)
            bad = ok.copy(); bad["base"][2] = 6
            out["base6-%%d/%%d" %% (mode, flags)] = call(bad, mode, seed, flags=flags)
            out["ok-%%d/%%d" %% (mode, flags)] = call(ok, mode, seed, flags=flags)
            out["empty-job-%%d/%%d" %% (mode, flags)] = call(ok, mode, seed, flags=flags, n=0)
        out["fast-null-seed/%%d" %% flags] = call(ok, 2, None, flags=flags)
        out["n0/%%d" %% flags] = lib.ndgpu_cns_walk_batch(None, 0, flags, None, None, None, None)
        out["n-neg/%%d" %% flags] = lib.ndgpu_cns_walk_batch(None, -1, flags, None, None, None, None)
    out["py-empty"] = api.cns_walk_batch([]) == [] and api.cns_walk_batch([], host=True) == []
    print(json.dumps(out))
"""


def child(lib, what, *args, timeout=1500, **env):
    # no switch of the caller's reaches the child
    e = {k: v for k, v in os.environ.items() if not k.startswith(("NDGPU_CNS", "NDGPU_RANK", "NDGPU_POA", "NDGPU_TRACE", "NDGPU_EXTRACT"))}
    e.update(env)
    if lib == "simt":
        e.setdefault("NDGPU_CONTEXTS", "1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE, os.path.join(HERE, "simt")), lib, what, *[str(a) for a in args]],
                         env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    r["trace"] = [ln for ln in out.stderr.splitlines() if ln.startswith("[ndgpu trace] cns_walk")]
    return r
