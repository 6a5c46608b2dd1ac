"""Shared by tests/test_simt_cns_windows.py and tests/test_zz_gpu_cns_windows.py: the loop of generate_cns_from_best_score restated in
Python from the reference's lines (lib/nextcorrect.c:1907-1982, the verdict :1986-1987), not from the library, with a count of how
often each branch was taken; directed walks, each the smallest shape at which K20 (cns_windows_kernel, msa_kernels.hip: 64 items a
chunk, a wave-uniform window automaton that skips from its idle state) can go wrong, and check_directed(), which asserts from the
restatement that each reaches its shape; a seeded two-state fuzz generator; and the child processes that run the batched entry
(api.cns_windows_batch) and the engine (api.correct_batch) under the switches that are read once per process.

A walk here is (steps, min_cov, lq_max_len, ratio) with steps an int array [n, 4]: t_pos, link, cov, base (A0 T1 G2 C3, 4 a gap, 5 N)."""
import json
import os
import subprocess
import sys

import numpy as np

import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

INT_TO_BASE = b"ATGC-N"
BRANCHES = ("reset", "join", "emit", "refuse_short", "refuse_long", "clamp", "shared_iter", "shared_p4", "third")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate(steps, min_cov, lq_max_len, ratio=0.8):
    """-> dict: bases (pos << 8 | char at index p, before reverse_consensus_base), regions [(start, end)], the five counters, ok, and
    br: how often each branch of BRANCHES was taken."""
    lq_min_length = 8
    p, lable = 0, 1
    hq = qv = lq_l = lq = 0
    lq_s = lq_e = -1
    lqseq_total_length = uncorrected_len = lstrip = rstrip = 0
    pos, chars, regions = [], [], []
    br = dict.fromkeys(BRANCHES, 0)
    for t_pos, link, cov, base in steps.tolist():
        if base == 4:                                            # :1908
            continue
        pos.append(t_pos)                                        # :1914
        pqv = 100 * link // cov                                  # :1916 (both non-negative: C's division)
        if pqv > 40:                                             # :1918-1923
            hq += 1
        else:
            hq = 0
            lqseq_total_length += 1
        if hq > lq_min_length // 2 and lq_e - lq_s < lq_min_length // 2:      # :1925-1928
            if qv or lq_l or lq or lq_s != -1:
                br["reset"] += 1
            qv = lq_l = lq = 0
            lq_s = -1
        if (qv + pqv) // (lq_l + 1) < 40:                        # :1930-1935
            if lq_s == -1:
                lq_s = p
            lq_e = p
            lq = 1
            lq_l += 1
            qv += pqv
            br["join"] += 1
        elif lq and p - lq_e > 2 * lq_min_length and pos[p] != pos[p - 1]:      # :1936
            if lq_e - lq_s + 1 > lq_min_length and lq_e - lq_s + 1 < lq_max_len:   # :1937
                lq_e = p - lq_min_length - 1
                if lq_s > lq_min_length:
                    lq_s = lq_s - lq_min_length
                else:
                    lq_s = 1
                    br["clamp"] += 1
                end, start = pos[lq_s], pos[lq_e]
                if regions and end == regions[-1][0]:             # :1943-1947
                    while end == regions[-1][0] and lq_s < p - 4:
                        lq_s += 1
                        end = pos[lq_s]
                        br["shared_iter"] += 1
                    if end == regions[-1][0]:
                        br["shared_p4"] += 1
                regions.append((start, end))
                br["emit"] += 1
            elif lq_e - lq_s + 1 <= lq_min_length:
                br["refuse_short"] += 1
            else:
                br["refuse_long"] += 1
            qv = lq_l = lq = 0                                   # :1957-1958
            lq_s = -1
        elif lq and pos[p] != pos[p - 1]:                        # :1959-1961
            qv = lq_l = 0
            br["third"] += 1
        if cov > min_cov and pqv > 20:                           # :1963-1974
            chars.append(INT_TO_BASE[base])
            lable = 0
            lstrip = 0
        else:
            chars.append(INT_TO_BASE[base] | 0x20)
            uncorrected_len += 1
            lstrip += 1
            if lable:
                rstrip += 1
        p += 1
    u32 = lambda v: np.float32(int(v) & 0xffffffff)              # :1986-1987: unsigned ints, converted to float
    ok = p > 2 and lqseq_total_length < p * 0.8 and \
        u32(uncorrected_len - lstrip - rstrip) < u32(p - lstrip - rstrip) * (np.float32(1) - np.float32(ratio))
    return dict(len=p, uncorrected_len=uncorrected_len, lstrip=lstrip, rstrip=rstrip, lqseq_total_length=lqseq_total_length, ok=bool(ok),
                bases=[(a << 8) | c for a, c in zip(pos, chars)], regions=regions, br=br)


def as_record(d):
    """A result of restate() or api.cns_windows_batch() as one comparable list."""
    return [int(d["len"]), int(d["uncorrected_len"]), int(d["lstrip"]), int(d["rstrip"]), int(d["lqseq_total_length"]), bool(d["ok"]),
            [int(x) for x in d["bases"]], [[int(a), int(b)] for a, b in d["regions"]]]


# ---- building walks -------------------------------------------------------------------------------------------------------------
class Walk:
    """Items appended origin first; positions descend by one per item unless `ins` (an insertion column keeps the position)."""

    def __init__(self, top=100000):
        self.rows = []
        self.pos = top

    def add(self, n, pqv=90, cov=100, base=None, ins=False, gap=False, pos=None):
        for k in range(n):
            if not ins:
                self.pos -= 1
            b = 4 if gap else (len(self.rows) % 4 if base is None else base)
            self.rows.append((self.pos if pos is None else pos, pqv * cov // 100, cov, b))
        return self

    def done(self, min_cov=4, lq_max_len=10000, ratio=0.8):
        return (np.asarray(self.rows, dtype=np.int64).reshape(-1, 4), min_cov, lq_max_len, ratio)


def directed_cases():
    """[(name, walk)].  Lows of pqv 39 are used where a window's length must be exact: up to 50 of them a following item of pqv 90
    does not join ((39 k + 90) / (k + 1) >= 40), so the window is the k lows."""
    c = []
    for n in (0, 1, 2, 3, 63, 64, 65, 128, 129):
        w = Walk()
        if n >= 63:
            w.add(5).add(10, 39).add(n - 15)
        else:
            w.add(n, 30 if n == 2 else 90)
        c.append(("n=%d" % n, w.done()))
    c.append(("all-gap", Walk().add(70, gap=True).done()))
    # gaps on both sides of the chunk edge 63 | 64 and of 127 | 128: the item index and p part; a window across the first edge
    w = Walk().add(54).add(6, 39).add(7, gap=True).add(4, 39).add(56).add(4, gap=True).add(10, 39).add(40)
    c.append(("gaps-at-chunk-edges", w.done()))
    # a window opened in chunk 0 and emitted in chunk 2: every item behind it is an insertion column up to index 140
    c.append(("emit-two-chunks-later", Walk().add(40).add(10, 39).add(90, ins=True).add(30).done()))
    for k in (8, 9):
        c.append(("window-%d" % k, Walk().add(20).add(k, 39).add(30).done()))
    for k in (11, 12):
        c.append(("window-%d-of-max-12" % k, Walk().add(20).add(k, 39).add(30).done(lq_max_len=12)))
    for tail in (16, 17):
        c.append(("tail-%d" % tail, Walk().add(20).add(9, 39).add(tail).done()))
    c.append(("held-back", Walk().add(20).add(9, 39).add(16).add(5, ins=True).add(10).done()))
    # two windows that share a boundary: the first one's start is pos[p1 - 9]; the run of equal positions reaches from there to p1 - 1
    w = Walk().add(20).add(9, 39).add(8).add(9, ins=True).add(1).add(10, 39).add(30)
    c.append(("shared-boundary", w.done()))
    # ... and a run of that position (positions are the caller's: they need not descend) up to the second emission: the loop ends at p - 4
    w = Walk().add(20).add(9, 39).add(7).add(8, pos=777).add(1).add(8, pos=777).add(10, 39, pos=777).add(17, pos=777).add(10)
    c.append(("shared-boundary-p4", w.done()))
    c.append(("clamp", Walk().add(3).add(9, 39).add(30).done()))
    c.append(("reset-3", Walk().add(20).add(3, 39).add(30).done()))
    c.append(("third-then-join", Walk().add(20).add(5, 39).add(1).add(4, 10).add(30).done()))
    for lane in (0, 63):
        c.append(("idle-3-chunks-lane-%d" % lane, Walk().add(256 if lane == 0 else 255).add(10, 39).add(40).done()))
    c.append(("all-lower", Walk().add(40, cov=3).done()))
    w = Walk().add(6, 75, cov=4).add(6, 80, cov=5).add(6, 75, cov=4)
    c.append(("cov-at-min-cov", w.done()))
    w = Walk().add(6)
    for q in (20, 21, 39, 40, 41, 41, 40, 39, 21, 20):
        w.add(1, q)
    c.append(("pqv-thresholds", w.add(30).done()))
    return c


def check_directed(cases=None):
    """Asserts, from the restatement alone, that every directed case reaches the shape it is named for."""
    cases = dict(cases or directed_cases())
    r = {k: restate(*v) for k, v in cases.items()}
    for n in (0, 1, 2, 3, 63, 64, 65, 128, 129):
        assert cases["n=%d" % n][0].shape[0] == n and r["n=%d" % n]["len"] == n
    for n in (63, 64, 65, 128, 129):
        assert r["n=%d" % n]["br"]["emit"] == 1
    assert r["all-gap"]["len"] == 0 and not r["all-gap"]["ok"]
    g = cases["gaps-at-chunk-edges"][0]
    assert g[63, 3] == 4 and g[64, 3] == 4 and g[127, 3] == 4 and g[128, 3] == 4 and g[59, 3] != 4 and g[67, 3] != 4 and r["gaps-at-chunk-edges"]["br"]["emit"] == 2
    e = r["emit-two-chunks-later"]
    assert e["br"]["emit"] == 1 and e["br"]["third"] == 0 and e["regions"][0][0] == cases["emit-two-chunks-later"][0][131, 0]   # lq_e = p - 9, p = 140
    assert r["window-8"]["br"] == dict(r["window-8"]["br"], emit=0, refuse_short=1) and r["window-9"]["br"]["emit"] == 1
    assert r["window-11-of-max-12"]["br"]["emit"] == 1 and r["window-12-of-max-12"]["br"] == dict(r["window-12-of-max-12"]["br"], emit=0, refuse_long=1)
    assert r["tail-16"]["br"]["emit"] == 0 and r["tail-17"]["br"]["emit"] == 1 and r["tail-16"]["len"] == 45
    assert r["held-back"]["br"]["emit"] == 1 and r["held-back"]["regions"][0][0] == cases["held-back"][0][20 + 9 + 16 + 5 - 9, 0]
    s = r["shared-boundary"]["br"]
    assert s["emit"] == 2 and s["shared_iter"] > 0 and s["shared_p4"] == 0 and r["shared-boundary"]["regions"][1][1] != r["shared-boundary"]["regions"][0][0]
    s = r["shared-boundary-p4"]["br"]
    assert s["emit"] == 2 and s["shared_iter"] > 0 and s["shared_p4"] == 1 and r["shared-boundary-p4"]["regions"][1][1] == r["shared-boundary-p4"]["regions"][0][0]
    assert r["clamp"]["br"]["clamp"] == 1 and r["clamp"]["br"]["emit"] == 1
    assert r["reset-3"]["br"] == dict(r["reset-3"]["br"], reset=1, join=3, emit=0, refuse_short=0)
    t = r["third-then-join"]["br"]
    assert t["third"] >= 1 and t["join"] == 11 and t["emit"] == 1     # 5 + 4 lows and two items of 90 under the new mean
    for lane in (0, 63):
        k = "idle-3-chunks-lane-%d" % lane
        first_low = int(np.nonzero(cases[k][0][:, 1] < 40)[0][0])
        assert first_low % 64 == lane and first_low // 64 >= 3 and r[k]["br"]["emit"] == 1
    a = r["all-lower"]
    assert a["lstrip"] == a["rstrip"] == a["len"] == 40 and a["uncorrected_len"] == 40 and not a["ok"]
    v = r["cov-at-min-cov"]
    assert [chr(b & 0xff).islower() for b in v["bases"]] == [True] * 6 + [False] * 6 + [True] * 6 and v["rstrip"] == v["lstrip"] == 6
    q = r["pqv-thresholds"]
    assert [chr(b & 0xff).islower() for b in q["bases"][6:16]] == [True, False, False, False, False, False, False, False, False, True]
    assert q["lqseq_total_length"] == 8 and q["br"]["join"] >= 4     # 41 alone is above DAG_MIN_QV; 39 and below join from the idle state
    return cases


# ---- fuzz -----------------------------------------------------------------------------------------------------------------------
def fuzz_walks(n, max_items, seed=2020, exact=False):
    """A two-state generator: high stretches of 1..60 items (link 50..100 % of the coverage) and low bursts of 1..40 (below 40 %); a
    tenth of the items gaps, a tenth insertion columns; coverage 1..60; lq_max_len 12..40 in a quarter of the walks.  Positions that
    descend end the shared-boundary loop at the boundary, never at p - 4, so every tenth walk has the caller's own positions, as the
    batched entry allows: one value, left for a single item 24 to 35 items behind each burst of 9 to 20 lows of pqv 30..39, no gaps.
    (Array operations per walk: the GPU tests draw millions of items.)"""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        total = max_items if exact else int(rng.integers(1, max_items + 1))
        few = it % 10 == 9
        if few:                 # runs in threes: high 9..19, low 9..20, high 24..35 whose last item leaves the position
            k = total // 42 + 1
            runs = np.stack([rng.integers(9, 20, k), rng.integers(9, 21, k), rng.integers(24, 36, k)], axis=1).reshape(-1)
            low_run = np.tile([False, True, False], k)
        else:
            k = total + 1
            first_low = bool(rng.integers(0, 2))
            low_run = (np.arange(k) % 2 == 0) == first_low
            runs = np.where(low_run, rng.integers(1, 41, k), rng.integers(1, 61, k))
        low = np.repeat(low_run, runs)[:total]
        u = rng.random(total)
        cov = rng.integers(1, 61, total)
        lo = np.where(low, 0, (cov + 1) // 2)
        hi = np.where(low, np.maximum(1, (40 * cov + 99) // 100), cov + 1)       # exclusive
        link = lo + (rng.random(total) * (hi - lo)).astype(np.int64)
        base = rng.integers(0, 6, total)
        if few:
            ends = np.cumsum(runs)[2::3] - 1
            pos = np.full(total, 1000)
            pos[ends[ends < total]] = 1001
            cov = np.where(low, 100, cov)
            link = np.where(low, rng.integers(30, 40, total), link)
            base[base == 4] = 5
        else:
            pos = 3 * max_items - np.cumsum(u >= 0.1)     # (an insertion column keeps the position)
            base[(u >= 0.1) & (u < 0.2)] = 4
        out.append((np.stack([pos, link, cov, base], axis=1).astype(np.int64), int(rng.integers(0, 8)),
                    int(rng.integers(12, 41)) if it % 4 == 0 else 10000, 0.8))
    return out


def branch_totals(walks):
    tot = dict.fromkeys(BRANCHES, 0)
    for w in walks:
        for k, v in restate(*w)["br"].items():
            tot[k] += v
    return tot


def long_walk(n=200000, seed=5):
    """One fuzz walk of exactly n items."""
    return fuzz_walks(1, n, seed, exact=True)[0]


def to_jobs(api, walks):
    return [(api.walk_steps(s[:, 0], s[:, 1], s[:, 2], s[:, 3]), mc, ml, ratio) for s, mc, ml, ratio in walks]


# ---- the engine's fixtures ------------------------------------------------------------------------------------------------------
def pile_sets(names):
    import rank_util
    return rank_util.pile_sets(names, None)


def is_raw(key):
    """A group key of util.edge_groups whose piles take K20: raw reads, not -fast."""
    return key[5] == 0 and key[6] != 3


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run --------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, cns_util
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
if what == "batch":             # directed + fuzz walks (+ the long one): device, host flag and the restatement, in calls of `call` walks
    n_fuzz, max_items, n_long = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    calls = [int(x) for x in sys.argv[6].split(",")]
    shuffle = len(sys.argv) > 7 and sys.argv[7] == "shuffle"
    walks = [c[1] for c in cns_util.directed_cases()] + cns_util.fuzz_walks(n_fuzz, max_items)
    if n_long:
        walks.append(cns_util.long_walk(n_long))
    if shuffle:
        order = np.random.default_rng(9).permutation(len(walks))
        walks = [walks[int(i)] for i in order]
    exp = [cns_util.as_record(cns_util.restate(*w)) for w in walks]
    jobs = cns_util.to_jobs(api, walks)
    out = dict(n=len(walks), longest=max(w[0].shape[0] for w in walks), regions=sum(len(e[7]) for e in exp), bad_dev={}, bad_host=[])
    host = [cns_util.as_record(r) for r in api.cns_windows_batch(jobs, host=True)]
    out["bad_host"] = [i for i in range(len(walks)) if host[i] != exp[i]][:20]
    api.reset_stats()
    for call in calls:
        call = call or len(jobs)
        ids = range(len(jobs)) if call > 1 or len(jobs) < 400 else range(0, len(jobs), 37)    # singly: every walk, or every 37th of a large set
        dev = {}
        for a in (range(0, len(jobs), call) if call > 1 else ids):
            for k, r in enumerate(api.cns_windows_batch(jobs[a:a + call])):
                dev[a + k] = cns_util.as_record(r)
        out["bad_dev"][str(call)] = [i for i in dev if dev[i] != exp[i]][:20]
    out["stats"] = api.stats()
    print(json.dumps(out))
elif what == "piles":           # fixtures through correct_batch, grouped by the arguments a call takes once; counters over the raw groups
    piles = cns_util.pile_sets(sys.argv[3].split(","))
    if len(sys.argv) > 4:
        piles = [p for p in piles if len(p["seqs"]) - 1 <= int(sys.argv[4])]
    rec, bad = {}, []
    raw = dict(cns_jobs=0, cns_declined=0, cns_launches=0, cns_d2h_bytes=0, walk_d2h_bytes=0, piles=0, expected=0)
    for key, members in util.edge_groups(piles).items():
        before = api.stats()
        for p, got in zip(members, util.edge_correct_group(api, key, members)):
            w = util.edge_wrong(p, got)
            if w:
                bad.append(w)
            rec[p["tag"]] = [int(got[0]), int(np.float32(got[1]).view(np.uint32)) if got[0] > 4 else 0, got[2].decode() if got[0] > 4 else ""]
        after = api.stats()
        if cns_util.is_raw(key):
            for k in ("cns_jobs", "cns_declined", "cns_launches", "cns_d2h_bytes", "walk_d2h_bytes"):
                raw[k] += after[k] - before[k]
            raw["piles"] += len(members)
            raw["expected"] += sum(1 for p in members if p["exp_len"] > 3)
    print(json.dumps(dict(rec=rec, bad=bad, n=len(piles), raw=raw, stats=api.stats())))
elif what == "args":
    lib = api.load() if sys.argv[1] != "simt" else api._LIB
    ok = api.walk_steps([10, 9, 8], [50, 50, 50], [60, 60, 60], [0, 1, 2])
    out = {}
    def call(steps, n=None, flags=0):
        st = np.ascontiguousarray(steps)
        job = (api.CnsJob * 1)(api.CnsJob(st.ctypes.data, st.size if n is None else n, 4, 10000, 0.8))
        res = (api.CnsResult * 1)()
        C.memset(res, 0x55, C.sizeof(res))
        bw, rw = C.c_void_p(0x55), C.c_void_p(0x55)
        rc = lib.ndgpu_cns_windows_batch(job, 1, flags, res, C.byref(bw), C.byref(rw))
        untouched = bytes(res) == b"\x55" * C.sizeof(res) and bw.value == 0x55 and rw.value == 0x55
        return [rc, untouched]
    for flags in (0, 1):
        bad = ok.copy(); bad["cov"][1] = 0
        out["cov0/%%d" %% flags] = call(bad, flags=flags)
        bad = ok.copy(); bad["base"][2] = 6
        out["base6/%%d" %% flags] = call(bad, flags=flags)
        bad = ok.copy(); bad["t_pos"][0] = (1 << 21) - 1
        out["tpos-high/%%d" %% flags] = call(bad, flags=flags)
        bad = ok.copy(); bad["t_pos"][0] = -1
        out["tpos-neg/%%d" %% flags] = call(bad, flags=flags)
        gap = ok.copy(); gap["base"][1] = 4; gap["cov"][1] = 0; gap["t_pos"][1] = -5     # a gap step is not looked at
        out["gap-any/%%d" %% flags] = call(gap, flags=flags)
        top = ok.copy(); top["t_pos"][0] = (1 << 21) - 2
        out["tpos-top/%%d" %% flags] = call(top, flags=flags)
        out["empty-job/%%d" %% flags] = call(ok, n=0, flags=flags)
        out["n0/%%d" %% flags] = lib.ndgpu_cns_windows_batch(None, 0, flags, None, None, None)
        out["n-neg/%%d" %% flags] = lib.ndgpu_cns_windows_batch(None, -1, flags, None, None, None)
    out["py-empty"] = api.cns_windows_batch([]) == [] and api.cns_windows_batch([], host=True) == []
    r = api.cns_windows_batch([(top, 4, 10000, 0.8)])[0]
    out["top-pos"] = int(r["bases"][0]) >> 8
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
    r["trace"] = [ln for ln in out.stderr.splitlines() if ln.startswith("[ndgpu trace] cns_windows")]
    return r
