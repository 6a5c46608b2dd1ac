"""Helpers of the batched-alignment tests (test_simt_align_batch.py, test_zz_gpu_align_batch.py): what ndgpu_align_batch must report
for a pair, worked out from the reference's answers alone -- tests/golden/align_pairs.npz (outputs of the compiled reference's align /
align_hq) and oracle/libndoracle.so's nd_oracle_align (held against the compiled reference by test_oracle.py).  The expected CIGAR and
counts are a numpy run-length encoding of those column kinds; nothing here comes from the library under test."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE_SO = os.path.join(ROOT, "oracle", "libndoracle.so")
FIELDS = ("status", "aln_len", "q_used", "t_used", "n_match", "n_ins", "n_del", "max_gap_run")
BAM_OP = np.array([7, 1, 2], dtype=np.uint32)    # OP_MATCH '=', OP_QONLY 'I', OP_TONLY 'D'


def rle(ops):
    """column kinds (0 match, 1 query only, 2 target only) -> (runs as len << 4 | BAM op, run lengths, run kinds)"""
    ops = np.asarray(ops, dtype=np.uint8)
    if ops.size == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    cut = np.flatnonzero(np.r_[True, ops[1:] != ops[:-1], True])
    lens, kinds = np.diff(cut), ops[cut[:-1]]
    return (lens.astype(np.uint32) << 4 | BAM_OP[kinds]).astype(np.uint32), lens, kinds


def expect(status, q_used, t_used, ops):
    """The result record of a pair the reference answered with (status, aln_q_len, aln_t_len, column kinds)."""
    if status == 0:
        return dict(status=0, aln_len=0, q_used=0, t_used=0, n_match=0, n_ins=0, n_del=0, max_gap_run=0, cigar=np.zeros(0, np.uint32))
    ops = np.asarray(ops, dtype=np.uint8)
    runs, lens, kinds = rle(ops)
    gaps = lens[kinds != 0]
    return dict(status=int(status), aln_len=int(ops.size), q_used=int(q_used), t_used=int(t_used), n_match=int((ops == 0).sum()),
                n_ins=int((ops == 1).sum()), n_del=int((ops == 2).sum()), max_gap_run=int(gaps.max()) if gaps.size else 0, cigar=runs)


def oracle():
    return C.CDLL(ORACLE_SO)


def oracle_expect(olib, q, t, hq):
    o, ts, qs, _ = util.oracle_align(olib, q, t, hq)
    return expect(o.status, o.q_used, o.t_used, util.strings_to_ops(ts, qs))


def golden_status(p):
    """align_pairs.npz records what align() left in its argument: nothing (aln_len 0), or aln_len 2 behind two long sequences (the
    > 250-gap abort), or an alignment."""
    if p["aln_len"] == 0:
        return 0
    return 2 if p["aln_len"] == 2 and max(p["q_used"], p["t_used"]) > 2 else 1


def golden_jobs(olib, max_total=None):
    """[(q, t, hq)], [expected] of the golden pairs with q_len + t_len <= max_total (None: all 71).  The fixture keeps the column
    kinds of the alignments only; the two columns an abort leaves are the oracle's, which must agree with what the fixture does keep."""
    jobs, exp = [], []
    for p in util.load_pairs():
        if max_total is not None and len(p["q"]) + len(p["t"]) > max_total:
            continue
        jobs.append((p["q"], p["t"], p["hq"]))
        st = golden_status(p)
        if st == 2:
            e = oracle_expect(olib, p["q"], p["t"], p["hq"])
            assert (e["status"], e["aln_len"], e["q_used"], e["t_used"]) == (2, 2, p["q_used"], p["t_used"]), (e, p["q_used"], p["t_used"])
        else:
            assert len(p["ops"]) == p["aln_len"]
            e = expect(st, p["q_used"], p["t_used"], p["ops"])
        exp.append(e)
    return jobs, exp


def max_window_starts(cigar, aln_len):
    """The most run starts in one of the 64-column windows the kernel takes the columns in (window k = columns [64k, 64k + 64))."""
    starts = np.cumsum(np.r_[0, cigar[:-1] >> 4]).astype(np.int64)
    return int(np.bincount(starts // 64, minlength=(aln_len + 63) // 64).max()) if cigar.size else 0


def _seq(rng, n):
    return util.ASC[rng.integers(0, 4, n)].tobytes()


def directed_jobs():
    """[(name, q, t, hq)] over ACGT from numpy.random.default_rng(7); check_directed() holds them to the shapes they are here for."""
    rng = np.random.default_rng(7)
    jobs = []
    for L in (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 192, 1000):
        s = _seq(rng, L)
        jobs.append(("same/%d" % L, s, s, 0))
    for L in (192, 1000):
        t = _seq(rng, L)
        for hq in (0, 1):
            jobs.append(("drop2/%d/hq%d" % (L, hq), t[::2], t, hq))
    t = _seq(rng, 300)
    q = bytes(b for i, b in enumerate(t) if i % 3 != 2)
    for hq in (0, 1):
        jobs.append(("drop3/300/hq%d" % hq, q, t, hq))
    # (the traceback places the deletions as early as the forward sweep allows, which eats into the equal columns in front of the first
    # block: of the first 60 targets of a generator of its own only a handful keep 129 of them -- the ninth is the first)
    rb = np.random.default_rng(7)
    t = [_seq(rb, 600) for _ in range(9)][-1]
    q = t[:170] + t[240:270] + t[470:]          # a 70-base and a 200-base block removed
    jobs.append(("blocks/qt", q, t, 0))
    jobs.append(("blocks/tq", t, q, 0))
    for L in (50, 500):
        jobs.append(("unrelated/%d" % L, _seq(rng, L), _seq(rng, L), 0))
    jobs.append(("unrelated/3000", _seq(rng, 3000), _seq(rng, 3000), 0))
    return jobs


def check_directed(olib):
    """The directed jobs with their expected records, after asserting from the ORACLE's answers that each reaches the shape it is
    named for (a changed generator cannot hide a case)."""
    jobs = directed_jobs()
    exp = {name: oracle_expect(olib, q, t, hq) for name, q, t, hq in jobs}
    lens = {name: (len(q), len(t)) for name, q, t, hq in jobs}
    assert exp["same/1"]["status"] == 0
    for L in (2, 3, 4, 63, 64, 65, 127, 128, 129, 192, 1000):
        e = exp["same/%d" % L]
        assert e["status"] == 1 and e["cigar"].tolist() == [L << 4 | 7], (L, e)
    for L, runs in ((192, 142), (1000, 757)):
        e = exp["drop2/%d/hq0" % L]
        assert e["status"] == 1 and e["aln_len"] == L and e["cigar"].size >= runs * 3 // 4, (L, e["status"], e["aln_len"], e["cigar"].size)
        assert max_window_starts(e["cigar"], e["aln_len"]) >= 48, max_window_starts(e["cigar"], e["aln_len"])
        assert exp["drop2/%d/hq1" % L]["status"] == 0          # mixed hq results in one call
    assert exp["drop2/192/hq0"]["aln_len"] % 64 == 0
    for hq in (0, 1):
        e = exp["drop3/300/hq%d" % hq]
        assert e["status"] == 1 and e["cigar"].size >= 150, (hq, e["status"], e["cigar"].size)
    for name in ("blocks/qt", "blocks/tq"):
        e = exp[name]
        lens_, kinds = e["cigar"] >> 4, e["cigar"] & 15
        eq = np.flatnonzero((kinds == 7) & (lens_ >= 129))
        assert e["status"] == 1 and eq.size >= 2 and eq[0] == 0 and eq[-1] == kinds.size - 1, (name, e["cigar"].tolist())
    assert (exp["blocks/qt"]["cigar"] & 15 == 2).any() and (exp["blocks/tq"]["cigar"] & 15 == 1).any()      # D runs and I runs
    for L in (50, 500):
        e = exp["unrelated/%d" % L]
        assert e["status"] == 1 and e["cigar"].size > L // 4 and e["n_ins"] and e["n_del"], (L, e["status"], e["cigar"].size)
    assert exp["unrelated/3000"]["status"] == 0 and lens["unrelated/3000"] == (3000, 3000)
    assert all(a + b < 2 * 1300 or name == "unrelated/3000" for name, (a, b) in lens.items())
    return [(q, t, hq) for _, q, t, hq in jobs], [exp[name] for name, _, _, _ in jobs]


def check_golden(exp):
    """The golden set's own shapes (all 71 pairs)."""
    st = [e["status"] for e in exp]
    assert len(exp) == 71 and (st.count(1), st.count(0), st.count(2)) == (54, 15, 2), st
    assert max(int((e["cigar"] >> 4).max()) for e in exp if e["cigar"].size) == 2300
    assert sum(1 for e in exp if e["status"] == 1 and e["aln_len"] % 64 == 0) == 3
    assert all(e["aln_len"] == 2 and e["cigar"].size in (1, 2) for e in exp if e["status"] == 2)


def fuzz_pairs(n=250):
    """The generator of test_gpu_parity.test_align_fuzz_vs_oracle: lengths 1..5,999, three error profiles, every 4th hq."""
    from nextdenovo_amd import synth
    rng = np.random.default_rng(2024)
    out = []
    for it in range(n):
        L = int(rng.integers(1, 6000))
        base = rng.integers(0, 4 if it % 9 else 2, L, dtype=np.uint8)
        prof = ("ont", "clr", "hifi")[it % 3]
        q = synth.mutate(base, np.random.default_rng(3 * it), prof)[0]
        t = synth.mutate(base, np.random.default_rng(3 * it + 1), prof)[0]
        if it % 10 == 0:
            q = q[int(rng.integers(0, 40)):]
        if it % 17 == 0:
            t = np.concatenate([t[: t.size // 3], rng.integers(0, 4, int(rng.integers(1, 300)), dtype=np.uint8), t[t.size // 3:]])
        out.append((util.ASC[q].tobytes(), util.ASC[t].tobytes(), int(it % 4 == 0)))
    return out


def diff(got, exp):
    """Indices (with the first differing field) where a list of result dicts differs from the expected records, run by run."""
    bad = []
    if len(got) != len(exp):
        return [("count", len(got), len(exp))]
    for i, (g, e) in enumerate(zip(got, exp)):
        for f in FIELDS:
            if int(g[f]) != int(e[f]):
                bad.append((i, f, int(g[f]), int(e[f])))
                break
        else:
            if np.asarray(g["cigar"]).tolist() != np.asarray(e["cigar"]).tolist():
                bad.append((i, "cigar", len(g["cigar"]), len(e["cigar"])))
    return bad


# ---- the DB form: a small read DB and windows over it ----------------------------------------------------------------------------
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def db_reads(n=20):
    """n reads of 200..600 bases: mutated copies of four templates' heads, every other one stored reverse-complemented, so that
    windows of two reads of a template align under the right (q_rev, t_rev)."""
    from nextdenovo_amd import synth
    rng = np.random.default_rng(11)
    tmpl = [rng.integers(0, 4, 600, dtype=np.uint8) for _ in range(4)]
    reads = []
    for i in range(n):
        b = synth.mutate(tmpl[i % 4][: int(rng.integers(200, 601))], np.random.default_rng(100 + i), "ont")[0]
        reads.append((3 - b[::-1]).astype(np.uint8) if (i // 4) % 2 else b)     # (codes A0 C1 G2 T3: the complement is 3 - code)
    return reads


def window(reads, r, s, e, rev):
    """ReadDb::window on host copies: bases [s, e] of read r, reverse-complemented when rev"""
    w = util.ASC[reads[r][s:e + 1]].tobytes()
    return w[::-1].translate(COMP) if rev else w


def db_jobs(reads):
    """24 jobs (q_read, q_start, q_end, q_rev, t_read, t_start, t_end, t_rev, hq): the same stretch [lo, hi] of two reads' template,
    both presented on strand x -- for a read stored reverse-complemented that is the mirrored window with the other rev flag --,
    every 6th over two templates (nothing to align), every 3rd hq."""
    rng = np.random.default_rng(12)
    n = len(reads)

    def side(r, lo, hi, x):
        ln, stored_rc = len(reads[r]), (r // 4) % 2
        return (r, ln - 1 - hi, ln - 1 - lo, 1 - x) if stored_rc else (r, lo, hi, x)

    jobs = []
    for k in range(24):
        qr = int(rng.integers(0, n))
        tr = (qr + 4 * int(rng.integers(1, 5))) % n if k % 6 else (qr + 1) % n
        lo = int(rng.integers(0, 20))
        hi = min(len(reads[qr]), len(reads[tr])) - 1 - int(rng.integers(0, 20))
        x = (k >> 1) & 1
        jobs.append(side(qr, lo, hi, x) + side(tr, lo, hi, x) + (int(k % 3 == 0),))
    return jobs


def make_db(api, reads):
    from nextdenovo_amd import synth
    words = [synth.pack_2bit_msb(r) for r in reads]
    word_off = np.cumsum([0] + [w.size for w in words[:-1]]).astype(np.uint64)
    return api.ReadDB(np.concatenate(words), word_off, np.array([r.size for r in reads], dtype=np.uint32))


# ---- child processes: argv[1] = "simt" (the interpreted library) or "native", argv[2] = what to run --------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, util, aln_util
from nextdenovo_amd import api
if sys.argv[1] == "simt":
    import build_simt
    api._LIB = api._bind(C.CDLL(build_simt.build()))
else:
    api.load()
what = sys.argv[2]
olib = aln_util.oracle()
if what == "batch":          # directed set + golden pairs up to a total length: device, host flag, expected
    jobs, exp = aln_util.check_directed(olib)
    gj, ge = aln_util.golden_jobs(olib, int(sys.argv[3]) if sys.argv[3] != "all" else None)
    jobs, exp = jobs + gj, exp + ge
    api.reset_stats()
    dev = api.align_batch(jobs)
    st = api.stats()
    host = api.align_batch(jobs, host=True)
    print(json.dumps(dict(n=len(jobs), bad_dev=aln_util.diff(dev, exp)[:10], bad_host=aln_util.diff(host, exp)[:10], stats=st,
                          stats_after_host=api.stats(), runs=int(sum(e["cigar"].size for e in exp)),
                          statuses=[e["status"] for e in exp])))
elif what == "strings":      # the strings flag against align() / align_hq() of the same library
    jobs, _ = aln_util.check_directed(olib)
    jobs += aln_util.golden_jobs(olib, int(sys.argv[3]) if sys.argv[3] != "all" else None)[0]
    bad = []
    single = [util.gpu_align(api._LIB, q, t, hq) for q, t, hq in jobs]      # (aln_len, aln_t_len, aln_q_len, t_aln_str, q_aln_str)
    for host in (False, True):
        got = api.align_batch(jobs, strings=True, host=host)
        bad += [(host, i) for i, g in enumerate(got) if single[i] != (g["aln_len"], g["t_used"], g["q_used"], g["t_aln"], g["q_aln"])]
    print(json.dumps(dict(n=len(jobs), bad=bad[:10], aligned=sum(1 for g in got if g["status"] == 1), aborts=sum(1 for g in got if g["status"] == 2))))
elif what == "db":           # the DB form against the ASCII form on host copies of the same windows
    reads = aln_util.db_reads()
    jobs = aln_util.db_jobs(reads)
    db = aln_util.make_db(api, reads)
    pairs = [(aln_util.window(reads, j[0], j[1], j[2], j[3]), aln_util.window(reads, j[4], j[5], j[6], j[7]), j[8]) for j in jobs]
    exp = [aln_util.oracle_expect(olib, *p) for p in pairs]
    asc = api.align_batch(pairs, strings=True)
    api.reset_stats()
    got = db.align_batch(jobs, strings=True)
    st = api.stats()
    strings_differ = [i for i in range(len(jobs)) if (got[i]["q_aln"], got[i]["t_aln"]) != (asc[i]["q_aln"], asc[i]["t_aln"])]
    rcs = []
    n_reads = len(reads)
    for badjob in ((n_reads, 0, 10, 0, 0, 0, 10, 0, 0), (0, 0, 10, 0, n_reads + 5, 0, 10, 0, 0), (0, 0, len(reads[0]), 0, 1, 0, 10, 0, 0),
                   (0, 5, 4, 0, 1, 0, 10, 0, 0), (0, 0, 10, 1, 1, 0, len(reads[1]), 1, 0)):
        arr = (api.AlnDbJob * 2)(api.AlnDbJob(*jobs[0]), api.AlnDbJob(*badjob))
        res = (api.AlnResult * 2)()
        C.memset(res, 0x55, C.sizeof(res))
        cg = C.c_void_p(0x5555)
        rc = api._LIB.ndgpu_align_db_batch(db._h, arr, 2, 0, res, C.byref(cg), None, None)
        rcs.append([rc, bytes(res) == b"\x55" * C.sizeof(res) and cg.value == 0x5555])
    db.close()
    print(json.dumps(dict(n=len(jobs), bad_db=aln_util.diff(got, exp)[:10], bad_ascii=aln_util.diff(asc, exp)[:10], strings_differ=strings_differ,
                          revs=sorted({(j[3], j[7]) for j in jobs}), aligned=sum(1 for e in exp if e["status"] == 1), rcs=rcs, stats=st)))
elif what == "order":        # the forced-chunk variant of the GPU test: everything in one call, chunks of a few jobs
    jobs, exp = aln_util.check_directed(olib)
    gj, ge = aln_util.golden_jobs(olib)
    jobs, exp = jobs + gj, exp + ge
    api.reset_stats()
    dev = api.align_batch(jobs)
    print(json.dumps(dict(n=len(jobs), bad_dev=aln_util.diff(dev, exp)[:10], stats=api.stats())))
"""


def child(lib, what, *args, timeout=1500, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("NDGPU_ALIGN", "SIMT_"))}   # no switch of the caller's reaches the child
    e.update(env)
    if lib == "simt":
        e.setdefault("NDGPU_CONTEXTS", "1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE, os.path.join(HERE, "simt")), lib, what, *[str(a) for a in args]],
                         env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])
