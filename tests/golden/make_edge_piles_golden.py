#!/usr/bin/env python
"""Generate tests/golden/edge_piles.npz: hand-built piles for nextCorrect() and the REAL reference's answers.

Run in the build container (needs the reference compiled into oracle/_ref by `make -C oracle ref`, the oracle library and the
interpreted kernel library of tests/simt):

    python tests/golden/make_edge_piles_golden.py            # writes the fixture, prints cases / died / live checks per family
    python tests/golden/make_edge_piles_golden.py --check    # builds everything again and compares with the committed arrays

Every other pile of the suite is a simulated read set from a repeat-free genome at depth ~30, pushed through the overlap chain
and corrected with one set of arguments.  The piles here are built by hand from seeded numpy generators and
nextdenovo_amd.synth, each for one edge of the device path (tests/test_simt_edge_piles.py, tests/test_gpu_edge_piles.py):

  args     min_len_aln, max_cov_aln, min_cov_base, ratio, max_lq_length, split, fast away from their defaults, ONT / CLR / HiFi
  cut      records listed beyond the admission cut (total aligned length / seed length > max_cov_aln, lib/nextcorrect.c:2271)
  count    63, 64, 65, 127, 128, 129 reads accepted (the seed is one): the link counter takes accepted reads 64 at a time
  seedlen  seed lengths around multiples of 32 (column blocks) and 256, where the number of scoring segments changes (segments of
           1,024 columns, (L + 512) / 1024 of them: 1535 | 1536, 2559 | 2560), and the shortest seed with an answer
  window   windows at the seed's ends, alignments of min_len_aln and min_len_aln -+ 1 columns, stretches no read covers, unrelated
           reads between good ones, a read whose alignment hits the > 250-column gap marker, a read without a run of 8 matches
  lowc     homopolymer-run and tandem-repeat seeds, three read types, plain and -s
  repeat   insertions of distinct lengths in front of one column: more than 64 distinct links in one MSA cell, so the link
           counter's first attempt overflows and the sub-batch is repeated with the full capacity -- without any test switch
  int64    an insertion longer than the scoring kernels' column tables hold: the pile goes through the int64 kernel
  links    the same with more than 192 distinct links in one cell: more than the second attempt holds, a third one follows
  stack    hundreds of short reads on one window of a long seed: the admission cut inside them, the link counter's later chunks,
           more link slots in a column than the scoring kernels' tables hold (the int64 kernel by that route)

Layout: that of piles.npz (2-bit packed reads `codes` / `codes_off` / `lens`, per pile `pile_off`, `max_aln`, `max_lq`,
`read_type`, `fast`, `split`, `exp_len`, `exp_ide`, `exp_seq` / `exp_seq_off`, per record `aln_start`, `aln_end`) with
  * `rec_read`: per record, the index of its read in `codes_off` / `lens` -- many cases share reads (the argument variants of
    one pile, the nested piles of the count family), and stored once per case they would not fit a committed file;
  * per pile `tag`, `min_len_aln`, `max_cov_aln`, `min_cov_base`, `ratio`;
  * `died`: "tag signal" of every case in which the reference itself died.  Those cases carry no expectation; their inputs
    are kept in the same layout under `died_*` names, because the product must answer them with a status and live.
The reference runs in a forked child per case, because it can die (a min_len_aln larger than the seed, which then is not
in its own pile, is one way).  max_aln_length is what the reference's driver computes (lib/nextcorrect.py:129-133,
tests/refpipe.py:171): with less the reference corrupts its heap, such inputs are outside its domain.
The file holds data only: inputs, arguments, and the reference's (len, identity, sequence)."""
import ctypes as C
import os
import pickle
import signal
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refpipe  # noqa: E402
import util  # noqa: E402
from nextdenovo_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "edge_piles.npz")
DEFAULTS = dict(min_len_aln=500, max_cov_aln=130, min_cov_base=4, ratio=0.8, split=0, fast=0)
RT = {"ont": 1, "clr": 2, "hifi": 3}


def asc(codes):
    return util.ASC[np.asarray(codes, dtype=np.uint8)].tobytes()


def noisy(seg, prof, seed):
    return synth.mutate(np.asarray(seg, dtype=np.uint8), np.random.default_rng(seed), prof)[0]


def make_case(tag, seqs, st, en, prof="ont", max_lq=None, **args):
    """One nextCorrect() call: ASCII reads (the seed first), windows, read type, arguments."""
    L = len(seqs[0])
    assert st[0] == 0 and en[0] == L - 1 and len(seqs) == len(st) == len(en)
    rt = RT[prof]
    c = dict(DEFAULTS)
    c.update(args)
    c.update(tag=tag, seqs=list(seqs), aln_start=[int(x) for x in st], aln_end=[int(x) for x in en], read_type=rt,
             max_aln=max([L] + [e - s + 1 + len(q) + 2 for s, e, q in zip(st[1:], en[1:], seqs[1:])]),
             max_lq=min(L // 2, 10000 if rt == 1 else 1000) if max_lq is None else max_lq)
    return c


def variant(c, tag, n=None, **args):
    v = {k: x for k, x in c.items() if k != "ref"}
    v.update(args)
    v["tag"] = tag
    if n is not None:
        for k in ("seqs", "aln_start", "aln_end"):
            v[k] = c[k][:n]
    return v


# ---- the reference, one forked child per case --------------------------------------------------------------------------------
def run_ref(c):
    """(len, identity, sequence) of the reference, or the name of the signal that killed it."""
    lib = refpipe.ref_cns()
    r, w = os.pipe()
    sys.stdout.flush()
    pid = os.fork()
    if pid == 0:
        os.close(r)
        try:
            ln, ide, seq = refpipe.call_nextcorrect(lib, c["seqs"], c["aln_start"], c["aln_end"], c["max_aln"], c["min_len_aln"],
                                                    c["max_cov_aln"], c["min_cov_base"], c["max_lq"], c["ratio"], c["split"],
                                                    c["fast"], c["read_type"])
            os.write(w, pickle.dumps((ln, float(np.float32(ide)) if ln > 4 else 0.0, seq or b"")))
        finally:
            os._exit(0)
    os.close(w)
    blob = b""
    while True:
        part = os.read(r, 1 << 20)
        if not part:
            break
        blob += part
    os.close(r)
    _, status = os.waitpid(pid, 0)
    if os.WIFSIGNALED(status):
        return signal.Signals(os.WTERMSIG(status)).name
    assert blob, "the reference's child ended without an answer: " + c["tag"]
    return pickle.loads(blob)


def answer(c):
    if "ref" not in c:
        c["ref"] = run_ref(c)
    return c["ref"]


# ---- the interpreted kernels with NDGPU_TRACE, in a child process -------------------------------------------------------------
_TRACE_CHILD = r"""
import ctypes as C, pickle, sys
sys.path[:0] = [%r, %r, %r]
import util, build_simt
from nextdenovo_amd import api
lib = api._bind(C.CDLL(build_simt.build()))
fn, fr = util.bind_correct(lib)
c = pickle.load(open(sys.argv[1], "rb"))
out = util.call_correct(fn, fr, c, **{k: c[k] for k in ("min_len_aln", "max_cov_aln", "min_cov_base", "ratio")})
st = api.Stats()
lib.ndgpu_get_stats(C.byref(st))
pickle.dump((out, int(st.score_slow_piles), int(st.tags)), open(sys.argv[2], "wb"))
"""


def run_traced(c):
    """-> (answer of the interpreted library or None, what it wrote to stderr, piles through the int64 kernel, alignment tags of the
    reads it admitted to the MSA: the sum of their alignment lengths, the seed's included).  No force switch is set."""
    with tempfile.TemporaryDirectory() as wd:
        a, b = os.path.join(wd, "in.pkl"), os.path.join(wd, "out.pkl")
        with open(a, "wb") as f:
            pickle.dump({k: v for k, v in c.items() if k != "ref"}, f)
        env = {k: v for k, v in os.environ.items() if not k.startswith("NDGPU_")}
        env.update(NDGPU_TRACE="1", NDGPU_CONTEXTS="1")
        code = _TRACE_CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "simt"))
        r = subprocess.run([sys.executable, "-c", code, a, b], env=env, capture_output=True, text=True, timeout=1500)
        if r.returncode:
            return None, r.stderr, 0, 0
        out, slow, tags = pickle.load(open(b, "rb"))
        return (out[0], float(np.float32(out[1])) if out[0] > 4 else 0.0, out[2]), r.stderr, slow, tags


# ---- accepted reads, counted with the oracle's aligner as the host engine does (tests/csrc/host_harness.cpp) -----------------
def accepted_reads(c):
    ora = C.CDLL(os.path.join(ROOT, "oracle", "libndoracle.so"))
    ora.nd_oracle_shift.restype = C.c_int
    n, total, L = 0, 0, len(c["seqs"][0])
    for i, (q, s, e) in enumerate(zip(c["seqs"], c["aln_start"], c["aln_end"])):
        if total // L > c["max_cov_aln"]:
            break
        if i == 0:
            if L >= c["min_len_aln"]:
                n, total = n + 1, total + L
            continue
        o, _, _, ops = util.oracle_align(ora, q, c["seqs"][0][s:e + 1], int(c["read_type"] == 3))
        if o.status != 1:
            continue
        ts, te, sh = C.c_uint(s), C.c_uint(e), C.c_int(0)
        buf = (C.c_uint8 * ops.size).from_buffer_copy(ops.tobytes())
        ln = ora.nd_oracle_shift(buf, int(o.aln_len), 8, C.byref(ts), C.byref(te), C.byref(sh))
        if ln and ln >= c["min_len_aln"]:
            n, total = n + 1, total + te.value - ts.value + 1
    return n


# ---- families -----------------------------------------------------------------------------------------------------------------
def plain_pile(tag, L, n_reads, prof, seed, windows=None, seed_codes=None, read_prof=None, two_haplotypes=False, **args):
    """A seed of L bases and n_reads reads of the same molecule over `windows` (default: random windows of at least 700 bases).
    two_haplotypes: every second read comes from a copy of the seed with a substitution, a short insertion or a homopolymer
    length difference every 300 bases (what gives high-quality reads low-quality regions at all)."""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 4, L + 200, dtype=np.uint8) if seed_codes is None else np.asarray(seed_codes, dtype=np.uint8)
    s = noisy(truth, prof, seed + 1)[:L] if seed_codes is None else truth
    L = s.size
    seqs, st, en = [asc(s)], [0], [L - 1]
    for i in range(n_reads):
        if windows is not None:
            a, b = windows[i % len(windows)]
        else:
            a = int(rng.integers(0, max(1, L - 700))) if i % 3 else 0
            b = L - 1 if i % 3 == 1 else min(L - 1, a + int(rng.integers(700, L + 1)))
        src = s[a:b + 1]
        if two_haplotypes and i % 2:
            parts, at = [], 0
            for pos in range((150 - a) % 300, src.size - 20, 300):   # seed columns 150, 450, ...
                kind = ((a + pos) // 300) % 3
                parts.append(src[at:pos])
                at = pos
                if kind == 0:
                    parts.append(np.asarray([(src[pos] + 1) & 3], dtype=np.uint8))
                    at = pos + 1
                elif kind == 1:
                    parts.append(np.resize(np.asarray([2, 0, 3, 1], dtype=np.uint8), 1 + ((a + pos) // 300) % 4))
                else:
                    parts.append(np.full(5, src[pos], dtype=np.uint8))
            src = np.concatenate(parts + [src[at:]])
        seqs.append(asc(noisy(src, read_prof or prof, seed * 1000 + i)))
        st.append(a)
        en.append(b)
    return make_case(tag, seqs, st, en, prof, **args)


def differs(a, b):
    return a[0] != b[0] or a[2] != b[2] or a[1] != b[1]


def args_family(live):
    cases = []
    for prof in ("ont", "clr", "hifi"):
        base = plain_pile("args/%s/default" % prof, 2400, 30 if prof == "hifi" else 16, prof, 40 + RT[prof], two_haplotypes=prof == "hifi")
        var = [("max_cov_aln", dict(max_cov_aln=1)), ("max_cov_aln", dict(max_cov_aln=3)), ("max_cov_aln", dict(max_cov_aln=6)),
               ("min_cov_base", dict(min_cov_base=1)), ("min_cov_base", dict(min_cov_base=12)),
               ("ratio", dict(ratio=0.3)), ("ratio", dict(ratio=0.97)),
               ("min_len_aln", dict(min_len_aln=50)), ("min_len_aln", dict(min_len_aln=1500)), ("min_len_aln", dict(min_len_aln=2390)),
               ("max_lq_length", dict(max_lq=0)), ("max_lq_length", dict(max_lq=40)), ("max_lq_length", dict(max_lq=6)),
               ("fast", dict(fast=1)), ("split", dict(split=1)), ("fast", dict(fast=1, split=1)),
               ("split", dict(split=1, min_cov_base=12)), ("records", dict(n=1)), ("records", dict(n=2))]
        if prof == "ont":       # larger than the seed: the seed is not in its own pile
            var.append(("min_len_aln", dict(min_len_aln=3000)))
        cases.append(base)
        seen = {}
        for name, kw in var:
            v = variant(base, "args/%s/%s" % (prof, ",".join("%s=%s" % kv for kv in sorted(kw.items()))), **kw)
            cases.append(v)
            if not isinstance(answer(v), str) and differs(answer(v), answer(base)):
                seen[name] = True
        for name in ("max_cov_aln", "min_cov_base", "min_len_aln", "max_lq_length", "split", "fast"):
            live("args: %s changes the reference's answer (%s)" % (name, prof), seen.get(name, False))
        # ratio: the default pile is corrected almost everywhere, so no ratio between 0.3 and 0.97 changes its fate.  A seed
        # with 900 of 2,400 bases uncovered in its middle is the pile where it does: the uncorrected part fails 0.8 and passes 0.3
        # (an uncovered END is stripped before the ratio is taken, and changes nothing).
        half = plain_pile("args/%s/half-covered" % prof, 2400, 14, prof, 60 + RT[prof], windows=[(0, 800), (0, 750), (1700, 2399), (1650, 2399)])
        lo = variant(half, "args/%s/half-covered,ratio=0.3" % prof, ratio=0.3)
        cases += [half, lo]
        if prof == "hifi":
            # No such pile exists for HiFi reads: their consensus (generate_cns_from_best_score_kmer, lib/nextcorrect.c:1786) never
            # counts an uncorrected base, so the ratio test of :1864-1865 holds for every ratio <= 1, and -fast does not read the
            # argument at all.  The two cases stay, as cases in which it must change nothing.
            live("args: ratio changes nothing for HiFi reads", not differs(answer(half), answer(lo)) and answer(half)[0] > 4)
        else:
            live("args: ratio changes the reference's answer (%s)" % prof, differs(answer(half), answer(lo)))
    return cases


def cut_family(live):
    """Records beyond the admission cut.  `at` keeps what the cut keeps, `below` one record less."""
    cases = []
    for prof, cov in (("ont", 5), ("clr", 8)):
        full = plain_pile("cut/%s/full" % prof, 1500, 14, prof, 70 + RT[prof], windows=[(0, 1499)], max_cov_aln=cov)
        n = len(full["seqs"])
        k = n
        while k > 1 and not differs(answer(variant(full, "x", n=k - 1)), answer(full)):
            k -= 1
        at, below = variant(full, "cut/%s/at" % prof, n=k), variant(full, "cut/%s/below" % prof, n=k - 1)
        live("cut: the pile lists %d records beyond the cut, which change nothing (%s)" % (n - k, prof),
             k < n and not differs(answer(at), answer(full)))
        live("cut: one record less changes the answer (%s)" % prof, differs(answer(below), answer(full)))
        live("cut: the cut falls where total / L first exceeds max_cov_aln (%s)" % prof, accepted_reads(full) == k)
        cases += [full, at, below]
    return cases


def count_family(live):
    """Full-window reads far below the coverage cut, so records handed in are reads accepted -- counted with the oracle's aligner and
    confirmed on the interpreted library, which reports the alignment tags of the reads it admitted (`tags` of its statistics)."""
    pile = plain_pile("count/pool", 800, 131, "ont", 81, windows=[(0, 799)])
    cases = []
    for k in (63, 64, 65, 127, 128, 129):
        c = variant(pile, "count/%d" % k, n=k)
        live("count: %d records are %d accepted reads" % (k, k), accepted_reads(c) == k)
        live("count: ... and for the interpreted library: record %d adds its tags to those of the %d before it" % (k, k - 1),
             run_traced(c)[3] > run_traced(variant(pile, "x", n=k - 1))[3] + 500)
        cases.append(c)
    for k in (64, 128):   # the same edges reached by the cut: records are listed beyond it
        # (trimmed to their outermost runs of eight matches the reads are a little shorter than the seed, so the cut comes later)
        m = next(m for m in range(k - 6, k + 2) if accepted_reads(variant(pile, "x", n=k + 3, max_cov_aln=m)) == k)
        c = variant(pile, "count/cut-at-%d" % k, n=k + 3, max_cov_aln=m)
        live("count: the cut leaves %d accepted reads of %d records" % (k, k + 3), accepted_reads(c) == k)
        # ... and by the interpreted library itself, not only by this file's model of the cut: it admits exactly the alignment
        # tags of the first k records (every read is about 800 tags), whatever stands behind them.  (The reference's answer
        # cannot tell: at this depth one read more or less changes nothing in it.)
        same, less, more = (run_traced(variant(pile, "x", n=j))[3] for j in (k, k - 1, k + 1))
        mine = run_traced(c)[3]
        live("count: the interpreted library admits the first %d records of the cut pile, not %d or %d" % (k, k - 1, k + 1),
             mine == same and less + 500 < mine < more - 500)
        cases.append(c)
    return cases


def seedlen_family(live):
    cases = []
    for L in (511, 512, 513, 543, 544, 545, 767, 768, 769, 1023, 1024, 1025, 1535, 1536, 1537, 2048, 2559, 2560):
        cases.append(plain_pile("seedlen/%d" % L, L, 6, "ont", 1000 + L, windows=[(0, L - 1), (0, L - 1), (0, L - 2), (1, L - 1)],
                                read_prof="hifi"))
    live("seedlen: every seed is answered with a sequence", all(answer(c)[0] > 4 for c in cases))
    # the shortest seed with an answer: the seed itself must reach min_len_aln, and so must the reads inside it
    rng = np.random.default_rng(91)
    s = rng.integers(0, 4, 501, dtype=np.uint8)
    for L in (499, 500, 501):
        cases.append(make_case("seedlen/%d-exact-copies" % L, [asc(s[:L])] * 7, [0] * 7, [L - 1] * 7))
    live("seedlen: 500 bases is the shortest seed with a sequence (at 499 the reference dies)", isinstance(answer(cases[-3]), str) and answer(cases[-2])[0] > 4 and answer(cases[-1])[0] > 4)
    return cases


def window_family(live):
    cases = []
    L = 3000
    W = [(0, 499), (0, 500), (0, 507), (L - 500, L - 1), (L - 501, L - 1), (0, L - 1), (1, L - 2), (1200, 1720), (0, 1500),
         (1499, L - 1), (600, 1200), (900, 1500), (1800, L - 1)]
    for prof in ("ont", "hifi"):
        cases.append(plain_pile("window/%s/ends" % prof, L, 26, prof, 100 + RT[prof], windows=W))
    # alignments of exactly min_len_aln columns and one more / one less: exact copies of a window but for one substitution, which
    # the aligner writes as an insertion and a deletion -- aln_len is the window and one column
    rng = np.random.default_rng(111)
    s = noisy(rng.integers(0, 4, 1700, dtype=np.uint8), "ont", 112)[:1500]
    for n in (498, 499, 500):
        seqs, st, en = [asc(s)], [0], [1499]
        for i in range(8):
            a = 100 + 90 * i
            v = s[a:a + n].copy()
            v[n // 2] = (v[n // 2] + 1) & 3       # every read carries the same substitution: five reads outvote the seed
            seqs.append(asc(v))
            st.append(a)
            en.append(a + n - 1)
        cases.append(make_case("window/aln-len-%d" % (n + 1), seqs, st, en))
    live("window: alignments of min_len_aln columns are taken (a sequence), those of min_len_aln - 1 are not (a status)",
         answer(cases[-3])[0] <= 4 < answer(cases[-2])[0] and [accepted_reads(c) for c in cases[-3:]] == [1, 9, 9])
    # stretches of the seed no read covers
    gaps = [(0, 1000), (0, 900), (2000, L - 1), (2100, L - 1)]
    for prof, kw in (("ont", {}), ("ont", dict(split=1)), ("hifi", {}), ("hifi", dict(split=1)), ("clr", dict(split=1))):
        cases.append(plain_pile("window/%s/uncovered%s" % (prof, ",split=1" if kw else ""), L, 40, prof, 120 + RT[prof], windows=gaps, **kw))
    live("window: the uncovered seed is a status for ONT and CLR reads, a sequence for HiFi reads",
         [answer(c)[0] > 4 for c in cases[-5:]] == [False, False, True, True, False])
    # reads that fail in the middle of a pile.  The seed has no 'A' so that a run of 'A' cannot be matched away.
    s3 = np.random.default_rng(131).integers(1, 4, 1600, dtype=np.uint8)
    good = [noisy(s3, "ont", 1320 + i) for i in range(12)]
    gap = np.concatenate([s3[:800], np.zeros(260, dtype=np.uint8), s3[800:]])            # > 250 gap columns: the marker
    comb = s3.copy()
    comb[3::7] = (comb[3::7] + 1) & 3                                                       # never eight matches in a row
    junk = [np.random.default_rng(1340 + i).integers(0, 4, 1500 + 40 * i, dtype=np.uint8) for i in range(3)]
    order = good[:3] + [junk[0]] + good[3:5] + [gap] + good[5:7] + [comb, junk[1]] + good[7:10] + [junk[2]] + good[10:]
    c = make_case("window/failing-reads-between", [asc(s3)] + [asc(q) for q in order], [0] * (1 + len(order)), [1599] * (1 + len(order)))
    only_good = make_case("window/failing-reads-left-out", [asc(s3)] + [asc(q) for q in good], [0] * 13, [1599] * 13)
    cases += [c, only_good]
    live("window: reads that fail change nothing", not differs(answer(c), answer(only_good)))
    live("window: the failing reads are not accepted", accepted_reads(c) == 13)
    return cases


def lowc_family(live):
    cases = []
    for kind in ("homopolymer", "tandem"):
        for prof in ("ont", "clr", "hifi"):
            rng = np.random.default_rng(140 + RT[prof] + (10 if kind == "tandem" else 0))
            parts, n = [], 0
            while n < 1500:
                if kind == "homopolymer":     # runs of 5 .. 40 between short random stretches
                    parts += [np.full(int(rng.integers(5, 40)), int(rng.integers(0, 4)), dtype=np.uint8), rng.integers(0, 4, int(rng.integers(3, 30)), dtype=np.uint8)]
                else:                         # units of 2 .. 6, 5 .. 60 copies, between random stretches
                    parts += [np.tile(rng.integers(0, 4, int(rng.integers(2, 7)), dtype=np.uint8), int(rng.integers(5, 60))), rng.integers(0, 4, int(rng.integers(20, 200)), dtype=np.uint8)]
                n += parts[-2].size + parts[-1].size
            s = np.concatenate(parts)[:1500]
            c = plain_pile("lowc/%s/%s" % (kind, prof), 1500, 10, prof, 150 + RT[prof], seed_codes=s)
            cases += [c, variant(c, c["tag"] + ",split=1", split=1)]
    live("lowc: at least ten of twelve piles are answered with a sequence", sum(answer(c)[0] > 4 for c in cases) >= 10)
    return cases


TRACE_REPEAT = "sub-batch repeated with 192"
TRACE_THIRD = "sub-batch repeated with the lists in device memory"


def craft_pile(tag, lengths, L=1200, w0=300, wlen=520, seed=161, n_bg=8, **args):
    """Exact copies of one window that each carry one insertion in front of the same column.  The seed has no 'A' and an insertion is a
    run of 'A', closed by 'A' or by a base that differs from the seed's bases on either side: no inserted base can be matched
    away or slide, the alignment keeps the run as one gap in that place.  The tag in front of the column -- (column - 1, length, last
    base) -- and with it the link into the column's cell is then a different one per (length, last base).
    lengths: [(inserted bases, 0 | 1: closed by 'A' | by the other base)]."""
    rng = np.random.default_rng(seed)
    s = rng.integers(1, 4, L, dtype=np.uint8)
    seqs, st, en = [asc(s)], [0], [L - 1]
    for i in range(n_bg):
        seqs.append(asc(noisy(s, "ont", seed * 100 + i)))
        st.append(0)
        en.append(L - 1)
    col = w0 + wlen // 2
    other = next(b for b in (1, 2, 3) if b != s[col - 1] and b != s[col])
    for ell, last in lengths:
        ins = np.zeros(ell, dtype=np.uint8)
        if last:
            ins[-1] = other
        seqs.append(asc(np.concatenate([s[w0:col], ins, s[col:w0 + wlen]])))
        st.append(w0)
        en.append(w0 + wlen - 1)
    return make_case(tag, seqs, st, en, **args)


def repeat_family(live):
    """The smallest pile of this build that overflows the first attempt's 64 links per cell, found with the interpreter's trace."""
    for n in range(60, 80):
        c = craft_pile("repeat/%d-insertions" % n, [(1 + i // 2, i % 2) for i in range(n)])
        got, err, _, _ = run_traced(c)
        if TRACE_REPEAT in err:
            break
    live("repeat: the interpreted library traces the K9 repeat without a switch (%d crafted reads)" % n, TRACE_REPEAT in err and TRACE_THIRD not in err)
    live("repeat: its answer is the reference's", got is not None and not differs(got, answer(c)))
    return [c]


def int64_family(live):
    """One read with an insertion of n bases makes a column n + 1 cell rows wide.  The scoring kernels' small tables take 16 rows,
    the large ones 32; beyond that the pile goes through the int64 kernel.  The smallest n of each tier, found with the trace."""
    cases, first = [], None
    for n in (15, 16, 31, 32, 33):
        c = craft_pile("int64/%d-base-insertion" % n, [(n, 1)], L=900, w0=100, wlen=640, seed=171)
        got, _, slow, _ = run_traced(c)
        live("int64: %d inserted bases, the answer is the reference's" % n, got is not None and not differs(got, answer(c)))
        if slow and first is None:
            first = n
        cases.append(c)
    live("int64: a pile goes through the int64 kernel without a switch, from 32 inserted bases on (33 rows)", first == 32)
    return cases


def stack_pile(tag, n_records, L=6000, w0=2600, wlen=700, n_distinct=24, n_bg=10, seed=181, **args):
    """Local depth far above the average: n_records reads of wlen bases on one window of a long seed.  The records list
    n_distinct noisy reads of that window in turn (the fixture stores a read once), each on a window of its own start, over a
    background of n_bg long reads."""
    rng = np.random.default_rng(seed)
    s = noisy(rng.integers(0, 4, L + 600, dtype=np.uint8), "ont", seed + 1)[:L]
    seqs, st, en = [asc(s)], [0], [L - 1]
    for i in range(n_bg):
        a = int(rng.integers(0, L // 2))
        b = min(L - 1, a + int(rng.integers(2500, 4000)))
        seqs.append(asc(noisy(s[a:b + 1], "ont", seed * 100 + i)))
        st.append(a)
        en.append(b)
    var = s.copy()
    var[w0 + wlen // 2] = (var[w0 + wlen // 2] + 1) & 3        # the stack outvotes the seed on one base
    pool = []
    for i in range(n_distinct):
        a = w0 + int(rng.integers(0, 20))
        pool.append((asc(noisy(var[a:a + wlen], "ont", seed * 1000 + i)), a, a + wlen - 1))
    for i in range(n_records):
        q, a, b = pool[i % n_distinct]
        seqs.append(q)
        st.append(a)
        en.append(b)
    return make_case(tag, seqs, st, en, **args)


def stack_family(live):
    cases = []
    # the admission cut inside the stack: the average coverage is at the limit while one window holds nearly all of it
    cut = stack_pile("stack/cut-inside-the-stack", 700, max_cov_aln=60)
    n_acc, n, L = accepted_reads(cut), len(cut["seqs"]), len(cut["seqs"][0])
    live("stack: the cut falls inside the stacked records (%d of %d accepted)" % (n_acc, n), 300 < n_acc < n - 50)
    live("stack: the window is %d deep, the average coverage 61" % (n_acc - 11), (n_acc - 11) * L > 6 * 61 * L)
    got, err, slow, tags = run_traced(cut)
    at, below = variant(cut, "x", n=n_acc), variant(cut, "x", n=n_acc - 1)
    live("stack: the records behind the cut change nothing for the reference", not differs(answer(cut), answer(at)))
    live("stack: the interpreted library admits the records up to the cut and no other",
         tags == run_traced(at)[3] and tags > run_traced(below)[3] + 500)
    live("stack: the cut pile's answer is the reference's", got is not None and not differs(got, answer(cut)))
    cases.append(cut)
    # more link slots in a column (coverage + inserted bases) than the scoring kernels' large tables hold (512): the int64
    # kernel by another route than a wide column -- at 300 records the same pile stays on the tables
    deep, shallow = stack_pile("stack/600-deep", 600), stack_pile("x", 300)
    got, err, slow, _ = run_traced(deep)
    live("stack: 600 reads on a window go through the int64 kernel without a switch", got is not None and slow >= 1)
    live("stack: its answer is the reference's, every record accepted", got is not None and not differs(got, answer(deep)) and accepted_reads(deep) == len(deep["seqs"]))
    got, err, slow, _ = run_traced(shallow)
    live("stack: 300 reads on the window do not (the route is the column's slot count, not its width)", got is not None and slow == 0)
    cases.append(deep)
    return cases


def links_family(live):
    """More than 192 distinct links in one cell -- more than the link counter's second attempt holds (kLinkCap in
    nextdenovo_amd/csrc/nd_device.h): the sub-batch is counted a third time with the lists in device memory.  Default arguments,
    every read accepted, coverage below 90: well inside what the reference takes, and it answers with a sequence."""
    for n in range(188, 216, 2):
        c = craft_pile("links/%d-insertions" % n, [(1 + i // 2, i % 2) for i in range(n)])
        got, err, _, _ = run_traced(c)
        if TRACE_THIRD in err:
            break
    live("links: the interpreted library traces the third attempt (%d crafted reads)" % n, TRACE_REPEAT in err and TRACE_THIRD in err)
    live("links: its answer is the reference's, a sequence", got is not None and not differs(got, answer(c)) and got[0] > 4)
    live("links: every record is an accepted read", accepted_reads(c) == len(c["seqs"]))
    return [c]


FAMILIES = [("args", args_family), ("cut", cut_family), ("count", count_family), ("seedlen", seedlen_family),
            ("window", window_family), ("lowc", lowc_family), ("repeat", repeat_family), ("int64", int64_family),
            ("links", links_family), ("stack", stack_family)]


# ---- the file -----------------------------------------------------------------------------------------------------------------
def pack2(codes):
    n = codes.size
    pad = np.zeros((n + 3) // 4 * 4, dtype=np.uint8)
    pad[:n] = codes
    pad = pad.reshape(-1, 4)
    return (pad[:, 0] | (pad[:, 1] << 2) | (pad[:, 2] << 4) | (pad[:, 3] << 6)).astype(np.uint8)


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
            packed.append(pack2(c))
            lens.append(len(s))
        return pool[s]

    keys = ("pile_off", "rec_read", "aln_start", "aln_end", "max_aln", "max_lq", "read_type", "fast", "split", "min_len_aln",
            "max_cov_aln", "min_cov_base", "ratio", "tag")
    tab = {pre: {k: [0] if k == "pile_off" else [] for k in keys} for pre in ("", "died_")}
    exp = {"exp_len": [], "exp_ide": [], "exp_seq": []}
    died, report, checks = [], [], []
    for name, fam in FAMILIES:
        n_live = [0, 0]

        def live(what, ok):
            n_live[0] += 1
            n_live[1] += bool(ok)
            checks.append((what, bool(ok)))
            print("  %-4s %s" % ("ok" if ok else "FAIL", what), flush=True)

        print("family %s" % name, flush=True)
        cases = fam(live)
        n_died = 0
        for c in cases:
            ref = answer(c)
            t = tab["died_" if isinstance(ref, str) else ""]
            for s in c["seqs"]:
                t["rec_read"].append(read_index(s))
            t["pile_off"].append(t["pile_off"][-1] + len(c["seqs"]))
            t["aln_start"] += c["aln_start"]
            t["aln_end"] += c["aln_end"]
            for k in keys[4:]:
                t[k].append(c[k])
            if isinstance(ref, str):
                n_died += 1
                died.append("%s %s" % (c["tag"], ref))
            else:
                exp["exp_len"].append(ref[0])
                exp["exp_ide"].append(ref[1])
                exp["exp_seq"].append(np.frombuffer(ref[2], dtype=np.uint8))
        assert n_died * 20 <= max(len(cases), 20), "family %s: the reference died in %d of %d cases -- its inputs are wrong" % (name, n_died, len(cases))
        report.append("%-8s %3d cases, %d died, %d / %d live checks passed" % (name, len(cases), n_died, n_live[1], n_live[0]))
    tags = tab[""]["tag"] + tab["died_"]["tag"]
    assert len(set(tags)) == len(tags), "case tags must be unique"
    dt = dict(pile_off=np.int64, rec_read=np.int32, aln_start=np.uint32, aln_end=np.uint32, max_aln=np.uint32, max_lq=np.uint32,
              read_type=np.int32, fast=np.int32, split=np.int32, min_len_aln=np.uint32, max_cov_aln=np.uint32, min_cov_base=np.uint32,
              ratio=np.float32, tag=np.str_)
    arrays = {}
    for pre, t in tab.items():
        for k in keys:
            arrays[pre + k] = np.asarray(t[k], dtype=dt[k])
    off = np.zeros(len(packed) + 1, dtype=np.int64)
    np.cumsum([a.size for a in packed], out=off[1:])
    arrays.update(codes=np.concatenate(packed), codes_off=off, lens=np.asarray(lens, dtype=np.int32),
                  exp_len=np.asarray(exp["exp_len"], dtype=np.uint32), exp_ide=np.asarray(exp["exp_ide"], dtype=np.float32),
                  died=np.asarray(died, dtype=np.str_))
    eoff = np.zeros(len(exp["exp_seq"]) + 1, dtype=np.int64)
    np.cumsum([a.size for a in exp["exp_seq"]], out=eoff[1:])
    arrays.update(exp_seq=np.concatenate(exp["exp_seq"]), exp_seq_off=eoff)
    return arrays, report, checks


def main():
    assert refpipe.have_ref("nextcorrect.so"), "build the reference first: make -C oracle ref"
    arrays, report, checks = build_arrays()
    print("\n".join(report))
    failed = [w for w, ok in checks if not ok]
    assert not failed, "live checks failed: %s" % failed
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(arrays), (sorted(old.files), sorted(arrays))
        for k, v in arrays.items():
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v), "array %s differs from the committed fixture" % k
        print("%s: the same %d arrays" % (os.path.basename(OUT), len(arrays)))
        return
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("%s: %d piles (%d died), %d reads, %d bytes" % (os.path.basename(OUT), arrays["tag"].size, arrays["died"].size, arrays["lens"].size, size))
    assert size <= 190766, "larger than the largest file under tests/golden"


if __name__ == "__main__":
    main()
