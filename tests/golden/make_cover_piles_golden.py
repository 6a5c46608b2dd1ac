#!/usr/bin/env python
"""Generate tests/golden/cover_piles.npz: piles for the link counter's two ways through a column block, and the REAL
reference's answers.

    python tests/golden/make_cover_piles_golden.py            # writes the fixture
    python tests/golden/make_cover_piles_golden.py --check    # builds everything again and compares with the committed arrays

(needs what make_edge_piles_golden.py needs: the reference compiled into oracle/_ref, the oracle library, tests/simt.)

count_links_kernel (nextdenovo_amd/csrc/msa_kernels.hip) owns 32 columns of a pile per wavefront.  It first counts the accepted
reads that reach those columns (the block's COVER): with at most 64 of them -- NDGPU_K9_COMPACT=<T> lowers the limit -- the
block takes the compact path, one lane per covering read; with more, the deep path over all accepted reads, 64 at a time.  The
piles here put blocks on both sides of that limit, inside one pile, and blocks exactly at it:

  stair   one pile per read type (ONT, CLR, HiFi).  A seed of 2,400 bases and 151 reads (152 accepted, the seed is one: three
          chunks of 64 for the deep path).  The reads' windows, each at least 520 bases, are staggered so that the number of
          reads reaching a 32-column block climbs from about 30 at the seed's first columns to about 90 in its middle and comes
          down again -- by one read per block where it passes 64 and 65, so blocks with exactly 64 and exactly 65 covering
          reads exist.  Windows begin at a block's first and at its last column, and end at a block's last column and at the
          next block's first.  The first and last 16 bases of a read are exact copies of the seed, so the alignment keeps the
          window as it is (t_s, t_e: the window) and the cover of a block is what stair_windows() computes.  The
          average depth stays far below max_cov_aln: the admission cut takes nothing away.
          The CLR and HiFi piles are recorded a second time as ONT piles (`,read_type=ont`): read type is an argument of a
          whole batched call, and the tests put all piles into one.
  flat    64 full-window reads (exact ends again) and a seed of 1,000 bases: 65 reads on every block (the seed is accepted into
          its own pile, at rank 0).
          And the same pile with 63 reads: every block at exactly 64.

Layout and fields: those of edge_piles.npz (make_edge_piles_golden.py), so tests/util.py's edge_wrong, call_correct and edge_args
apply.  The file holds data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_edge_piles_golden as E  # noqa: E402  (puts the repository, tests/ and tests/simt on the path)

OUT = os.path.join(HERE, "cover_piles.npz")
BLOCK = 32          # kColBlock
EXACT_ENDS = 16     # bases at either end of a read that are copies of the seed


def stair_windows(L=2400):
    """-> windows [(a, b)], cover per block.  The cover climbs and falls by `step(c)` reads per block: by one between 58 and 72,
    faster elsewhere.  Every block of the middle also retires its oldest read or two (once long enough) and begins others in their place,
    which is what brings the pile to ~150 reads, three chunks of 64."""
    K = L // BLOCK
    lo, hi = 30, 90

    def step(c):
        return 1 if 58 <= c < 72 else 4 if c < 58 else 2

    up = [lo]
    while up[-1] < hi:
        up.append(min(hi, up[-1] + step(up[-1])))
    assert 2 * len(up) <= K
    target = up + [hi] * (K - 2 * len(up)) + up[::-1]
    start_off = [0, 31, 5, 13, 22, 9, 27, 16, 3, 30, 18, 1]      # a block's first and last column among them
    end_off = [31, 0, 7, 24, 31, 0, 12, 19, 2, 29]               # ends at a block's last column, at the next block's first
    active, done, n_s, n_e = [], [], 0, 0                        # active: (start column, start block), oldest first
    for k in range(K):
        want = target[k] - 1                                     # the seed covers every block
        n_end = max(0, len(active) - want) + (2 if 25 <= k <= 48 else 1 if 19 <= k <= K - 19 else 0)   # (a read begun later had no 520 bases left)
        while n_end and active and k - 1 - active[0][1] >= 18:   # the oldest reads end in block k - 1, once they have 520 bases
            a, _ = active.pop(0)
            done.append((a, (k - 1) * BLOCK + end_off[n_e % len(end_off)]))
            n_e, n_end = n_e + 1, n_end - 1
        while len(active) < want:
            active.append((0 if k == 0 else k * BLOCK + start_off[n_s % len(start_off)], k))
            n_s += 1
    done += [(a, L - 1) for a, _ in active]
    assert all(b - a + 1 >= 520 for a, b in done), min(b - a + 1 for a, b in done)
    cover = [1 + sum(a < (k + 1) * BLOCK and b >= k * BLOCK for a, b in done) for k in range(K)]
    return done, cover


def stair_pile(prof, seed):
    L = 2400
    windows, cover = stair_windows(L)
    rng = np.random.default_rng(seed)
    s = E.noisy(rng.integers(0, 4, L + 400, dtype=np.uint8), prof, seed + 1)[:L]
    seqs, st, en = [E.asc(s)], [0], [L - 1]
    for i, (a, b) in enumerate(windows):
        src = s[a:b + 1]
        mid = E.noisy(src[EXACT_ENDS:-EXACT_ENDS], prof, seed * 1000 + i)
        seqs.append(E.asc(np.concatenate([src[:EXACT_ENDS], mid, src[-EXACT_ENDS:]])))
        st.append(a)
        en.append(b)
    return E.make_case("stair/%s" % prof, seqs, st, en, prof), windows, cover


def stair_family(live):
    cases = []
    for prof, seed in (("ont", 211), ("clr", 212), ("hifi", 213)):
        c, windows, cover = stair_pile(prof, seed)
        n = len(c["seqs"])
        live("stair: %d records, all accepted -- three chunks of 64 (%s)" % (n, prof), 140 <= n <= 192 and E.accepted_reads(c) == n)
        live("stair: covers %d .. %d, blocks with exactly 64 and exactly 65 reads (%s)" % (min(cover), max(cover), prof),
             min(cover) <= 32 and max(cover) >= 88 and 64 in cover and 65 in cover and 63 in cover)
        live("stair: windows begin at a block's first and last column and end at a block's last column and the next one's first",
             {a % BLOCK for a, _ in windows} >= {0, 31} and {b % BLOCK for _, b in windows} >= {0, 31})
        live("stair: average depth %d, below max_cov_aln" % (sum(b - a + 1 for a, b in windows) // 2400),
             sum(b - a + 1 for a, b in windows) // 2400 + 1 < c["max_cov_aln"])
        live("stair: the reference answers with a sequence (%s)" % prof, E.answer(c)[0] > 4)
        cases.append(c)
        if prof != "ont":
            cases.append(E.variant(c, c["tag"] + ",read_type=ont", read_type=1, max_lq=min(2400 // 2, 10000)))
    return cases


def flat_family(live):
    L = 1000
    s = E.noisy(np.random.default_rng(221).integers(0, 4, L + 200, dtype=np.uint8), "ont", 222)[:L]
    reads = [np.concatenate([s[:EXACT_ENDS], E.noisy(s[EXACT_ENDS:-EXACT_ENDS], "ont", 221000 + i), s[-EXACT_ENDS:]]) for i in range(64)]
    pile = E.make_case("flat/65", [E.asc(s)] + [E.asc(q) for q in reads], [0] * 65, [L - 1] * 65)
    one_less = E.variant(pile, "flat/64", n=64)
    for c, n in ((pile, 65), (one_less, 64)):
        live("flat: %d accepted reads, every one on every block" % n, len(c["seqs"]) == n and E.accepted_reads(c) == n)
        live("flat: the reference answers with a sequence", E.answer(c)[0] > 4)
    return [pile, one_less]


def main():
    assert E.refpipe.have_ref("nextcorrect.so"), "build the reference first: make -C oracle ref"
    E.FAMILIES = [("stair", stair_family), ("flat", flat_family)]
    arrays, report, checks = E.build_arrays()
    print("\n".join(report))
    failed = [w for w, ok in checks if not ok]
    assert not failed, "live checks failed: %s" % failed
    assert arrays["died"].size == 0
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(arrays), (sorted(old.files), sorted(arrays))
        for k, v in arrays.items():
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v), "array %s differs from the committed fixture" % k
        print("%s: the same %d arrays" % (os.path.basename(OUT), len(arrays)))
        return
    np.savez_compressed(OUT, **arrays)
    print("%s: %d piles, %d reads, %d bytes" % (os.path.basename(OUT), arrays["tag"].size, arrays["lens"].size, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
