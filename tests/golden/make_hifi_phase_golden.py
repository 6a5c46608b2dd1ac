#!/usr/bin/env python
"""Generate tests/golden/hifi_phase_piles.npz: HiFi piles (read type 3) whose low-quality regions go through the second half of
generate_lqseqs_from_tags_kmer (lib/nextcorrect.c:874-948: the phased choice, remove_differ_len, the sort by length, the trims, the
8-mer ranking with c = 40 and its tail pass), with the REAL reference's answers.

Run in the build container (needs the reference compiled into oracle/_ref by `make -C oracle ref` and the interpreted kernel
library of tests/simt):

    python tests/golden/make_hifi_phase_golden.py            # writes the fixture, prints what the rule met pile by pile
    python tests/golden/make_hifi_phase_golden.py --check    # builds everything again and compares with the committed arrays

The HiFi piles of piles.npz and edge_piles.npz end nearly every region as a pseudo-seed.  The piles here have a 3,000-base truth and
reads over the full window, of two kinds:
  (a) two haplotypes that differ every 300 bases by a substitution, a short insertion or a homopolymer length (`sites`: all three,
      substitutions only, or none of them), the seed's haplotype carried by two thirds of the reads or by one third (the minority);
  (b) a window at column 1,500 where every read carries its own variant: a di- or tri-nucleotide repeat whose copy number is drawn per
      read from 8..30, 35..60 or 8..60, or substitutions of its own in a window of 150 to 300 bases at 5, 8 or 15 in a hundred (the
      last: one region over the window, every candidate beyond 100 bases, the ranking's tail pass), with 6, 9 and 30 reads, so that
      no string repeats three times.
A pile the reference answers with a status is left out and printed.

Layout and recipe: those of make_rank_piles_golden.py.  The file holds data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_edge_piles_golden as E  # noqa: E402
import make_rank_piles_golden as R  # noqa: E402
import refpipe  # noqa: E402

OUT = os.path.join(HERE, "hifi_phase_piles.npz")
L = 3000


def _other_haplotype(codes, sites):
    """A copy with a difference every 300 bases from column 150 on: by turns a substitution, an insertion of 1..4 bases, a homopolymer
    of five (sites 'all'); a substitution at each (sites 'snp'); an insertion or a homopolymer at each (sites 'indel')."""
    parts, at = [], 0
    for n, pos in enumerate(range(150, codes.size - 20, 300)):
        kind = n % 3 if sites == "all" else 0 if sites == "snp" else 1 + n % 2
        parts.append(codes[at:pos])
        at = pos
        if kind == 0:
            parts.append(np.asarray([(codes[pos] + 1) & 3], dtype=np.uint8))
            at = pos + 1
        elif kind == 1:
            parts.append(np.resize(np.asarray([2, 0, 3, 1], dtype=np.uint8), 1 + n % 4))
        else:
            parts.append(np.full(5, codes[pos], dtype=np.uint8))
    return np.concatenate(parts + [codes[at:]])


def hap_pile(sites, n_reads, minority, seed):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 4, L, dtype=np.uint8)
    s = E.noisy(truth, "hifi", seed + 1)
    other = _other_haplotype(truth, sites)
    seqs, st, en = [E.asc(s)], [0], [s.size - 1]
    for i in range(n_reads):
        with_seed = (i % 3 == 0) if minority else (i % 3 != 0)
        seqs.append(E.asc(E.noisy(truth if with_seed else other, "hifi", seed * 1000 + i)))
        st.append(0)
        en.append(s.size - 1)
    return E.make_case("phase/hap/%s/%s/reads%d" % (sites, "minority" if minority else "majority", n_reads), seqs, st, en, "hifi")


def own_pile(unit, lo, hi, n_reads, seed, rep=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 4, L, dtype=np.uint8)
    u = np.asarray(unit, dtype=np.uint8)

    def with_copies(k):
        return np.concatenate([truth[:1500], np.tile(u, k), truth[1500:]])

    s = E.noisy(with_copies((lo + hi) // 2), "hifi", seed + 1)
    seqs, st, en = [E.asc(s)], [0], [s.size - 1]
    for i in range(n_reads):
        seqs.append(E.asc(E.noisy(with_copies(int(rng.integers(lo, hi + 1))), "hifi", seed * 1000 + i)))
        st.append(0)
        en.append(s.size - 1)
    return E.make_case("phase/own/unit%d/copies%d-%d/reads%d/%d" % (len(unit), lo, hi, n_reads, rep), seqs, st, en, "hifi")


def scatter_pile(width, rate, n_reads, seed):
    """Every read, and the seed, with substitutions of its own at `rate` inside the window [1500, 1500 + width)."""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 4, L, dtype=np.uint8)

    def own():
        c = truth.copy()
        hit = 1500 + np.nonzero(rng.random(width) < rate)[0]
        c[hit] = (c[hit] + rng.integers(1, 4, hit.size)) & 3
        return c

    s = E.noisy(own(), "hifi", seed + 1)
    seqs, st, en = [E.asc(s)], [0], [s.size - 1]
    for i in range(n_reads):
        seqs.append(E.asc(E.noisy(own(), "hifi", seed * 1000 + i)))
        st.append(0)
        en.append(s.size - 1)
    return E.make_case("phase/own/scatter/width%d/rate%d/reads%d" % (width, int(rate * 100), n_reads), seqs, st, en, "hifi")


def cases():
    out = []
    for k, (sites, n, minority) in enumerate((("all", 9, False), ("all", 9, True), ("all", 30, False), ("all", 30, True),
                                              ("snp", 9, False), ("snp", 30, True), ("indel", 9, False), ("indel", 30, False),
                                              ("indel", 30, True))):
        out.append(hap_pile(sites, n, minority, 7100 + 10 * k))
    k = 0
    for unit, lo, hi in (((0, 3), 8, 30), ((0, 3, 2), 8, 30), ((0, 3, 2), 35, 60), ((1, 2), 8, 60)):
        for n in (6, 9, 30):
            for rep in range(1 if n > 9 else 2):   # (the small piles twice: they are what the interpreter can run quickly)
                out.append(own_pile(unit, lo, hi, n, 7300 + 10 * k, rep))
                k += 1
    # a window where every read has substitutions of its own: one region over the window, every candidate beyond 100 bases
    for width, rate in ((150, 0.08), (300, 0.05), (160, 0.15)):
        for n in (6, 9, 30):
            out.append(scatter_pile(width, rate, n, 7800 + width + n))
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    return [c for c in out if not only or only[0] in c["tag"]]


def main():
    assert refpipe.have_ref("nextcorrect.so"), "build the reference first: make -C oracle ref"
    R.cases = cases      # (make_rank_piles_golden.build_arrays asks its module for the cases: the same layout, these piles)
    arrays = R.build_arrays()
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
    # what the rule meets, pile by pile: the counters of ndgpu_phase_stats on the interpreted library with NDGPU_PHASE_DEVICE=1
    import phase_util
    r = phase_util.child("simt", "piles_each", "phase", "all", NDGPU_PHASE_DEVICE="1")
    tot = dict(kind=[0, 0, 0, 0], tail_passes=0, seed_lower=0, pass2_piles=0)
    for tag, st in r["each"]:
        print("  %-44s regions %3d: dropped %d, seed %d (%d lower), ranked %d (%d tail) | pass 2: %d"
              % (tag, st["regions"], st["kind"][1], st["kind"][2], st["seed_lower"], st["kind"][3], st["tail_passes"], st["pass2_piles"]))
        for k in range(4):
            tot["kind"][k] += st["kind"][k]
        for k in ("tail_passes", "seed_lower", "pass2_piles"):
            tot[k] += st[k]
    print("in all:", tot, "wrong:", r["bad"])
    assert r["bad"] == []
    assert tot["tail_passes"] > 0 and tot["kind"][3] > tot["tail_passes"], "RANKED with and without the tail pass"
    assert tot["seed_lower"] > 0 and tot["kind"][2] > tot["seed_lower"], "SEED with and without lower"
    assert tot["pass2_piles"] > 0, "pass 2"
    # (DROPPED is not asserted: no pile built here reaches it through nextCorrect -- repeats whose copy numbers form a geometric row
    # end as ranked regions, an insertion beyond 100 bases is answered with a status -- see DESIGN.md; the restatement covers it)


if __name__ == "__main__":
    main()
