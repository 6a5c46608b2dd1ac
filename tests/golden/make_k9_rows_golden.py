#!/usr/bin/env python
"""Generate tests/golden/k9_rows.npz: piles for the row routine of the link counter's compact path, and the REAL reference's
answers.

    python tests/golden/make_k9_rows_golden.py            # writes the fixture
    python tests/golden/make_k9_rows_golden.py --check    # builds everything again and compares with the committed arrays

(needs what make_edge_piles_golden.py needs: the reference compiled into oracle/_ref, the oracle library, tests/simt.)

On the compact path (count_links_kernel, nextdenovo_amd/csrc/msa_kernels.hip: k9_row) the at most 64 reads that reach a block of
32 columns sit one per lane, and the links of a cell row -- six cells: A, T, G, C, gap, and one nobody uses -- are elected in one
pass over the lanes.  The six cells' link counts are bytes of one 64-bit word; one multiplication turns them into the cells'
offsets.  The piles here are small (a seed of 640 bases, at most 64 accepted reads, every block on the compact path) and made
for that routine.  Seeds hold no 'A' and the reads are copies of the seed with hand-placed edits, most of them runs of 'A', so
that the aligner has one way to place them (make_edge_piles_golden.py: craft_pile).

  fan     the seed and 63 reads over the whole seed: 64 lanes, all of them busy in every row.  The reads agree on the base of
          column 330 and differ in front of it: 48 carry an insertion of 1 .. 24 bases closed by 'A' or by another base, others a
          replaced base one or two columns before, a deletion of either or both, and some are plain copies or repeat another
          read's edit (links with counts above one).  The cell of that base holds more than 48 distinct links -- one byte counter
          near 64, the others of the row at zero or one, prefix sums with no carry to spare.
  spread  20 reads.  The aligner knows equal pairs, insertions and deletions only, so in row 0 of a column stand the seed's base
          and the gap, and every other symbol stands in an insertion row.  Behind column `c` (the first of a two-base run) reads
          insert 'A' (three reads), each base that is neither the run's nor 'A' (two reads, one read) and the run's own base (one
          read: it lands where the aligner slides it); two reads lose a base of the run.  Behind column c + 100 three reads insert
          'AAA', 'AA' and 'A': rows 1, 2, 3 carried by three, two and one read.  Three reads cover 560 bases of the seed only, so
          the blocks at either end have idle lanes between busy ones.
  thin    the seed and one read over its first 560 bases: blocks with two covering reads and blocks with one.

min_cov_base is 1 in all of them (the thin pile has no column deeper than two), so that one batched call takes the three.

Layout and fields: those of edge_piles.npz (make_edge_piles_golden.py).  The file holds data only."""
import os
import pickle
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_edge_piles_golden as E  # noqa: E402  (puts the repository, tests/ and tests/simt on the path)

OUT = os.path.join(HERE, "k9_rows.npz")
L = 640
ARGS = dict(min_cov_base=1)
TABLES = re.compile(r"K9 tables: digest=([0-9a-f]{16}) cells=(\d+) links=(\d+) max_cell_len=(\d+)")


def edited(s, a, b, edits):
    """Columns a .. b of the seed with edits {column: ("del",) | ("sub", base) | ("ins", [bases behind the column])}."""
    out = []
    for t in range(a, b + 1):
        e = edits.get(t, ("keep",))
        if e[0] == "keep":
            out.append(s[t])
        elif e[0] == "sub":
            out.append(e[1])
        elif e[0] == "ins":
            out.append(s[t])
            out.extend(e[1])
        else:
            assert e[0] == "del"
    return E.asc(np.asarray(out, dtype=np.uint8))


def pile(tag, s, reads):
    """reads: [(a, b, edits)]"""
    seqs, st, en = [E.asc(s)], [0], [L - 1]
    for a, b, edits in reads:
        seqs.append(edited(s, a, b, edits))
        st.append(a)
        en.append(b)
    return E.make_case(tag, seqs, st, en, **ARGS)


def tables(c):
    """The K9 tables line (digest, cells, links, longest cell) of the interpreted library's first attempt on the pile."""
    with tempfile.TemporaryDirectory() as wd:
        a, b = os.path.join(wd, "in.pkl"), os.path.join(wd, "out.pkl")
        with open(a, "wb") as f:
            pickle.dump({k: v for k, v in c.items() if k != "ref"}, f)
        env = {k: v for k, v in os.environ.items() if not k.startswith("NDGPU_")}
        env.update(NDGPU_TRACE="1", NDGPU_CONTEXTS="1", NDGPU_K9_DIGEST="1")
        code = E._TRACE_CHILD % (E.ROOT, os.path.join(E.ROOT, "tests"), os.path.join(E.ROOT, "tests", "simt"))
        r = subprocess.run([sys.executable, "-c", code, a, b], env=env, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        m = TABLES.search(r.stderr)
        assert m, r.stderr[-2000:]
        return m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))


def fan_family(live):
    s = np.random.default_rng(311).integers(1, 4, L, dtype=np.uint8)
    col = 330
    other = next(x for x in (1, 2, 3) if x != s[col - 1] and x != s[col])
    reads = []
    for i in range(48):
        ins = [0] * (1 + i // 2)
        if i % 2:
            ins[-1] = other
        reads.append((0, L - 1, {col - 1: ("ins", ins)}))
    reads.append((0, L - 1, {col - 1: ("sub", 0)}))
    reads.append((0, L - 1, {col - 2: ("sub", 0)}))
    reads += [(0, L - 1, {col - 1: ("del",)})] * 3
    reads.append((0, L - 1, {col - 2: ("del",)}))
    reads.append((0, L - 1, {col - 1: ("del",), col - 2: ("del",)}))
    reads.append((0, L - 1, {col - 1: ("sub", 0), col - 2: ("sub", 0)}))
    reads += [(0, L - 1, {})] * 4
    reads += [(0, L - 1, {col - 1: ("ins", [0])})] * 3
    c = pile("fan", s, reads)
    live("fan: the seed and 63 reads, all accepted", len(c["seqs"]) == 64 and E.accepted_reads(c) == 64)
    t = tables(c)
    live("fan: a cell of the interpreted library's tables holds %d distinct links (48 or more)" % t[3], t[3] >= 48)
    live("fan: the reference answers with a sequence", E.answer(c)[0] > 4)
    return [c]


def spread_family(live):
    s = np.random.default_rng(321).integers(1, 4, L, dtype=np.uint8)
    c0 = next(t for t in range(200, 300) if s[t] == s[t + 1] and s[t - 1] != s[t] and s[t + 2] != s[t])
    o1, o2 = [x for x in (1, 2, 3) if x != s[c0]]
    c1 = c0 + 100
    reads = [(0, L - 1, {})] * 4 + [(0, L - 1, {c0: ("del",)})] * 2
    reads += [(0, L - 1, {c0: ("ins", [0])})] * 3 + [(0, L - 1, {c0: ("ins", [o1])})] * 2
    reads += [(0, L - 1, {c0: ("ins", [o2])}), (0, L - 1, {c0: ("ins", [s[c0]])})]
    reads += [(0, L - 1, {c1: ("ins", [0] * n)}) for n in (3, 2, 1)]
    reads += [(0, 559, {}), (40, 599, {}), (80, L - 1, {})]
    c = pile("spread", s, reads)
    live("spread: 20 records, all accepted", len(c["seqs"]) == 20 and E.accepted_reads(c) == 20)
    live("spread: the reference answers with a sequence", E.answer(c)[0] > 4)
    return [c]


def thin_family(live):
    s = np.random.default_rng(331).integers(1, 4, L, dtype=np.uint8)
    c = pile("thin", s, [(0, 559, {300: ("ins", [0])})])
    live("thin: two accepted reads", len(c["seqs"]) == 2 and E.accepted_reads(c) == 2)
    live("thin: the reference answers with a sequence", E.answer(c)[0] > 4)
    return [c]


def main():
    assert E.refpipe.have_ref("nextcorrect.so"), "build the reference first: make -C oracle ref"
    E.FAMILIES = [("fan", fan_family), ("spread", spread_family), ("thin", thin_family)]
    arrays, report, checks = E.build_arrays()
    print("\n".join(report))
    failed = [w for w, ok in checks if not ok]
    assert not failed, "live checks failed: %s" % failed
    assert arrays["died"].size == 0
    assert all(int(x) > 4 for x in arrays["exp_len"]), "every pile's reference answer is a consensus"
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
