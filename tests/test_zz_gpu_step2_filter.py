"""K23, the step-2 writer on the device (ndgpu_s2_filter_encode_flags, bit 1): filter_ovl's verdicts, the 10-field bytes, the
encoder's `prev` and the `.bl` table of streams fed through the device path, alone or alternating with the host loop on one state.

Expected values never come from the device path: verdicts and `.bl` text are the oracle library's (nd_s2_filter / nd_s2_out_bl,
pinned to the compiled reference by tests/test_oracle.py), bytes and `prev` are the host loop's (flags bit 0, pinned to the
reference's files by the golden command-line runs).  tests/test_simt_step2_filter.py runs the same bodies under the interpreter.

The command-line test at the end runs every golden `--step 2` case with NDGPU_S2_DEVICE=1; it is GPU only (the k = 17 cases take
20-30 s each under the interpreter), the interpreter file runs the two cases that take seconds there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu

F = ("rev", "qname", "qs", "qe", "qlen", "tname", "ts", "te", "tlen", "identity")


class S2(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in F]


def _bind_oracle(o):
    o.nd_s2_new.restype = C.c_void_p
    o.nd_s2_free.argtypes = [C.c_void_p]
    o.nd_s2_filter.argtypes = [C.c_void_p, C.POINTER(S2), C.c_int32, C.c_int32]
    o.nd_s2_out_bl.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    o.nd_s2_out_bl.restype = C.c_int64
    return o


def to_array(recs):
    from nextdenovo_amd import overlap
    a = np.zeros(len(recs), dtype=overlap.REC10)
    for k, name in enumerate(F):
        a[name] = [r[k] for r in recs]
    return a


_ORACLE = {}


def oracle_of(o, key, recs, h1, h2):
    """Verdicts and `.bl` text of the whole stream, computed once per stream (key) and shared."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    _bind_oracle(o)
    st = o.nd_s2_new()
    try:
        v = np.array([o.nd_s2_filter(st, C.byref(S2(*r)), h1, h2) for r in recs], dtype=bool)
        buf = C.create_string_buffer(4096 + 64 * 2 * len(recs) + 48 * len(recs))
        n = o.nd_s2_out_bl(st, buf, len(buf))
        assert n >= 0
        res = (v, buf.raw[:n].decode())
    finally:
        o.nd_s2_free(st)
    if key is not None:
        _ORACLE[key] = res
    return res


def check_stream(o, recs, h1, h2, plan, prev0=(0, 0), key=None):
    """Feed recs[a:b] call by call -- plan = [(a, b, device), ...] covering the stream in order -- to one state and compare every
    call's verdicts with the oracle's and its bytes and `prev` with the host loop's over the same calls, then the `.bl` text."""
    from nextdenovo_amd import overlap
    want_v, want_bl = oracle_of(o, key, recs, h1, h2)
    arr = to_array(recs)
    with overlap.Step2Filter() as flt, overlap.Step2Filter() as host:
        flt.prev[:] = prev0
        host.prev[:] = prev0
        for a, b, device in plan:
            want_b, host_v = host.feed(arr[a:b], h1, h2, want_verdicts=True, device=False)
            got_b, got_v = flt.feed(arr[a:b], h1, h2, want_verdicts=True, device=device)
            assert np.array_equal(host_v, want_v[a:b]), (a, b)
            assert np.array_equal(got_v, want_v[a:b]), (a, b, np.flatnonzero(got_v != want_v[a:b])[:5])
            assert got_b == want_b, (a, b)
            assert tuple(flt.prev) == tuple(host.prev), (a, b)
        assert host.bl() == want_bl
        got_bl = flt.bl()
    assert got_bl == want_bl, [(x, y) for x, y in zip(got_bl.splitlines(), want_bl.splitlines()) if x != y][:3]
    return want_v


def fresh_stats():
    from nextdenovo_amd import overlap
    overlap.s2_reset_stats()


def stats():
    from nextdenovo_amd import overlap
    return overlap.s2_stats()


def assert_on_device(min_calls=1, max_rounds=16):
    st = stats()
    assert st["device_calls"] >= min_calls, st
    assert st["declined"] == [0] * 6, st
    assert st["max_rounds"] <= max_rounds, st
    return st


# ---- seeded random streams: the generator of test_oracle.py::test_step2_filter_and_bl_vs_reference with a seventh kind, both reads
# covered end to end, for a fraction of the records
PARAMS = [(1, 40, 1500, 500, 50), (2, 300, 6000, 5000, 500), (3, 9, 400, 200, 20), (4, 1200, 9000, 800, 100)]
FRACTIONS = [0.0, 0.1, 0.5]
_STREAMS = {}


def random_stream(seed, n_reads, n_ovl, han1, han2, p_double):
    key = (seed, n_reads, n_ovl, han1, han2, p_double)
    if key in _STREAMS:
        return _STREAMS[key]
    rng = np.random.default_rng(seed)
    names = rng.permutation(50000)[:n_reads] + 1
    lens = rng.integers(max(3 * han1 // 2, 300), 8 * han1, n_reads)

    def piece(L, where):
        if where == "lo":
            s = int(rng.integers(0, han1 + han1 // 2)); e = int(min(L, s + rng.integers(han1 // 2, L)))
        elif where == "hi":
            e = L - int(rng.integers(0, han1 + han1 // 2)); s = int(max(0, e - rng.integers(han1 // 2, L)))
        elif where == "all":
            s = int(rng.integers(0, han2 * 2)); e = L - int(rng.integers(0, han2 * 2))
        else:
            s = int(rng.integers(0, L // 2)); e = int(min(L, s + rng.integers(han2 + 21, L // 2 + han2 + 22)))
        if e - s < 21:
            s, e = 0, min(L, 40)
        return s, e
    recs = []
    for it in range(n_ovl):
        a, b = rng.choice(n_reads, 2, replace=False)
        ql, tl = int(lens[a]), int(lens[b])
        kind = 6 if rng.random() < p_double else it % 6
        rev = int(rng.integers(0, 2))
        if kind == 0:
            (qs, qe), (ts, te) = (piece(ql, "lo"), piece(tl, "lo")) if rev else (piece(ql, "hi"), piece(tl, "lo"))
        elif kind == 1:
            (qs, qe), (ts, te) = (piece(ql, "hi"), piece(tl, "hi")) if rev else (piece(ql, "lo"), piece(tl, "hi"))
        elif kind == 2:
            (qs, qe), (ts, te) = piece(ql, "all"), piece(tl, "mid")
        elif kind == 3:
            (qs, qe), (ts, te) = piece(ql, "mid"), piece(tl, "all")
        elif kind == 6:
            (qs, qe), (ts, te) = piece(ql, "all"), piece(tl, "all")
        else:
            (qs, qe), (ts, te) = piece(ql, "mid"), piece(tl, "mid")
        recs.append((rev, int(names[a]), qs, qe, ql, int(names[b]), ts, te, tl, int(rng.integers(500, 10001))))
    _STREAMS[key] = recs
    return recs


def plan_of(n, way):
    if way == "one":
        return [(0, n, True)]
    if way == "ones":
        return [(i, i + 1, True) for i in range(n)]
    if way == "ones-300":   # (the interpreter's form of "ones" for the long streams: calls of 1 for 300 records, the rest in one call)
        return [(i, i + 1, True) for i in range(min(n, 300))] + ([(300, n, True)] if n > 300 else [])
    cuts = list(range(0, n, 257)) + [n]
    if way == "257":
        return [(a, b, True) for a, b in zip(cuts, cuts[1:])]
    return [(a, b, k % 2 == 1) for k, (a, b) in enumerate(zip(cuts, cuts[1:]))]   # "mixed": host and device calls alternate


def check_random(o, params, p_double, way):
    seed, n_reads, n_ovl, han1, han2 = params
    recs = random_stream(seed, n_reads, n_ovl, han1, han2, p_double)
    fresh_stats()
    v = check_stream(o, recs, han1, han2, plan_of(len(recs), way), key=("random", params, p_double))
    assert 0 < int(v.sum()) < len(recs)
    st = assert_on_device()
    print("random", params, p_double, way, "rounds", st["rounds"], "max_rounds", st["max_rounds"], "device_calls", st["device_calls"])


@pytest.mark.parametrize("way", ["one", "ones", "257", "mixed"])
@pytest.mark.parametrize("p_double", FRACTIONS)
@pytest.mark.parametrize("params", PARAMS, ids=["r40", "r300", "r9", "r1200"])
def test_random_streams(oracle_lib, params, p_double, way):
    check_random(oracle_lib, params, p_double, way)


# ---- directed streams
L0 = 20000


def dovetail(q, t, ide=9700, L=L0):   # the 3' end of q over the 5' end of t
    return (0, q, L - 6000, L - 100, L, t, 50, 5950, L, ide)


def contained(q, t, L=L0):            # q covered end to end by the middle of a long t
    return (0, q, 5, L - 5, L, t, 3000, 3000 + L - 10, 3 * L, 9000)


def internal(q, qs, qe, t, ts=None, L=100000):   # an overlap inside both reads
    ts = 30000 if ts is None else ts
    return (1, q, qs, qe, L, t, ts, ts + (qe - qs), L, 8000)


def check_record_counts(o, n):
    recs = random_stream(11, 12, 257, 500, 50, 0.1)[:n]
    fresh_stats()
    check_stream(o, recs, 500, 50, [(0, n, True)], prev0=(70000, 3))
    assert_on_device()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_record_counts_against_a_carried_prev(oracle_lib, n):
    check_record_counts(oracle_lib, n)


def check_one_read(o, k, as_target):
    """One read in k records (a segment inside a wavefront, one wavefront, over one, over a block): both end counters, the four
    maxima, the longest internal overlap (equal lengths: the first) and a long interval list."""
    rng = np.random.default_rng(100 + k)
    X, L, h1, h2 = 7, 30000, 2000, 300
    recs = []
    for j in range(k):
        other, kind = 1000 + j, j % 4
        ide = int(rng.integers(500, 10001))
        if kind == 0:     # X's 3' end over the other's 5' end
            g1, g2 = int(rng.integers(0, 600)), int(rng.integers(0, 600))
            x, y, rev = (L - g1 - int(rng.integers(1000, 9000)), L - g1), (g2, g2 + int(rng.integers(1000, 9000))), 0
            if as_target:   # (as the target the 3' end of X meets the 5' end of the query's reverse strand: rev, both 3' ends)
                y, rev = (L - g2 - (y[1] - y[0]), L - g2), 1
        elif kind == 1:   # X's 5' end
            g1, g2 = int(rng.integers(0, 600)), int(rng.integers(0, 600))
            x, y, rev = (g1, g1 + int(rng.integers(1000, 9000))), (g2, g2 + int(rng.integers(1000, 9000))), 1
        else:             # internal; every third pair of them as long as the one before
            s = int(rng.integers(3000, 15000))
            n = 4000 if j % 3 == 0 else int(rng.integers(100, 9000))
            x, y, rev = (s, s + n), (5000, 5000 + n), int(rng.integers(0, 2))
        r = (rev, X, x[0], x[1], L, other, y[0], y[1], L, ide)
        if as_target:
            r = (rev, other, y[0], y[1], L, X, x[0], x[1], L, ide)
        recs.append(r)
    fresh_stats()
    v = check_stream(o, recs, h1, h2, [(0, k, True)])
    assert k < 4 or 0 < int(v.sum()) < k
    assert_on_device()


@pytest.mark.parametrize("as_target", [False, True], ids=["query", "target"])
@pytest.mark.parametrize("k", [1, 2, 64, 65, 300])
def test_one_read_in_k_records(oracle_lib, k, as_target):
    check_one_read(oracle_lib, k, as_target)


def chain(k, L=L0):
    """Reads 1 .. k + 1; read 1 contained twice by outsiders, every other read once; link j = (query j, target j + 1, both covered end
    to end); then a dovetail per read against a fresh outsider.  In stream order link j kills read j + 1 -- the dead query j does not
    take the bump -- so no dovetail survives; one round of the fixed point knows only that read 1 is dead."""
    out = 1000
    recs = [contained(1, out), contained(1, out + 1)]
    recs += [contained(j, out + j) for j in range(2, k + 2)]
    recs += [(0, j, 7, L - 7, L, j + 1, 9, L - 9, L, 9500) for j in range(1, k + 1)]
    recs += [dovetail(j, out + 50 + j) for j in range(1, k + 2)]
    return recs


def check_chain(o, k, on_device, monkeypatch, cap=None):
    if cap is not None:
        monkeypatch.setenv("NDGPU_S2_MAX_ROUNDS", str(cap))
    recs = chain(k)
    fresh_stats()
    v = check_stream(o, recs, 2000, 500, [(0, len(recs), True)], key=("chain", k))
    assert not v[-(k + 1):].any() and not v.any()
    st = stats()
    if on_device:
        assert st["device_calls"] == 1 and st["declined"] == [0] * 6 and st["max_rounds"] >= k, st
    else:
        assert st["device_calls"] == 0 and st["declined"] == [0, 0, 0, 1, 0, 0], st


@pytest.mark.parametrize("k", [1, 5])
def test_chain_needs_as_many_rounds_as_it_has_links(oracle_lib, k, monkeypatch):
    monkeypatch.delenv("NDGPU_S2_MAX_ROUNDS", raising=False)
    check_chain(oracle_lib, k, True, monkeypatch)


def test_chain_of_40_declines_at_the_default_cap(oracle_lib, monkeypatch):
    monkeypatch.delenv("NDGPU_S2_MAX_ROUNDS", raising=False)
    check_chain(oracle_lib, 40, False, monkeypatch)


def test_chain_of_40_runs_with_a_cap_of_64(oracle_lib, monkeypatch):
    check_chain(oracle_lib, 40, True, monkeypatch, cap=64)


def check_decline(o, which, monkeypatch):
    """A stream the device must not compute: the same result through the host loop, its own counter, and the state good for a device call."""
    base = random_stream(12, 12, 200, 500, 50, 0.1)
    first, second = list(base[:100]), list(base[100:])
    if which == 0:
        first[40] = (0, 901, 100, 120, 4000, 902, 200, 240, 4000, 9000)      # a 20-base query span
    elif which == 1:
        r = first[40]
        first[40] = r[:9] + (40000,)
    fresh_stats()
    recs = first + second
    want_v, _ = oracle_of(o, None, recs, 500, 50)
    from nextdenovo_amd import overlap
    arr = to_array(recs)
    with overlap.Step2Filter() as flt, overlap.Step2Filter() as host:
        if which == 5:
            monkeypatch.setenv("NDGPU_S2_DECLINE", "1")
        b1, v1 = flt.feed(arr[:100], 500, 50, want_verdicts=True, device=True)
        monkeypatch.delenv("NDGPU_S2_DECLINE", raising=False)
        st = stats()
        assert st["device_calls"] == 0 and st["declined"] == [int(x == which) for x in range(6)], st
        b2, v2 = flt.feed(arr[100:], 500, 50, want_verdicts=True, device=True)
        st = stats()
        assert st["device_calls"] == 1 and sum(st["declined"]) == 1, st
        assert b1 == host.feed(arr[:100], 500, 50, device=False) and b2 == host.feed(arr[100:], 500, 50, device=False)
        assert tuple(flt.prev) == tuple(host.prev)
        assert np.array_equal(np.concatenate([v1, v2]), want_v)
        _, want_bl = oracle_of(o, None, recs, 500, 50)
        assert flt.bl() == want_bl


@pytest.mark.parametrize("which", [0, 1, 5], ids=["span-20", "identity-40000", "hook"])
def test_declined_calls_run_the_host_loop(oracle_lib, which, monkeypatch):
    check_decline(oracle_lib, which, monkeypatch)


def check_across_calls(o):
    # read 1: contained once in the first call, once more in the second -- its dovetail behind that is dropped, the one before kept
    a = [contained(1, 500), dovetail(2, 3)]
    b = [dovetail(1, 600), contained(1, 501), dovetail(1, 601), dovetail(2, 602)]
    # read 10 dead after the first call; read 11 contained once.  Second call: (query 10, target 11, both covered): the dead query
    # takes no bump, the target does and dies; its dovetail is dropped
    a += [contained(10, 510), contained(10, 511), contained(11, 512), dovetail(11, 610)]
    b += [(0, 10, 7, L0 - 7, L0, 11, 9, L0 - 9, L0, 9500), dovetail(11, 611), dovetail(12, 612)]
    recs = a + b
    for plan in ([(0, len(a), True), (len(a), len(recs), True)], [(0, len(a), False), (len(a), len(recs), True)]):
        fresh_stats()
        v = check_stream(o, recs, 2000, 500, plan, key="across")
        assert_on_device()
    kept = {i for i in range(len(recs)) if v[i]}
    assert kept == {1, 5, len(a) + 0, len(a) + 3, len(a) + 6}, kept


def test_state_carried_across_calls(oracle_lib):
    check_across_calls(oracle_lib)


UNIONS = {
    "nested": [(1000, 9000), (2000, 3000), (1500, 8999), (2500, 9000)],
    "touching": [(1000, 2000), (1980, 3000), (5000, 6000), (3980, 5020)],          # stored (s + 10, e - 10): 1990 == 1990 joins
    "one-apart": [(1000, 2000), (1981, 3000), (4981, 6000), (4000, 5000)],         # 1991 > 1990 stays apart
    "equal-starts": [(1000, 2000), (1000, 5000), (1000, 1500), (7000, 7100), (7000, 7050)],
    "seven": [(1000 * k, 1000 * k + 500) for k in (3, 1, 7, 5, 2, 6, 4)],
    "twelve": [(1000 * k, 1000 * k + 500) for k in (12, 3, 1, 7, 10, 5, 2, 9, 6, 4, 11, 8)],
    "twelve-then-bridge": [(1000 * k, 1000 * k + 500) for k in range(1, 13)] + [(1400, 12100)],
}


def check_union(o, name):
    recs = [internal(7, s, e, 2000 + j) for j, (s, e) in enumerate(UNIONS[name])]
    fresh_stats()
    for plan in ([(0, len(recs), True)], [(0, 2, True), (2, len(recs), True)], [(0, 3, False), (3, len(recs), True)]):
        check_stream(o, recs, 2000, 500, plan, key=("union", name))
    assert_on_device(min_calls=4)


@pytest.mark.parametrize("name", list(UNIONS))
def test_interval_union(oracle_lib, name):
    check_union(oracle_lib, name)


def check_encoder(o):
    """Kept records only (everything is a dovetail within maxhan1 = 2^31 - 1) except where a record is made to drop: names going up
    and down, both span orders, every field at every varint length it can have (the identity: 3 bytes, beyond is a decline)."""
    size = [1, 128, 16384, 1 << 21, 1 << 28]
    h1, h2 = (1 << 31) - 1, 0
    recs, q, t = [], 5, 1 << 30
    for k in range(5):
        for up in (0, 1):
            dq, dt, v = size[k], size[4 - k], size[k]
            q, t = (q + dq, t - dt) if up else (q - dq + 3 * size[k], t + dt + 1)
            qspan, tspan = (v + 40, 40 + size[(k + 2) % 5]) if up else (40 + size[(k + 1) % 5], v + 40)
            qs, ts = size[(k + up) % 5], size[(k + 3 + up) % 5]
            recs.append((up, q, qs, qs + qspan, qs + qspan + size[(k + 1) % 5], t, ts, ts + tspan, ts + tspan + size[k], min(size[k], 16384) + k))
    # the same names three times with the middle record dropped (an internal overlap beyond a small maxhan1 would be; here: a contained
    # query), then a third read: the lengths are written against the previous KEPT record
    recs2 = [dovetail(40, 41), contained(50, 51), dovetail(50, 41), dovetail(40, 41), contained(40, 52), dovetail(40, 41), dovetail(40, 41, ide=1)]
    fresh_stats()
    v = check_stream(o, recs, h1, h2, [(0, len(recs), True)], prev0=(3, 1 << 31))
    assert v.all()
    for cut in (1, 4, 9):
        check_stream(o, recs, h1, h2, [(0, cut, True), (cut, len(recs), True)], prev0=(3, 1 << 31))
    v = check_stream(o, recs2, 2000, 500, [(0, len(recs2), True)], prev0=(50, 41))
    assert list(v) == [True, False, True, True, False, True, True]
    check_stream(o, recs2, 2000, 500, [(0, 2, True), (2, 5, True), (5, 7, True)], prev0=(50, 41))
    assert_on_device()


def test_encoder_fields_names_and_dropped_records(oracle_lib):
    check_encoder(oracle_lib)


def check_flags():
    from nextdenovo_amd import overlap
    lib = overlap.load()
    arr = to_array([dovetail(1, 2)])
    with overlap.Step2Filter() as flt:
        for flags in (3, 4, 6, 1 << 20):
            out = C.c_void_p(0x1234)
            prev = np.array([9, 8], dtype=np.uint32)
            kept = np.full(1, 77, dtype=np.uint8)
            n = lib.ndgpu_s2_filter_encode_flags(flt.h, arr.ctypes.data_as(C.c_void_p), 1, 2000, 500, prev.ctypes.data_as(C.c_void_p), flags,
                                                 C.byref(out), kept.ctypes.data_as(C.c_void_p))
            assert n == -2 and out.value == 0x1234 and list(prev) == [9, 8] and kept[0] == 77
        assert flt.bl() == ""


def test_bad_flags_write_nothing():
    check_flags()


# ---- the command
def check_command(tag, argv, tmp_path, monkeypatch):
    import test_zz_gpu_step2 as S2
    monkeypatch.setenv("NDGPU_S2_DEVICE", "1")
    fresh_stats()
    S2.run_case(tag, argv, tmp_path)
    st = stats()
    print("step2 command", tag, "declined", st["declined"], "max_rounds", st["max_rounds"], "device_calls", st["device_calls"], "calls", st["calls"])
    assert st["device_calls"] > 0, st


def _all_cases():
    from make_step2_golden import CASES, CASES_M1, CASES_M2, CASES_RECHAIN, CASES_THIN
    return CASES + CASES_M2 + CASES_M1 + CASES_RECHAIN + CASES_THIN


@pytest.mark.parametrize("tag,argv", _all_cases(), ids=[c[0] for c in _all_cases()])
def test_step2_command_with_the_device_writer(tag, argv, tmp_path, monkeypatch):
    check_command(tag, argv, tmp_path, monkeypatch)
