"""ctypes binding of libndgpu_nextcorrect.so -- the host-side mirror of the reference's
Python<->C boundary (lib/nextcorrect.py:19-24,56-90): same struct, same argument order,
same return convention (len, identity, sequence)."""
from __future__ import annotations

import ctypes as C
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")  # one hardware queue per device context (read when HIP initialises)

from . import build as _build

_LIB = None
_BIG = C.c_char * (1 << 30)   # (one array type for every record's view; never instantiated over memory it does not own)


class ConsensusTrimed(C.Structure):
    # lib/nextcorrect.py:19-24
    _fields_ = [("len", C.c_uint), ("identity", C.c_float), ("seq", C.c_void_p)]


class PoaJob(C.Structure):
    # ndgpu_poa_job
    _fields_ = [("seqs", C.POINTER(C.c_char_p)), ("len", C.POINTER(C.c_uint16)), ("seq_count", C.c_int32)]


class RankJob(C.Structure):
    # ndgpu_rank_job
    _fields_ = [("seqs", C.POINTER(C.c_char_p)), ("len", C.POINTER(C.c_uint16)), ("seq_count", C.c_int32)]


class RankResult(C.Structure):
    # ndgpu_rank_result
    _fields_ = [("order", C.c_uint8 * 40), ("kscore", C.c_uint16 * 40), ("tail", C.c_int32)]


class WalkStep(C.Structure):
    # ndgpu_walk_step
    _fields_ = [("t_pos", C.c_int32), ("link", C.c_uint16), ("cov", C.c_uint16), ("base", C.c_uint8), ("pad_", C.c_uint8 * 3)]


class CnsJob(C.Structure):
    # ndgpu_cns_job
    _fields_ = [("steps", C.c_void_p), ("n", C.c_uint32), ("min_cov", C.c_int32), ("lq_max_len", C.c_uint32),
                ("min_error_corrected_ratio", C.c_float)]


class CnsResult(C.Structure):
    # ndgpu_cns_result
    _fields_ = [("len", C.c_uint32), ("uncorrected_len", C.c_uint32), ("lstrip", C.c_uint32), ("rstrip", C.c_uint32),
                ("lqseq_total_length", C.c_uint32), ("ok", C.c_int32), ("n_regions", C.c_uint32), ("pad_", C.c_uint32),
                ("base_off", C.c_uint64), ("region_off", C.c_uint64)]


class CnsWalkJob(C.Structure):
    # ndgpu_cns_walk_job
    _fields_ = [("steps", C.c_void_p), ("n", C.c_uint32), ("min_cov", C.c_int32), ("lq_max_len", C.c_uint32),
                ("min_error_corrected_ratio", C.c_float), ("mode", C.c_int32), ("seed_len", C.c_uint32), ("seed", C.c_char_p)]


class CnsWalkResult(C.Structure):
    # ndgpu_cns_walk_result
    _fields_ = [("len", C.c_uint32), ("uncorrected_len", C.c_uint32), ("lstrip", C.c_uint32), ("rstrip", C.c_uint32),
                ("lqseq_total_length", C.c_uint32), ("ok", C.c_int32), ("n_regions", C.c_uint32), ("pad_", C.c_uint32),
                ("base_off", C.c_uint64), ("region_off", C.c_uint64), ("lq_total_len", C.c_uint32), ("seq_len", C.c_uint32),
                ("identity", C.c_float), ("pad2_", C.c_uint32), ("seq_off", C.c_uint64)]


class CnsModeStats(C.Structure):
    # ndgpu_cns_mode_stats
    _fields_ = [("hifi_jobs", C.c_uint64), ("hifi_declined", C.c_uint64), ("hifi_regions", C.c_uint64), ("fast_jobs", C.c_uint64),
                ("fast_declined", C.c_uint64), ("launches", C.c_uint64), ("ms", C.c_double), ("d2h_bytes", C.c_uint64)]


class SpliceRegion(C.Structure):
    # ndgpu_splice_region
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("len", C.c_int32), ("sudoseed_len", C.c_uint32), ("sudoseed", C.c_char_p)]


class SpliceJob(C.Structure):
    # ndgpu_splice_job
    _fields_ = [("words", C.c_void_p), ("n_words", C.c_uint32), ("lstrip", C.c_uint32), ("rstrip", C.c_uint32), ("n_regions", C.c_uint32),
                ("regions", C.POINTER(SpliceRegion)), ("read_type", C.c_int32), ("pad_", C.c_uint32)]


class SpliceResult(C.Structure):
    # ndgpu_splice_result
    _fields_ = [("len", C.c_uint32), ("lq_total_len", C.c_uint32), ("identity", C.c_float), ("out_len", C.c_uint32), ("lq_m", C.c_uint32),
                ("hq_m", C.c_uint32), ("lq_i", C.c_int32), ("clip_s", C.c_int32), ("clip_e", C.c_int32), ("seq_len", C.c_uint32),
                ("seq_off", C.c_uint64)]


class SpliceStats(C.Structure):
    # ndgpu_splice_stats
    _fields_ = [("jobs", C.c_uint64), ("declined", C.c_uint64), ("launches", C.c_uint64), ("h2d_bytes", C.c_uint64),
                ("d2h_bytes", C.c_uint64), ("trimmed", C.c_uint64), ("ms", C.c_double)]


class PhaseRegionIn(C.Structure):
    # ndgpu_phase_region_in
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_cand", C.c_int32), ("pad_", C.c_uint32), ("seqs", C.POINTER(C.c_char_p)),
                ("len", C.POINTER(C.c_uint16)), ("src", C.POINTER(C.c_uint16))]


class PhaseJob(C.Structure):
    # ndgpu_phase_job
    _fields_ = [("n_aligned", C.c_uint32), ("n_regions", C.c_uint32), ("regions", C.POINTER(PhaseRegionIn))]


class PhaseRegion(C.Structure):
    # ndgpu_phase_region
    _fields_ = [("kind", C.c_uint8), ("lower", C.c_uint8), ("indexs", C.c_uint8), ("tail", C.c_uint8), ("n", C.c_int16),
                ("seed", C.c_uint8), ("seed_pos", C.c_uint8), ("perm", C.c_uint8 * 40), ("kscore", C.c_uint16 * 40)]


class PhasePile(C.Structure):
    # ndgpu_phase_pile
    _fields_ = [("has_heter", C.c_uint8), ("pass2", C.c_uint8), ("declined", C.c_uint8), ("pad_", C.c_uint8)]


class PhaseStats(C.Structure):
    # ndgpu_phase_stats
    _fields_ = [("piles", C.c_uint64), ("regions", C.c_uint64), ("kind", C.c_uint64 * 4), ("pass2_piles", C.c_uint64),
                ("tail_passes", C.c_uint64), ("declined", C.c_uint64 * 5), ("launches", C.c_uint64), ("ms", C.c_double),
                ("d2h_record_bytes", C.c_uint64), ("d2h_string_bytes", C.c_uint64), ("seed_lower", C.c_uint64)]


class AlnJob(C.Structure):
    # ndgpu_aln_job
    _fields_ = [("q", C.c_char_p), ("q_len", C.c_int32), ("t", C.c_char_p), ("t_len", C.c_int32), ("hq", C.c_int32)]


class AlnDbJob(C.Structure):
    # ndgpu_aln_dbjob (ends inclusive)
    _fields_ = [("q_read", C.c_uint32), ("q_start", C.c_uint32), ("q_end", C.c_uint32), ("q_rev", C.c_uint32),
                ("t_read", C.c_uint32), ("t_start", C.c_uint32), ("t_end", C.c_uint32), ("t_rev", C.c_uint32), ("hq", C.c_int32)]


class AlnResult(C.Structure):
    # ndgpu_aln_result
    _fields_ = [("status", C.c_int32), ("aln_len", C.c_uint32), ("q_used", C.c_uint32), ("t_used", C.c_uint32),
                ("n_match", C.c_uint32), ("n_ins", C.c_uint32), ("n_del", C.c_uint32), ("max_gap_run", C.c_uint32),
                ("n_cigar", C.c_uint32), ("cigar_off", C.c_uint64)]


PILES_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint32), C.c_int)   # ndgpu_piles_done_fn


class Stats(C.Structure):
    _fields_ = [("tasks", C.c_uint64), ("wide_tasks", C.c_uint64), ("cells", C.c_uint64), ("d_steps", C.c_uint64),
                ("trace_bits", C.c_uint64), ("columns", C.c_uint64), ("pool_bases", C.c_uint64), ("seq_bases", C.c_uint64),
                ("max_band", C.c_uint32), ("forward_launches", C.c_uint32), ("forward_ms", C.c_double),
                ("traceback_ms", C.c_double), ("tags_ms", C.c_double), ("links_ms", C.c_double),
                ("score_ms", C.c_double), ("extract_ms", C.c_double), ("piles", C.c_uint64), ("tags", C.c_uint64),
                ("cells_msa", C.c_uint64), ("path_items", C.c_uint64), ("links", C.c_uint64),
                ("score_launches", C.c_uint64), ("backtrack_ms", C.c_double), ("score_segments", C.c_uint64),
                ("score_repairs", C.c_uint64), ("score_slow_piles", C.c_uint64), ("trace_words", C.c_uint64), ("lq_rounds", C.c_uint64), ("lq_declined", C.c_uint64),
                ("lq_ms", C.c_double), ("allocs", C.c_uint64), ("alloc_ms", C.c_double), ("level_allocs", C.c_uint64), ("level_ms", C.c_double),
                ("traceback_launches", C.c_uint64), ("lq_launches", C.c_uint64), ("lq_columns", C.c_uint64), ("lq_aln_columns", C.c_uint64),
                ("lq_bases", C.c_uint64), ("lq_out", C.c_uint64), ("lq_jobs", C.c_uint64), ("lq_repairs", C.c_uint64),
                ("tb_tasks", C.c_uint64), ("tb_walkers", C.c_uint64), ("tb_fallbacks", C.c_uint64),
                ("poa_jobs", C.c_uint64), ("poa_declined", C.c_uint64), ("poa_rounds", C.c_uint64), ("poa_launches", C.c_uint64),
                ("poa_cells", C.c_uint64), ("poa_ms", C.c_double),
                ("rank_jobs", C.c_uint64), ("rank_tail", C.c_uint64), ("rank_launches", C.c_uint64), ("rank_ms", C.c_double),
                ("aln_batch_jobs", C.c_uint64), ("aln_batch_launches", C.c_uint64), ("aln_batch_runs", C.c_uint64),
                ("aln_batch_ms", C.c_double),
                ("poa_resident_jobs", C.c_uint64), ("poa_resident_declined", C.c_uint64), ("poa_graph_launches", C.c_uint64),
                ("poa_graph_ms", C.c_double), ("poa_h2d_bytes", C.c_uint64), ("poa_d2h_bytes", C.c_uint64),
                ("cns_jobs", C.c_uint64), ("cns_declined", C.c_uint64), ("cns_launches", C.c_uint64), ("cns_regions", C.c_uint64),
                ("cns_ms", C.c_double), ("cns_d2h_bytes", C.c_uint64), ("walk_d2h_bytes", C.c_uint64)]


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """Load the native library.  Raises (never falls back to a CPU path) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError("libndgpu_nextcorrect.so is not built; run `python -m nextdenovo_amd.build`")
        _build.build()
    _LIB = _bind(C.CDLL(path))
    return _LIB


def _bind(lib):
    """Argument / result types of the entry points declared in include/ndgpu_nextcorrect.h."""
    lib.nextCorrect.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.c_uint, C.c_uint,
                                C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_uint, C.c_uint, C.c_int]
    lib.nextCorrect.restype = C.POINTER(ConsensusTrimed)
    lib.free_consensus_trimed.argtypes = [C.POINTER(ConsensusTrimed)]
    lib.ndgpu_correct_batch.argtypes = [C.c_int, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_uint)),
                                        C.POINTER(C.POINTER(C.c_uint)), C.POINTER(C.c_uint), C.POINTER(C.c_uint),
                                        C.POINTER(C.c_uint), C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_uint,
                                        C.c_uint, C.c_int, C.c_int, C.POINTER(C.POINTER(ConsensusTrimed))]
    lib.ndgpu_correct_batch.restype = C.c_int
    lib.ndgpu_db_create.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ndgpu_db_create.restype = C.c_void_p
    lib.ndgpu_db_destroy.argtypes = [C.c_void_p]
    lib.ndgpu_correct_piles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                        C.c_uint, C.c_float, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                        C.POINTER(C.POINTER(ConsensusTrimed))]
    lib.ndgpu_correct_piles.restype = C.c_int
    lib.ndgpu_correct_piles_stream.argtypes = lib.ndgpu_correct_piles.argtypes + [PILES_DONE_FN, C.c_void_p]
    lib.ndgpu_correct_piles_stream.restype = C.c_int
    lib.ndgpu_write_records.argtypes = [C.POINTER(C.POINTER(ConsensusTrimed)), C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_uint32, C.c_double,
                                        C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    lib.ndgpu_write_records.restype = C.c_int
    lib.ndgpu_poa_batch.argtypes = [C.POINTER(PoaJob), C.c_int, C.POINTER(C.c_void_p)]
    lib.ndgpu_poa_batch.restype = C.c_int
    lib.ndgpu_poa_batch_flags.argtypes = [C.POINTER(PoaJob), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ndgpu_poa_batch_flags.restype = C.c_int
    lib.ndgpu_lq_rank_batch.argtypes = [C.POINTER(RankJob), C.c_int, C.c_int, C.POINTER(RankResult)]
    lib.ndgpu_lq_rank_batch.restype = C.c_int
    lib.ndgpu_cns_windows_batch.argtypes = [C.POINTER(CnsJob), C.c_int, C.c_int, C.POINTER(CnsResult), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p)]
    lib.ndgpu_cns_windows_batch.restype = C.c_int
    lib.ndgpu_cns_walk_batch.argtypes = [C.POINTER(CnsWalkJob), C.c_int, C.c_int, C.POINTER(CnsWalkResult), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.ndgpu_cns_walk_batch.restype = C.c_int
    lib.ndgpu_get_cns_mode_stats.argtypes = [C.POINTER(CnsModeStats)]
    lib.ndgpu_get_cns_mode_stats.restype = None
    lib.ndgpu_hifi_phase_batch.argtypes = [C.POINTER(PhaseJob), C.c_int, C.c_int, C.POINTER(PhaseRegion), C.POINTER(PhasePile)]
    lib.ndgpu_hifi_phase_batch.restype = C.c_int
    lib.ndgpu_get_phase_stats.argtypes = [C.POINTER(PhaseStats)]
    lib.ndgpu_get_phase_stats.restype = None
    lib.ndgpu_splice_batch.argtypes = [C.POINTER(SpliceJob), C.c_int, C.c_int, C.POINTER(SpliceResult), C.POINTER(C.c_void_p)]
    lib.ndgpu_splice_batch.restype = C.c_int
    lib.ndgpu_get_splice_stats.argtypes = [C.POINTER(SpliceStats)]
    lib.ndgpu_get_splice_stats.restype = None
    lib.ndgpu_align_batch.argtypes = [C.POINTER(AlnJob), C.c_int, C.c_int, C.POINTER(AlnResult), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.ndgpu_align_batch.restype = C.c_int
    lib.ndgpu_align_db_batch.argtypes = [C.c_void_p, C.POINTER(AlnDbJob)] + lib.ndgpu_align_batch.argtypes[1:]
    lib.ndgpu_align_db_batch.restype = C.c_int
    lib.ndgpu_get_stats.argtypes = [C.POINTER(Stats)]
    lib.ndgpu_reset_stats.argtypes = []
    lib.ndgpu_device_count.restype = C.c_int
    return lib


def _take(lib, r):
    ln = r.contents.len
    ide = r.contents.identity
    seq = C.string_at(r.contents.seq, ln) if ln > 4 else b""
    lib.free_consensus_trimed(r)
    return ln, ide, seq


def correct(seqs, aln_start, aln_end, max_aln_length, min_len_aln=500, max_cov_aln=130, min_cov_base=4,
            max_lq_length=10000, min_error_corrected_ratio=0.8, split=0, fast=0, read_type=1):
    """Mirror of lib/nextcorrect.py:72-90 `correct()`; returns (len, identity, sequence bytes)."""
    lib = load()
    n = len(seqs)
    c_seqs = (C.c_char_p * n)()
    c_seqs[:] = seqs
    st = (C.c_uint * n)(*aln_start)
    en = (C.c_uint * n)(*aln_end)
    r = lib.nextCorrect(c_seqs, st, en, n, max_aln_length, min_len_aln, max_cov_aln, min_cov_base, max_lq_length,
                        min_error_corrected_ratio, split, fast, read_type)
    return _take(lib, r)


def correct_batch(piles, min_len_aln=500, max_cov_aln=130, min_cov_base=4, min_error_corrected_ratio=0.8, split=0,
                  fast=0, read_type=1, host_threads=0):
    """piles: list of (seqs, aln_start, aln_end, max_aln_length, max_lq_length).
    Returns a list of (len, identity, sequence bytes) in pile order."""
    lib = load()
    n = len(piles)
    if n == 0:
        return []
    keep = []
    a_seqs = (C.POINTER(C.c_char_p) * n)()
    a_st = (C.POINTER(C.c_uint) * n)()
    a_en = (C.POINTER(C.c_uint) * n)()
    cnt = (C.c_uint * n)()
    mml = (C.c_uint * n)()
    mlq = (C.c_uint * n)()
    for i, (seqs, st, en, max_aln, max_lq) in enumerate(piles):
        k = len(seqs)
        cs = (C.c_char_p * k)()
        cs[:] = seqs
        s = (C.c_uint * k)(*st)
        e = (C.c_uint * k)(*en)
        keep.append((cs, s, e))
        a_seqs[i] = C.cast(cs, C.POINTER(C.c_char_p))
        a_st[i] = C.cast(s, C.POINTER(C.c_uint))
        a_en[i] = C.cast(e, C.POINTER(C.c_uint))
        cnt[i] = k
        mml[i] = max_aln
        mlq[i] = max_lq
    out = (C.POINTER(ConsensusTrimed) * n)()
    lib.ndgpu_correct_batch(n, a_seqs, a_st, a_en, cnt, mml, mlq, min_len_aln, max_cov_aln, min_cov_base,
                            min_error_corrected_ratio, split, fast, read_type, host_threads, out)
    return [_take(lib, out[i]) for i in range(n)]


class ReadDB:
    """Device-resident 2-bit read database (additive replacement for ovlseq.so's
    init_ovls/getseq, lib/nextcorrect.py:62-69).  words/word_off/lens as produced by
    synth.pack_db() or read from a reference .2bit file."""

    def __init__(self, words, word_off, lens):
        import numpy as np
        self._lib = load()
        self._words = np.ascontiguousarray(words, dtype=np.uint32)
        self._off = np.ascontiguousarray(word_off, dtype=np.uint64)
        self._len = np.ascontiguousarray(lens, dtype=np.uint32)
        self.n_reads = int(self._len.size)
        self._h = self._lib.ndgpu_db_create(self.n_reads, self._words.ctypes.data, self._off.ctypes.data,
                                            self._len.ctypes.data)
        if not self._h:
            raise MemoryError("ndgpu_db_create: the read DB does not fit the device memory")

    def close(self):
        if self._h:
            self._lib.ndgpu_db_destroy(self._h)
            self._h = None

    def correct_piles(self, recs, pile_off, min_len_aln=500, max_cov_aln=130, min_cov_base=4, max_lq_length=10000,
                      min_error_corrected_ratio=0.8, split=0, fast=0, read_type=1, host_threads=0, lengths_only=False, fasta=None, lib_wall=None):
        """fasta = (OUT, IDX, seed names, min_len_seed, min_error_corrected_ratio): the accepted records are written as
        lib/nextcorrect.py:236-260 writes them and [(len, identity)] comes back instead of the sequences."""
        import numpy as np
        recs = np.ascontiguousarray(recs, dtype=np.uint32)
        pile_off = np.ascontiguousarray(pile_off, dtype=np.uint64)
        n = int(pile_off.size) - 1
        out = (C.POINTER(ConsensusTrimed) * n)()
        import time
        t0 = time.perf_counter()
        if fasta is not None:
            # the records are handed over sub-batch by sub-batch, while the later ones are still on the device: the parent of
            # lib/nextcorrect.py:232-260 prints each seed as its worker returns it, in no particular order
            OUT, IDX, names, min_len_seed, min_ratio = fasta
            res = [None] * n
            state = {"pos": OUT.tell(), "err": None, "t": 0.0}
            # real files: the library formats and writes a sub-batch's records itself (ndgpu_write_records: one writev per 340
            # records, the bases straight from where it holds them); anything else that has a write(): the loop below, record by record
            try:
                fd_out, fd_idx = OUT.fileno(), (IDX.fileno() if IDX is not None else -1)
                OUT.flush()
                if IDX is not None:
                    IDX.flush()
            except (AttributeError, OSError, ValueError):
                fd_out = None
            if fd_out is not None:
                names32 = np.ascontiguousarray(names, dtype=np.uint32)
                lens, ides = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float32)
                pos = C.c_uint64(state["pos"])
                wr = self._lib.ndgpu_write_records

                def done(_user, ids, cnt):
                    tw = time.perf_counter()
                    if wr(out, ids, cnt, names32.ctypes.data, int(min_len_seed), float(min_ratio), fd_out, fd_idx, C.byref(pos),
                          lens.ctypes.data, ides.ctypes.data) != 0:
                        state["err"] = OSError("writing the corrected records failed")
                    state["t"] += time.perf_counter() - tw
            else:
                def done(_user, ids, cnt):
                    tw = time.perf_counter()
                    try:
                        self._write_records(out, [ids[k] for k in range(cnt)], res, state, OUT, IDX, names, min_len_seed, min_ratio)
                    except BaseException as e:  # noqa: BLE001  (an exception must not unwind through the C caller)
                        state["err"] = e
                    state["t"] += time.perf_counter() - tw

            cb = PILES_DONE_FN(done)
            rc = self._lib.ndgpu_correct_piles_stream(self._h, n, recs.ctypes.data, pile_off.ctypes.data, min_len_aln, max_cov_aln,
                                                      min_cov_base, max_lq_length, min_error_corrected_ratio, split, fast, read_type,
                                                      host_threads, out, cb, None)
            if state["err"] is not None or rc != 0:
                # records that were never handed over (the call failed, or a hand-over did): they are the caller's to free
                for i in range(n):
                    if out[i]:
                        self._lib.free_consensus_trimed(out[i])
                        out[i] = None
            if state["err"] is not None:
                raise state["err"]
        else:
            rc = self._lib.ndgpu_correct_piles(self._h, n, recs.ctypes.data, pile_off.ctypes.data, min_len_aln, max_cov_aln,
                                               min_cov_base, max_lq_length, min_error_corrected_ratio, split, fast, read_type,
                                               host_threads, out)
        if lib_wall is not None:   # (the library call, hand-over included when it streams; [1]: the time inside the hand-over)
            lib_wall[0] = time.perf_counter() - t0
            if len(lib_wall) > 1:
                lib_wall[1] = state["t"] if fasta is not None else 0.0
        if rc == -2:
            raise ValueError("ndgpu_correct_piles: an overlap record names a read or a window that is not in this read DB "
                             "(sorted.ovl and the .idx / .2bit files do not belong together?)")
        if rc != 0:
            raise RuntimeError("ndgpu_correct_piles failed (%d)" % rc)
        if fasta is not None:
            if fd_out is not None:
                OUT.seek(0, 2)   # (the descriptor moved under the file objects)
                if IDX is not None:
                    IDX.seek(0, 2)
                res = list(zip(lens.tolist(), ides.tolist()))
            return res
        if lengths_only:
            res = []
            for i in range(n):
                res.append((out[i].contents.len, out[i].contents.identity))
                self._lib.free_consensus_trimed(out[i])
            return res
        return [_take(self._lib, out[i]) for i in range(n)]

    def align_batch(self, jobs, hq=False, host=False, strings=False):
        """jobs: [(q_read, q_start, q_end, q_rev, t_read, t_start, t_end, t_rev[, hq])], ends inclusive -> what align_batch() returns,
        for windows of this DB (ndgpu_align_db_batch: nothing is packed or uploaded)."""
        arr = (AlnDbJob * max(1, len(jobs)))()
        for i, j in enumerate(jobs):
            arr[i] = AlnDbJob(*[int(x) for x in j[:8]], int(j[8]) if len(j) > 8 else int(bool(hq)))
        return _align_call(lambda *a: self._lib.ndgpu_align_db_batch(self._h, *a), "ndgpu_align_db_batch", arr, len(jobs), host, strings)

    def _write_records(self, out, ids, res, state, OUT, IDX, names, min_len_seed, min_ratio):
        """The output loop of lib/nextcorrect.py:236-260 (no -s) straight from the library's records: header, the bases as the
        library holds them (one copy, into the file), the .idx line.  OUT / IDX are binary files; res[i] = (len, identity)."""
        pos = state["pos"]
        free = self._lib.free_consensus_trimed
        for i in ids:
            c = out[i].contents
            ln, ide = c.len, c.identity
            name = int(names[i])
            if ln >= min_len_seed and ln > 4 and ide >= min_ratio:
                head = b">%d %d %f\n" % (name, ln, ide)
                OUT.write(head)
                OUT.write(memoryview(_BIG.from_address(c.seq))[:ln])   # (a view of the library's bytes: no copy before the file's)
                OUT.write(b"\n")
                pos += len(head) + ln + 1
                if IDX is not None:
                    IDX.write(b"%d\t%d\t%d\n" % (name, pos - ln - 1, ln))
            elif ln != 3 and IDX is not None:
                IDX.write(b"%d\t0\t0\n" % name)
            res[i] = (ln, ide)
            free(out[i])
            out[i] = None   # (handed over: nobody frees it again)
        state["pos"] = pos


class ExtJob(C.Structure):
    _fields_ = [("q", C.c_char_p), ("q_len", C.c_int32), ("t", C.c_char_p), ("t_len", C.c_int32), ("max_d", C.c_int32),
                ("band_size", C.c_int32), ("d_factor", C.c_float), ("kind", C.c_int32)]


class ExtResult(C.Structure):
    _fields_ = [("done", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("pos", C.c_uint32 * 6)]


EXT_KINDS = {"ide": 0, "alnpos": 1, "extend_fwd": 2, "extend_rev": 3}


def ext_batch(jobs):
    """jobs: [(kind, q bytes, t bytes, max_d, band_size, d_factor)] -> [(done, a, b, pos[6])] through ndgpu_ext_batch
    (the ide / alnpos / extend_fwd / extend_rev family of lib/align.h:51-58, one device launch)."""
    lib = load()
    n = len(jobs)
    arr = (ExtJob * max(1, n))()
    for i, (kind, q, t, max_d, band, f) in enumerate(jobs):
        arr[i] = ExtJob(q, len(q), t, len(t), max_d, band, f, EXT_KINDS[kind])
    res = (ExtResult * max(1, n))()
    lib.ndgpu_ext_batch.argtypes = [C.POINTER(ExtJob), C.c_int, C.POINTER(ExtResult)]
    lib.ndgpu_ext_batch.restype = C.c_int
    if lib.ndgpu_ext_batch(arr, n, res) != 0:
        raise RuntimeError("ndgpu_ext_batch failed: no usable HIP device?")
    return [(r.done, r.a, r.b, list(r.pos)) for r in res[:n]]


def poa_batch(jobs, resident=None, host=False):
    """jobs: [[bytes, ...]] -> [bytes]: what poa_to_consensus returns for every job's sequences, through ndgpu_poa_batch_flags (the
    alignments of all jobs on the device in lockstep rounds; lib/dag.c:658-694).  resident=True: the graphs live on the device from
    the first sequence to the consensus string; False: they stay on the host between the rounds; None: NDGPU_POA_RESIDENT=1 selects
    the former.  host=True: the host routine for every job.  The bytes are the same whichever way."""
    lib = load()
    n = len(jobs)
    arr = (PoaJob * max(1, n))()
    keep = []
    for i, seqs in enumerate(jobs):
        k = len(seqs)
        cs = (C.c_char_p * max(1, k))()
        cs[:k] = list(seqs)
        ln = (C.c_uint16 * max(1, k))(*[len(s) for s in seqs])
        keep.append((cs, ln))
        arr[i] = PoaJob(C.cast(cs, C.POINTER(C.c_char_p)), C.cast(ln, C.POINTER(C.c_uint16)), k)
    out = (C.c_void_p * max(1, n))()
    flags = (1 if host else 0) | (0 if resident is None else 2 if resident else 4)
    rc = lib.ndgpu_poa_batch_flags(arr, n, flags, out)
    if rc != 0:
        raise RuntimeError("ndgpu_poa_batch_flags failed (%d)" % rc)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    res = []
    for i in range(n):
        res.append(C.string_at(out[i]))
        libc.free(out[i])
    return res


def lq_rank_batch(jobs, host=False):
    """jobs: [[bytes, ...]] (1..40 sequences each) -> [(order, kscore, tail)]: the 8-mer ranking of every job's sequences through
    ndgpu_lq_rank_batch (lib/nextcorrect.c:281-337, 405-440) -- order[r] = the input index of the sequence at rank r, kscore[r] its
    score, tail = whether the tail windows were ranked too.  host=True: the engine's own host routine instead of the device."""
    lib = load()
    n = len(jobs)
    arr = (RankJob * max(1, n))()
    keep = []
    for i, seqs in enumerate(jobs):
        k = len(seqs)
        cs = (C.c_char_p * max(1, k))()
        cs[:k] = list(seqs)
        ln = (C.c_uint16 * max(1, k))(*[len(s) for s in seqs])
        keep.append((cs, ln))
        arr[i] = RankJob(C.cast(cs, C.POINTER(C.c_char_p)), C.cast(ln, C.POINTER(C.c_uint16)), k)
    res = (RankResult * max(1, n))()
    rc = lib.ndgpu_lq_rank_batch(arr, n, 1 if host else 0, res)
    if rc != 0:
        raise RuntimeError("ndgpu_lq_rank_batch failed (%d)" % rc)
    return [(list(res[i].order[:len(jobs[i])]), list(res[i].kscore[:len(jobs[i])]), int(res[i].tail)) for i in range(n)]


def walk_steps(t_pos, link, cov, base):
    """Four equally long integer sequences -> a numpy array of ndgpu_walk_step records (what cns_windows_batch takes as a job's steps)."""
    import numpy as np
    a = np.zeros(len(t_pos), dtype=np.dtype([("t_pos", "<i4"), ("link", "<u2"), ("cov", "<u2"), ("base", "u1"), ("pad_", "u1", (3,))]))
    a["t_pos"], a["link"], a["cov"], a["base"] = t_pos, link, cov, base
    return a


def cns_windows_batch(jobs, host=False):
    """jobs: [(steps, min_cov, lq_max_len, min_error_corrected_ratio)], steps as walk_steps() makes them (a best_pp walk, origin first)
    -> one dict per job through ndgpu_cns_windows_batch: the loop of generate_cns_from_best_score (lib/nextcorrect.c:1907-1982) on the
    device -- `bases` (numpy.uint32, pos << 8 | character, numbered as before reverse_consensus_base), `regions` (numpy.uint32 [k, 2]:
    start, end in emission order), len, uncorrected_len, lstrip, rstrip, lqseq_total_length and ok, the verdict of :1986-1987.
    host=True: the engine's own host routine instead of the device.  ValueError for a step the entry refuses (-2)."""
    import numpy as np
    lib = load()
    n = len(jobs)
    if n == 0:
        return []
    arr = (CnsJob * n)()
    keep = []
    for i, (steps, min_cov, lq_max_len, ratio) in enumerate(jobs):
        st = np.ascontiguousarray(steps)
        if st.dtype.itemsize != C.sizeof(WalkStep):
            raise ValueError("steps must be records of ndgpu_walk_step (api.walk_steps)")
        keep.append(st)
        arr[i] = CnsJob(st.ctypes.data if st.size else None, int(st.size), int(min_cov), int(lq_max_len), float(ratio))
    res = (CnsResult * n)()
    bw, rw = C.c_void_p(), C.c_void_p()
    rc = lib.ndgpu_cns_windows_batch(arr, n, 1 if host else 0, res, C.byref(bw), C.byref(rw))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("ndgpu_cns_windows_batch failed (%d)" % rc)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    n_words = sum(r.len for r in res)
    n_reg = sum(r.n_regions for r in res)
    words = np.ctypeslib.as_array(C.cast(bw, C.POINTER(C.c_uint32)), shape=(max(1, n_words),))[:n_words].copy()
    regs = np.ctypeslib.as_array(C.cast(rw, C.POINTER(C.c_uint32)), shape=(max(1, 2 * n_reg),))[:2 * n_reg].copy().reshape(-1, 2)
    libc.free(bw)
    libc.free(rw)
    return [dict(len=int(r.len), uncorrected_len=int(r.uncorrected_len), lstrip=int(r.lstrip), rstrip=int(r.rstrip),
                 lqseq_total_length=int(r.lqseq_total_length), ok=bool(r.ok), bases=words[r.base_off:r.base_off + r.len],
                 regions=regs[r.region_off:r.region_off + r.n_regions]) for r in res]


def cns_walk_batch(jobs, host=False):
    """jobs: [(steps, min_cov, lq_max_len, min_error_corrected_ratio, mode, seed)], steps as walk_steps() makes them, mode 0 raw reads
    (what cns_windows_batch answers), 1 HiFi reads (seed: the seed's bases as bytes, read at every non-gap step's t_pos), 2 -fast (seed
    None) -> one dict per job through ndgpu_cns_walk_batch.  Modes 0 and 1: the keys of cns_windows_batch (mode 1 counts len and
    lqseq_total_length alone).  Mode 2: len and identity (numpy.float32) as the engine reports them, lq_total_len, seq (bytes, the chosen
    stretch reversed), ok True.  Every dict carries its mode.  host=True: the engine's own host routines instead of the device.
    ValueError for what the entry refuses (-2)."""
    import numpy as np
    lib = load()
    n = len(jobs)
    if n == 0:
        return []
    arr = (CnsWalkJob * n)()
    keep = []
    for i, (steps, min_cov, lq_max_len, ratio, mode, seed) in enumerate(jobs):
        st = np.ascontiguousarray(steps)
        if st.dtype.itemsize != C.sizeof(WalkStep):
            raise ValueError("steps must be records of ndgpu_walk_step (api.walk_steps)")
        seed = None if seed is None else bytes(seed)
        keep.append((st, seed))
        arr[i] = CnsWalkJob(st.ctypes.data if st.size else None, int(st.size), int(min_cov), int(lq_max_len), float(ratio), int(mode),
                            0 if seed is None else len(seed), seed)
    res = (CnsWalkResult * n)()
    bw, rw, sw = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib.ndgpu_cns_walk_batch(arr, n, 1 if host else 0, res, C.byref(bw), C.byref(rw), C.byref(sw))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("ndgpu_cns_walk_batch failed (%d)" % rc)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    n_words = sum(r.len for r, j in zip(res, jobs) if j[4] != 2)
    n_reg = sum(r.n_regions for r in res)
    n_seq = sum(r.seq_len for r in res)
    words = np.ctypeslib.as_array(C.cast(bw, C.POINTER(C.c_uint32)), shape=(max(1, n_words),))[:n_words].copy()
    regs = np.ctypeslib.as_array(C.cast(rw, C.POINTER(C.c_uint32)), shape=(max(1, 2 * n_reg),))[:2 * n_reg].copy().reshape(-1, 2)
    seqs = C.string_at(sw, n_seq)
    libc.free(bw)
    libc.free(rw)
    libc.free(sw)
    out = []
    for r, j in zip(res, jobs):
        if j[4] == 2:
            out.append(dict(mode=2, len=int(r.len), identity=np.float32(r.identity), lq_total_len=int(r.lq_total_len), ok=bool(r.ok),
                            seq=seqs[r.seq_off:r.seq_off + r.seq_len]))
        else:
            out.append(dict(mode=int(j[4]), len=int(r.len), uncorrected_len=int(r.uncorrected_len), lstrip=int(r.lstrip),
                            rstrip=int(r.rstrip), lqseq_total_length=int(r.lqseq_total_length), ok=bool(r.ok),
                            bases=words[r.base_off:r.base_off + r.len], regions=regs[r.region_off:r.region_off + r.n_regions]))
    return out


def cns_mode_stats() -> dict:
    """ndgpu_cns_mode_stats: the counters of the HiFi and -fast forms on the device (K21), cleared by reset_stats()."""
    s = CnsModeStats()
    load().ndgpu_get_cns_mode_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in CnsModeStats._fields_}


def splice_batch(jobs, host=False):
    """jobs: [(words, lstrip, rstrip, regions, read_type)]: words a uint32 array of pos << 8 | char in ascending positions, regions
    [(start, end, len, sudoseed bytes)] in the engine's order (the index counts down while the positions go up), read_type 3 for HiFi
    -> one dict per job through ndgpu_splice_batch: len and identity (numpy.float32) as the engine reports them (len 2 and 4: the two
    error outcomes), lq_total_len, out_len, lq_m, hq_m, lq_i, clip_s, clip_e, seq (bytes).  host=True: the host statement instead of
    the device.  ValueError for what the entry refuses (-2)."""
    import numpy as np
    lib = load()
    n = len(jobs)
    if n == 0:
        return []
    arr = (SpliceJob * n)()
    keep = []
    for i, (words, lstrip, rstrip, regions, read_type) in enumerate(jobs):
        w = np.ascontiguousarray(words, dtype=np.uint32)
        rg = (SpliceRegion * max(1, len(regions)))()
        for k, (start, end, ln, seed) in enumerate(regions):
            seed = bytes(seed)
            keep.append(seed)
            rg[k] = SpliceRegion(int(start), int(end), int(ln), len(seed), seed)
        keep.append((w, rg))
        arr[i] = SpliceJob(w.ctypes.data if w.size else None, int(w.size), int(lstrip), int(rstrip), len(regions),
                           rg if len(regions) else None, int(read_type), 0)
    res = (SpliceResult * n)()
    sw = C.c_void_p()
    rc = lib.ndgpu_splice_batch(arr, n, 1 if host else 0, res, C.byref(sw))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("ndgpu_splice_batch failed (%d)" % rc)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    seqs = C.string_at(sw, sum(r.seq_len for r in res))
    libc.free(sw)
    return [dict(len=int(r.len), identity=np.float32(r.identity), lq_total_len=int(r.lq_total_len), out_len=int(r.out_len), lq_m=int(r.lq_m),
                 hq_m=int(r.hq_m), lq_i=int(r.lq_i), clip_s=int(r.clip_s), clip_e=int(r.clip_e), seq=seqs[r.seq_off:r.seq_off + r.seq_len])
            for r in res]


def splice_stats() -> dict:
    """ndgpu_splice_stats: the counters of the splice and the SSR trim on the device (K24), cleared by reset_stats()."""
    s = SpliceStats()
    load().ndgpu_get_splice_stats(C.byref(s))
    return {n: getattr(s, n) for n, _ in SpliceStats._fields_}


PHASE_EMPTY, PHASE_DROPPED, PHASE_SEED, PHASE_RANKED = 0, 1, 2, 3


def hifi_phase_batch(jobs, host=False):
    """jobs: [(n_aligned, [(start, end, [bytes, ...], [source read, ...]), ...])] -- a HiFi pile each: its regions in order, every one
    with its inclusive seed columns and 0..40 candidates -> one dict per job through ndgpu_hifi_phase_batch
    (generate_lqseqs_from_tags_kmer, lib/nextcorrect.c:787-948 with the helpers of 512-737): has_heter, pass2, declined and `regions`,
    one dict per region: kind (PHASE_*), lower, indexs, tail, n, seed, seed_pos, and perm / kscore over the region's candidates -- the
    input index and the score of the candidate at every position of lq.seqs as the routine leaves it.  host=True: the engine's own
    host rule instead of the device (K22)."""
    lib = load()
    n = len(jobs)
    arr = (PhaseJob * max(1, n))()
    keep = []
    total = 0
    for i, (n_aligned, regions) in enumerate(jobs):
        m = len(regions)
        ra = (PhaseRegionIn * max(1, m))()
        for r, (start, end, seqs, src) in enumerate(regions):
            k = len(seqs)
            if len(src) != k:
                raise ValueError("a source read per candidate")
            cs = (C.c_char_p * max(1, k))()
            cs[:k] = list(seqs)
            ln = (C.c_uint16 * max(1, k))(*[len(s) for s in seqs])
            sr = (C.c_uint16 * max(1, k))(*src)
            keep.append((cs, ln, sr))
            ra[r] = PhaseRegionIn(start, end, k, 0, C.cast(cs, C.POINTER(C.c_char_p)), C.cast(ln, C.POINTER(C.c_uint16)),
                                  C.cast(sr, C.POINTER(C.c_uint16)))
        keep.append(ra)
        arr[i] = PhaseJob(n_aligned, m, C.cast(ra, C.POINTER(PhaseRegionIn)))
        total += m
    res = (PhaseRegion * max(1, total))()
    piles = (PhasePile * max(1, n))()
    rc = lib.ndgpu_hifi_phase_batch(arr, n, 1 if host else 0, res, piles)
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("ndgpu_hifi_phase_batch failed (%d)" % rc)
    out, at = [], 0
    for i, (_, regions) in enumerate(jobs):
        regs = []
        for r, (_, _, seqs, _) in enumerate(regions):
            g = res[at + r]
            k = len(seqs)
            regs.append(dict(kind=int(g.kind), lower=int(g.lower), indexs=int(g.indexs), tail=int(g.tail), n=int(g.n), seed=int(g.seed),
                             seed_pos=int(g.seed_pos), perm=list(g.perm[:k]), kscore=list(g.kscore[:k])))
        at += len(regions)
        out.append(dict(has_heter=int(piles[i].has_heter), pass2=int(piles[i].pass2), declined=int(piles[i].declined), regions=regs))
    return out


def phase_stats() -> dict:
    """ndgpu_phase_stats: the counters of the phasing and ranking of HiFi candidates on the device (K22), cleared by reset_stats()."""
    s = PhaseStats()
    load().ndgpu_get_phase_stats(C.byref(s))
    return {n: (list(getattr(s, n)) if n in ("kind", "declined") else getattr(s, n)) for n, _ in PhaseStats._fields_}


def _align_call(fn, name, arr, n, host, strings):
    import numpy as np
    if n == 0:
        return []
    res = (AlnResult * n)()
    cg, qa, ta = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = fn(arr, n, (1 if host else 0) | (2 if strings else 0), res, C.byref(cg), C.byref(qa) if strings else None,
            C.byref(ta) if strings else None)
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("%s failed (%d)" % (name, rc))
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    total = sum(r.n_cigar for r in res)
    runs = np.ctypeslib.as_array(C.cast(cg, C.POINTER(C.c_uint32)), shape=(max(1, total),))[:total].copy()
    out, at = [], 0
    for r in res:
        d = dict(status=int(r.status), aln_len=int(r.aln_len), q_used=int(r.q_used), t_used=int(r.t_used), n_match=int(r.n_match),
                 n_ins=int(r.n_ins), n_del=int(r.n_del), max_gap_run=int(r.max_gap_run),
                 cigar=runs[r.cigar_off:r.cigar_off + r.n_cigar])
        if strings:
            d["q_aln"] = C.string_at(qa.value + at, r.aln_len)
            d["t_aln"] = C.string_at(ta.value + at, r.aln_len)
            at += r.aln_len + 1
        out.append(d)
    libc.free(cg)
    if strings:
        libc.free(qa)
        libc.free(ta)
    return out


def align_batch(pairs, hq=False, host=False, strings=False):
    """pairs: [(q, t)] or [(q, t, hq)] (bytes) -> one dict per pair: what align() / align_hq() would report -- status (0 none,
    1 aligned, 2 the > 250-gap abort), aln_len, q_used, t_used --, the columns by kind (n_match, n_ins, n_del), max_gap_run and
    `cigar`, a numpy.uint32 array of length << 4 | op (7 '=', 1 'I', 2 'D'; cigar_string() prints it), through ndgpu_align_batch:
    all pairs share the kernel launches and the CIGARs are built on the device.  host=True: summaries and runs from the
    downloaded columns on the host instead.  strings=True: also q_aln / t_aln, the gapped strings as align() writes them."""
    lib = load()
    arr = (AlnJob * max(1, len(pairs)))()
    for i, p in enumerate(pairs):
        arr[i] = AlnJob(p[0], len(p[0]), p[1], len(p[1]), int(p[2]) if len(p) > 2 else int(bool(hq)))
    return _align_call(lib.ndgpu_align_batch, "ndgpu_align_batch", arr, len(pairs), host, strings)


def cigar_string(cigar) -> str:
    """'12=1I3D...' of a cigar array as align_batch() returns it (BAM operation numbers)."""
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=X"[int(w) & 15]) for w in cigar)


_POA_RESIDENT_STATS = ("poa_resident_jobs", "poa_resident_declined", "poa_graph_launches", "poa_graph_ms", "poa_h2d_bytes", "poa_d2h_bytes")


_CNS_STATS = ("cns_jobs", "cns_declined", "cns_launches", "cns_regions", "cns_ms", "cns_d2h_bytes", "walk_d2h_bytes")


def stats() -> dict:
    lib = load()
    s = Stats()
    lib.ndgpu_get_stats(C.byref(s))
    names = [f[0] for f in Stats._fields_]
    # ndgpu_stats grows at its end (the C ABI); the dictionary lists the counters of the resident POA graphs with the other POA
    # counters, behind poa_ms, so the keys that closed it before still close it
    late = [n for n in names if n in _POA_RESIDENT_STATS]
    names = [n for n in names if n not in _POA_RESIDENT_STATS]
    at = names.index("poa_ms") + 1
    names[at:at] = late
    # likewise the counters of the walk's consensus words and windows (K20), behind backtrack_ms
    late = [n for n in names if n in _CNS_STATS]
    names = [n for n in names if n not in _CNS_STATS]
    at = names.index("backtrack_ms") + 1
    names[at:at] = late
    return {n: getattr(s, n) for n in names}


def release_device_memory() -> int:
    """Hand the consensus contexts' device buffers back (ndgpu_release_memory); returns the bytes released."""
    lib = load()
    lib.ndgpu_release_memory.restype = C.c_uint64
    return int(lib.ndgpu_release_memory())


def reserve_device_memory(n_bytes: int):
    """Device bytes every later consensus call leaves free (ndgpu_reserve_device_memory)."""
    lib = load()
    lib.ndgpu_reserve_device_memory.argtypes = [C.c_uint64]
    lib.ndgpu_reserve_device_memory.restype = None
    lib.ndgpu_reserve_device_memory(int(max(0, n_bytes)))


def reset_stats():
    load().ndgpu_reset_stats()


def device_count() -> int:
    return int(load().ndgpu_device_count())
