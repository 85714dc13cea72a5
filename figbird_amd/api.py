"""ctypes binding of libfighip.so (include/figbird_hip.h) and libfighost.so.

This is the Python face of the C ABI used by the tests and bench.py.  It does no computing
itself: every gap is filled by the HIP engine behind `fig_fill_gaps`.  If the library or a
GPU is missing it raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from dataclasses import replace as dc_replace
from typing import List, Optional

import numpy as np

from . import build as _build

c_double_p = C.POINTER(C.c_double)
c_i32_p = C.POINTER(C.c_int32)
c_i64_p = C.POINTER(C.c_int64)
c_u8_p = C.POINTER(C.c_uint8)


class FigModel(C.Structure):
    _fields_ = [
        ("max_read_length", C.c_int32), ("error_pos_dist", c_double_p), ("in_pos_dist", c_double_p),
        ("del_pos_dist", c_double_p), ("error_type_probs", C.c_double * 25),
        ("insert_len_dist_smoothed", c_double_p), ("max_insert_size", C.c_int32),
        ("insert_threshold_min", C.c_int32), ("insert_threshold_max", C.c_int32), ("gap_prob_cutoff", C.c_int32),
        ("partial_flag", C.c_int32), ("unmapped_flag", C.c_int32), ("script_itr", C.c_int32),
        ("max_distance", C.c_int32), ("read_length", C.c_int32), ("neg_overlap", C.c_int32),
        ("partial_len", C.c_int32), ("unm_limit", C.c_int32),
    ]


class FigGapBatch(C.Structure):
    _fields_ = [
        ("n_gaps", C.c_int64), ("n_contigs", C.c_int64), ("contig_off", c_i64_p), ("contig_seq", C.c_char_p),
        ("gap_contig", c_i32_p), ("gap_start", c_i64_p), ("gap_len", c_i32_p), ("gap_stat2", c_i32_p),
        ("gap_fillflag", c_i32_p),
        ("u_read_off", c_i64_p), ("u_anchor_pos", c_i32_p), ("u_is_reverse", c_u8_p), ("u_seq_off", c_i64_p),
        ("u_seq", C.c_char_p),
        ("p_read_off", c_i64_p), ("p_clipped_index", c_i32_p), ("p_match", c_i32_p), ("p_pos", c_i32_p),
        ("p_ref_pos", c_i32_p), ("p_seq_off", c_i64_p), ("p_seq", C.c_char_p), ("p_qual", C.c_char_p),
        ("gap_ot_preset", c_u8_p),
    ]


class FigGapResults(C.Structure):
    _fields_ = [
        ("filled_len", c_i32_p), ("gaptofill", c_i32_p), ("str_off", c_i64_p), ("str", C.c_char_p),
        ("str_capacity", C.c_int64),
        ("dbg_max_cand", C.c_int32), ("dbg_n_cand", c_i32_p), ("dbg_cand_i", c_i32_p), ("dbg_cand_lik", c_double_p),
        ("dbg_n_place", c_i32_p),
        ("draw_pos", c_i32_p), ("draw_isz", c_i32_p), ("draw_len", c_i32_p),
        ("dbg_plane_cols", C.c_int32), ("dbg_plane_reads", C.c_int32), ("dbg_counts", c_double_p), ("dbg_read_maxlv", c_double_p),
    ]


class FigGapSupport(C.Structure):
    _fields_ = [("counts", c_i32_p), ("origin", c_i32_p)]


# fig_gap_support::origin (include/figbird_hip.h)
SUP_NONE, SUP_FINAL, SUP_ORIGINAL, SUP_TIEBREAK = 0, 1, 2, 4


class FigGapQuality(C.Structure):
    _fields_ = [("loglik", c_double_p), ("phred", c_u8_p), ("state", c_u8_p)]


# fig_gap_quality::state (include/figbird_hip.h)
QUAL_OFF, QUAL_ON = 0, 1


class FigReadPlacement(C.Structure):
    _fields_ = [("ll_drawn", c_double_p), ("ll_other", c_double_p), ("sum_other", c_double_p), ("off_other", c_i32_p), ("n_valid", c_i32_p),
                ("pq", c_u8_p), ("state", c_u8_p)]


# fig_read_placement::state / ::pq (include/figbird_hip.h)
PLACE_OFF, PLACE_ON, PLACE_NONE, PLACE_MAX_PQ = 0, 1, 255, 60


@dataclass
class Placement:
    """fig_read_placement of one call: the six per-read arrays are indexed like the unmapped part of draw_pos, state per gap"""
    ll_drawn: np.ndarray
    ll_other: np.ndarray
    sum_other: np.ndarray
    off_other: np.ndarray
    n_valid: np.ndarray
    pq: np.ndarray
    state: np.ndarray


class FigGapSoftqual(C.Structure):
    _fields_ = [("wcount", c_double_p), ("eloglik", c_double_p), ("phred", c_u8_p), ("state", c_u8_p)]


# fig_gap_softqual::state (include/figbird_hip.h)
SOFTQ_OFF, SOFTQ_ON = 0, 1


@dataclass
class SoftQual:
    """fig_gap_softqual of one call: the planes are indexed like the strings (base x of gap g at str_off[g] + x), state per gap;
    placement: the fig_read_placement of the same call, when asked for"""
    wcount: np.ndarray
    eloglik: np.ndarray
    phred: np.ndarray
    state: np.ndarray
    placement: Optional[Placement] = None


class FigGapIndel(C.Structure):
    _fields_ = [("ll_flat", c_double_p), ("ll_gapped", c_double_p), ("n_ins", c_i32_p), ("n_del", c_i32_p), ("d_end", c_i32_p), ("d_start", c_i32_p),
                ("del_reads", c_i32_p), ("ins_reads", c_i32_p), ("cover", c_i32_p), ("ins_end", c_i32_p),
                ("call", c_u8_p), ("call_end", c_u8_p), ("state", c_u8_p)]


# fig_gap_indel::state and the band's half width (include/figbird_hip.h)
INDEL_OFF, INDEL_ON, INDEL_W = 0, 1, 7


@dataclass
class Indel:
    """fig_gap_indel of one call: the six per-read arrays are indexed like the unmapped part of draw_pos, the three planes and call
    (uint8: ord of 'D', 'I' or '.') like the strings (base x of gap g at str_off[g] + x), ins_end, call_end and state per gap"""
    ll_flat: np.ndarray
    ll_gapped: np.ndarray
    n_ins: np.ndarray
    n_del: np.ndarray
    d_end: np.ndarray
    d_start: np.ndarray
    del_reads: np.ndarray
    ins_reads: np.ndarray
    cover: np.ndarray
    ins_end: np.ndarray
    call: np.ndarray
    call_end: np.ndarray
    state: np.ndarray


class FigGapPolish(C.Structure):
    _fields_ = [("edit", c_i32_p), ("edit_end", c_i32_p), ("polished_len", c_i32_p), ("draw_pos", c_i32_p), ("n_ins", c_i32_p), ("n_del", c_i32_p),
                ("rounds", c_i32_p), ("ll_before", c_double_p), ("ll_after", c_double_p), ("state", c_u8_p)]


# fig_gap_polish::state bits and the limits of the loop (include/figbird_hip.h)
POLISH_ON, POLISH_EDITED, POLISH_REJECTED, POLISH_REVERTED, POLISH_CAPPED = 1, 2, 4, 8, 16
POLISH_MAX_SITES, POLISH_MAX_ROUNDS, POLISH_DEFAULT_ROUNDS = 16, 8, 4


def polish_string(edit, edit_end: int, string) -> np.ndarray:
    """the polished string of one gap (uint8) from its original bytes and its edit words: the inserted bases of edit[x], then
    string[x] unless removed; then the bases of edit_end"""
    out = bytearray()
    for w, ch in list(zip(edit, string)) + [(edit_end, None)]:
        w = int(w)
        out += bytes(b"ACGT"[(w >> (4 + 2 * i)) & 3] for i in range((w >> 1) & 7))
        if ch is not None and not w & 1:
            out.append(int(ch))
    return np.frombuffer(bytes(out), dtype=np.uint8)


@dataclass
class Polish:
    """fig_gap_polish of one call: edit is indexed like the strings (column x of gap g at str_off[g] + x), draw_pos like the unmapped
    part of the draw plane, everything else per gap.  filled: the FillResult the call was given."""
    edit: np.ndarray
    edit_end: np.ndarray
    polished_len: np.ndarray
    draw_pos: np.ndarray
    n_ins: np.ndarray
    n_del: np.ndarray
    rounds: np.ndarray
    ll_before: np.ndarray
    ll_after: np.ndarray
    state: np.ndarray
    filled: Optional["FillResult"] = None

    def strings(self):
        """the polished string of every gap (uint8 arrays); a gap that is off keeps its own bytes"""
        f = self.filled
        out = []
        for g in range(len(self.state)):
            a = int(f.str_off[g]); n = max(int(f.filled_len[g]), 0)
            own = np.asarray(f.raw[a:a + n], dtype=np.uint8)
            out.append(polish_string(self.edit[a:a + n], int(self.edit_end[g]), own) if self.state[g] & POLISH_ON else own)
        return out

    def result(self) -> "FillResult":
        """a FillResult made by hand of the polished strings, the shifted offsets and the draw planes: it goes straight into
        quality(), placement() or indel() while the batch is resident"""
        f = self.filled
        strs = self.strings()
        n = len(strs)
        fl = np.array(f.filled_len[:n], dtype=np.int32)
        dpos, disz, dlen = (np.array(a, dtype=np.int32) for a in f.draw)
        for g in range(n):
            if self.state[g] & POLISH_ON:
                fl[g] = len(strs[g]); dlen[2 * g] = len(strs[g])
        so = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.int64)
        raw = np.concatenate(strs + [np.zeros(0, np.uint8)]).astype(np.uint8)
        dpos[:len(self.draw_pos)] = self.draw_pos
        return FillResult(fl, np.array(f.gaptofill[:n]), None, str_off=so, raw=raw if len(raw) else np.zeros(1, np.uint8), draw=(dpos, disz, dlen),
                          support_origin=f.support_origin)


class FigReadRecruit(C.Structure):
    _fields_ = [("ll_seed", c_double_p), ("ll_second", c_double_p), ("ll_flat", c_double_p), ("ll_gapped", c_double_p), ("score", c_double_p),
                ("off_seed", c_i32_p), ("off_second", c_i32_p), ("n_valid", c_i32_p), ("d_end", c_i32_p), ("read_state", c_u8_p),
                ("draw_pos", c_i32_p), ("draw_isz", c_i32_p), ("n_candidates", c_i32_p), ("n_recruited", c_i32_p), ("state", c_u8_p)]


# fig_read_recruit::state and ::read_state (include/figbird_hip.h)
RECRUIT_OFF, RECRUIT_ON = 0, 1
RECRUIT_READ_OFF, RECRUIT_KEPT, RECRUIT_NONE, RECRUIT_BELOW, RECRUIT_AMBIGUOUS, RECRUIT_RECRUITED = 0, 1, 2, 3, 4, 5


@dataclass
class Recruit:
    """fig_read_recruit of one call: the twelve per-read arrays are indexed like the unmapped part of draw_pos, n_candidates,
    n_recruited and state per gap.  filled: the FillResult the call was given."""
    ll_seed: np.ndarray
    ll_second: np.ndarray
    ll_flat: np.ndarray
    ll_gapped: np.ndarray
    score: np.ndarray
    off_seed: np.ndarray
    off_second: np.ndarray
    n_valid: np.ndarray
    d_end: np.ndarray
    read_state: np.ndarray
    draw_pos: np.ndarray
    draw_isz: np.ndarray
    n_candidates: np.ndarray
    n_recruited: np.ndarray
    state: np.ndarray
    filled: Optional["FillResult"] = None

    def result(self) -> "FillResult":
        """a FillResult made by hand of the caller's strings and the merged draw planes, the partial reads' part of the planes
        carried over unchanged: it goes straight into indel() and polish() while the batch is resident"""
        f = self.filled
        dpos, disz, dlen = (np.array(a, dtype=np.int32) for a in f.draw)
        dpos[:len(self.draw_pos)] = self.draw_pos
        disz[:len(self.draw_isz)] = self.draw_isz
        return dc_replace(f, draw=(dpos, disz, dlen), placement=None, quality=None, indel=None, polish=None, softqual=None, recruit=None)


class FigGapAlnqual(C.Structure):
    _fields_ = [("loglik", c_double_p), ("depth", c_i32_p), ("agree", c_i32_p), ("skip", c_i32_p), ("phred", c_u8_p), ("ll_gapped", c_double_p),
                ("n_ins", c_i32_p), ("n_del", c_i32_p), ("d_end", c_i32_p), ("d_start", c_i32_p), ("state", c_u8_p)]


# fig_gap_alnqual::state (include/figbird_hip.h)
ALNQ_OFF, ALNQ_ON = 0, 1


@dataclass
class AlnQual:
    """fig_gap_alnqual of one call: the five planes are indexed like the strings (base x of gap g at str_off[g] + x), the five per-read
    arrays like the unmapped part of draw_pos, state per gap.  filled: the FillResult the call was given."""
    loglik: np.ndarray
    depth: np.ndarray
    agree: np.ndarray
    skip: np.ndarray
    phred: np.ndarray
    ll_gapped: np.ndarray
    n_ins: np.ndarray
    n_del: np.ndarray
    d_end: np.ndarray
    d_start: np.ndarray
    state: np.ndarray
    filled: Optional["FillResult"] = None


class FigStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
                ("packed_bytes", C.c_int64), ("place_calls", C.c_int64), ("alg_flops", C.c_double),
                ("n_launches", C.c_int32), ("cont_chunks", C.c_int32), ("spec_flops", C.c_double),
                ("mle_alg_flops", C.c_double), ("mle_exec_flops", C.c_double)]


EXPORTS = ["fig_version", "fig_strerror", "fig_ctx_create", "fig_ctx_destroy", "fig_ctx_set_model",
           "fig_results_capacity", "fig_batch_upload", "fig_fill_resident", "fig_fill_resident_ex", "fig_batch_free", "fig_fill_gaps",
           "fig_get_stats", "fig_batch_probe_reach", "fig_batch_set_ot_preset", "fig_batch_quality", "fig_batch_placement",
           "fig_batch_softqual", "fig_batch_indel", "fig_batch_polish", "fig_polish_apply", "fig_batch_recruit", "fig_batch_alnqual"]

_lib = None
_host = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libfighip.so and set prototypes.  Raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _build.LIB
    if not os.path.exists(p):
        raise RuntimeError(f"libfighip.so not built at {p}: run `python -m figbird_amd.build` (there is no CPU fallback)")
    lib = C.CDLL(p)
    lib.fig_version.restype = C.c_int
    lib.fig_strerror.restype = C.c_char_p
    lib.fig_strerror.argtypes = [C.c_int]
    lib.fig_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.fig_ctx_destroy.argtypes = [C.c_void_p]
    lib.fig_ctx_destroy.restype = None
    lib.fig_ctx_set_model.argtypes = [C.c_void_p, C.POINTER(FigModel)]
    lib.fig_results_capacity.argtypes = [C.POINTER(FigModel), C.POINTER(FigGapBatch)]
    lib.fig_results_capacity.restype = C.c_int64
    lib.fig_batch_upload.argtypes = [C.c_void_p, C.POINTER(FigGapBatch)]
    lib.fig_fill_resident.argtypes = [C.c_void_p, C.POINTER(FigGapResults)]
    lib.fig_batch_free.argtypes = [C.c_void_p]
    lib.fig_batch_free.restype = None
    lib.fig_fill_gaps.argtypes = [C.c_void_p, C.POINTER(FigGapBatch), C.POINTER(FigGapResults)]
    lib.fig_get_stats.argtypes = [C.c_void_p, C.POINTER(FigStats)]
    lib.fig_batch_probe_reach.argtypes = [C.c_void_p, c_u8_p]
    lib.fig_batch_set_ot_preset.argtypes = [C.c_void_p, c_u8_p]
    if hasattr(lib, "fig_fill_resident_ex"):          # (the CPU emulation of the tests implements the ABI without it)
        lib.fig_fill_resident_ex.argtypes = [C.c_void_p, C.POINTER(FigGapResults), C.POINTER(FigGapSupport)]
    if hasattr(lib, "fig_batch_quality"):             # (likewise)
        lib.fig_batch_quality.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.POINTER(FigGapQuality)]
    if hasattr(lib, "fig_batch_placement"):           # (likewise)
        lib.fig_batch_placement.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.POINTER(FigReadPlacement)]
    if hasattr(lib, "fig_batch_softqual"):            # (likewise)
        lib.fig_batch_softqual.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.POINTER(FigReadPlacement), C.POINTER(FigGapSoftqual)]
    if hasattr(lib, "fig_batch_indel"):               # (likewise)
        lib.fig_batch_indel.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.POINTER(FigGapIndel)]
    if hasattr(lib, "fig_batch_polish"):              # (likewise)
        lib.fig_batch_polish.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.c_int, C.POINTER(FigGapPolish)]
        lib.fig_polish_apply.argtypes = [C.POINTER(FigGapResults), C.POINTER(FigGapPolish), C.c_int64, c_u8_p]
    if hasattr(lib, "fig_batch_recruit"):             # (likewise)
        lib.fig_batch_recruit.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.c_double, C.POINTER(FigReadRecruit)]
    if hasattr(lib, "fig_batch_alnqual"):             # (likewise)
        lib.fig_batch_alnqual.argtypes = [C.c_void_p, C.POINTER(FigGapResults), c_i32_p, C.POINTER(FigGapAlnqual)]
    if path is None:
        _lib = lib
    return lib


def load_host_library() -> C.CDLL:
    global _host
    if _host is None:
        if not os.path.exists(_build.HOSTLIB):
            raise RuntimeError("libfighost.so not built: run `python -m figbird_amd.build`")
        _host = C.CDLL(_build.HOSTLIB)
        _host.fighost_build_model.restype = C.c_int
        _host.fighost_run_open.restype = C.c_void_p
        _host.fighost_run_open.argtypes = [C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
        _host.fighost_run_close.argtypes = [C.c_void_p]; _host.fighost_run_close.restype = None
        _host.fighost_run_ngaps.argtypes = [C.c_void_p]; _host.fighost_run_ngaps.restype = C.c_int64
        _host.fighost_run_sizes.argtypes = [C.c_void_p, c_i32_p, c_i64_p, c_i64_p]
        _host.fighost_run_params.argtypes = [C.c_void_p, c_i32_p]
        _host.fighost_run_message.argtypes = [C.c_void_p, C.c_int]; _host.fighost_run_message.restype = C.c_char_p
        _host.fighost_run_model.argtypes = [C.c_void_p, C.POINTER(FigModel)]
        _host.fighost_run_shard.argtypes = [C.c_void_p, c_i64_p, C.c_int64, C.POINTER(FigGapBatch), c_i64_p, c_i64_p]
        _host.fighost_run_ot_presets.argtypes = [C.c_void_p, c_u8_p, c_u8_p]
        _host.fighost_run_write.argtypes = [C.c_void_p, c_i32_p, c_i32_p, c_i64_p, C.c_char_p, c_i32_p, c_i32_p, c_i32_p, C.c_char_p, C.c_int]
        _host.fighost_run_write_support.argtypes = [C.c_void_p, c_i32_p, c_i64_p, C.c_char_p, c_i32_p, c_i32_p, C.c_char_p, C.c_int]
        _host.fighost_quality_tables.argtypes = [C.POINTER(FigModel), c_double_p, c_double_p, c_double_p]
        _host.fighost_quality_phred.argtypes = [C.c_int64, c_double_p, C.c_char_p, c_u8_p]
        _host.fighost_quality_gaps_on.argtypes = [C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_run_write_quality.argtypes = [C.c_void_p, c_i32_p, c_i64_p, c_u8_p, c_u8_p, C.c_char_p, C.c_int]
        _host.fighost_placement_li.argtypes = [C.POINTER(FigModel), c_double_p]
        _host.fighost_placement_isz.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _host.fighost_placement_isz.restype = C.c_int64
        _host.fighost_placement_valid.argtypes = [C.POINTER(FigModel), C.c_int64]
        _host.fighost_placement_phred.argtypes = [C.c_int64, c_double_p, c_double_p, c_double_p, c_u8_p]
        _host.fighost_placement_gaps_on.argtypes = [C.c_int, C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_run_write_placement.argtypes = [C.c_void_p, c_i32_p, c_u8_p, c_u8_p, C.c_char_p, C.c_int]
        _host.fighost_softqual_gaps_on.argtypes = [C.c_int, C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_softqual_active.argtypes = [C.c_double]
        _host.fighost_softqual_mz.argtypes = [C.c_int64, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_u8_p]
        _host.fighost_run_write_softquality.argtypes = [C.c_void_p, c_i32_p, c_i64_p, c_u8_p, c_u8_p, C.c_char_p, C.c_int]
        _host.fighost_indel_tables.argtypes = [C.POINTER(FigModel), c_double_p, c_double_p]
        _host.fighost_indel_gaps_on.argtypes = [C.c_int, C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_indel_aligned.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        _host.fighost_indel_end_order.argtypes = [C.c_int]
        _host.fighost_indel_call.argtypes = [C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_indel_call_end.argtypes = [C.c_int32, C.c_int32]
        _host.fighost_run_write_indel.argtypes = [C.c_void_p, c_i32_p, c_i64_p, C.c_char_p, C.c_char_p, c_u8_p, C.c_char_p, C.c_int]
        _host.fighost_polish_shift.argtypes = [C.c_int32, C.c_int, C.c_int32]
        _host.fighost_polish_touched.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        _host.fighost_polish_counted.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_int32]
        _host.fighost_polish_sites.argtypes = [C.c_char_p, C.c_int32, C.c_char, c_i32_p, c_i32_p]
        _host.fighost_polish_best.argtypes = [c_double_p, C.c_int]
        _host.fighost_polish_accept.argtypes = [C.c_double, C.c_double]
        _host.fighost_polish_keep.argtypes = [C.c_double, C.c_double]
        _host.fighost_polish_insert.argtypes = [c_i32_p, C.c_int32, c_i32_p, C.c_int64, C.c_int]
        _host.fighost_polish_remove.argtypes = [c_i32_p, C.c_int32, c_i32_p, C.c_int64]
        _host.fig_polish_apply.argtypes = [C.POINTER(FigGapResults), C.POINTER(FigGapPolish), C.c_int64, c_u8_p]
        _host.fighost_run_write_polished.argtypes = [C.c_void_p, c_i32_p, c_i64_p, C.c_char_p, c_i32_p, c_i32_p, c_i32_p, c_u8_p, c_i32_p, c_i32_p, C.c_char_p, C.c_int]
        _host.fighost_recruit_gaps_on.argtypes = [C.c_int, C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_recruit_candidate.argtypes = [C.c_int32]
        _host.fighost_recruit_outside.argtypes = [C.c_int32, C.c_int32]
        _host.fighost_recruit_before.argtypes = [C.c_double, C.c_int32, C.c_double, C.c_int32]
        _host.fighost_recruit_seeded.argtypes = [C.c_int32, C.c_double]
        _host.fighost_recruit_score.argtypes = [C.c_double, C.c_double]; _host.fighost_recruit_score.restype = C.c_double
        _host.fighost_recruit_rule.argtypes = [C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double]
        _host.fighost_recruit_margin_ok.argtypes = [C.c_double]
        _host.fighost_recruit_merge.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i32_p]
        _host.fighost_recruit_char.argtypes = [C.c_int]
        _host.fighost_run_write_recruit.argtypes = [C.c_void_p, c_i32_p, c_u8_p, c_i32_p, c_i32_p, c_i32_p, C.c_char_p, C.c_int]
        _host.fighost_alnqual_gaps_on.argtypes = [C.c_int, C.c_int64, c_i32_p, c_i32_p, c_i32_p, c_u8_p]
        _host.fighost_alnqual_map_bytes.argtypes = [C.c_int]
        _host.fighost_alnqual_nibble.argtypes = [c_u8_p, C.c_int]
        _host.fighost_alnqual_set_nibble.argtypes = [c_u8_p, C.c_int, C.c_int]
        _host.fighost_alnqual_flat.argtypes = [c_u8_p, C.c_int, c_i32_p]
        _host.fighost_alnqual_span.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i32_p]
        _host.fighost_run_write_alnquality.argtypes = [C.c_void_p, c_i32_p, c_i64_p, c_u8_p, c_u8_p, C.c_char_p, C.c_int]
    return _host


def _p(arr, typ):
    return arr.ctypes.data_as(typ)


@dataclass
class Model:
    """Run-level model tables (A0) + run parameters; mirrors `fig_model`."""
    e: np.ndarray
    ins: np.ndarray
    dele: np.ndarray
    T: np.ndarray
    insd: np.ndarray
    Tmin: int
    Tmax: int
    cutoff: int
    partial_flag: int
    unmapped_flag: int
    script_itr: int
    max_distance: int
    read_length: int
    neg_overlap: int
    partial_len: int
    unm_limit: int = 400
    stats: tuple = (0.0, 0.0, 0.0)

    def cstruct(self) -> FigModel:
        m = FigModel()
        m.max_read_length = len(self.e)
        m.error_pos_dist = _p(self.e, c_double_p)
        m.in_pos_dist = _p(self.ins, c_double_p)
        m.del_pos_dist = _p(self.dele, c_double_p)
        for i in range(25):
            m.error_type_probs[i] = float(self.T[i])
        m.insert_len_dist_smoothed = _p(self.insd, c_double_p)
        m.max_insert_size = len(self.insd)
        m.insert_threshold_min = self.Tmin
        m.insert_threshold_max = self.Tmax
        m.gap_prob_cutoff = self.cutoff
        m.partial_flag = self.partial_flag
        m.unmapped_flag = self.unmapped_flag
        m.script_itr = self.script_itr
        m.max_distance = self.max_distance
        m.read_length = self.read_length
        m.neg_overlap = self.neg_overlap
        m.partial_len = self.partial_len
        m.unm_limit = self.unm_limit
        return m


def model_from_files(scf: str, tmp_dir: str, map_file: str, *, partial_flag: int, unmapped_flag: int, script_itr: int,
                     max_distance: int, read_length: int, neg_overlap: int, partial_len: int,
                     setinputmean: int = 0, isz: int = 0) -> Model:
    """Build the model exactly as figfill does (host C++, figbird_amd/csrc/host/fig_host.cpp)."""
    h = load_host_library()
    cap_l, cap_i = 256, 1 << 20
    e = np.zeros(cap_l); ins = np.zeros(cap_l); dele = np.zeros(cap_l); T = np.zeros(25); insd = np.zeros(cap_i)
    ints = np.zeros(5, dtype=np.int32); st = np.zeros(3)
    rc = h.fighost_build_model(scf.encode(), tmp_dir.encode(), map_file.encode(), C.c_int(partial_flag), C.c_int(partial_len),
                               C.c_int(setinputmean), C.c_int(isz), C.c_int(cap_l), C.c_int(cap_i),
                               _p(e, c_double_p), _p(ins, c_double_p), _p(dele, c_double_p), _p(T, c_double_p),
                               _p(insd, c_double_p), _p(ints, c_i32_p), _p(st, c_double_p))
    if rc != 0:
        raise RuntimeError(f"fighost_build_model failed rc={rc}")
    L, mi = int(ints[0]), int(ints[1])
    return Model(e=e[:L].copy(), ins=ins[:L].copy(), dele=dele[:L].copy(), T=T, insd=insd[:mi].copy(), Tmin=int(ints[2]),
                 Tmax=int(ints[3]), cutoff=int(ints[4]), partial_flag=partial_flag, unmapped_flag=unmapped_flag,
                 script_itr=script_itr, max_distance=max_distance, read_length=read_length, neg_overlap=neg_overlap,
                 partial_len=partial_len, stats=(float(st[0]), float(st[1]), float(st[2])))


@dataclass
class GapBatch:
    """Host arrays behind `fig_gap_batch` (SoA + CSR)."""
    contig_off: np.ndarray
    contig_seq: np.ndarray          # uint8 ASCII, upper case
    gap_contig: np.ndarray
    gap_start: np.ndarray
    gap_len: np.ndarray
    gap_stat2: np.ndarray
    gap_fillflag: np.ndarray
    u_read_off: np.ndarray
    u_anchor_pos: np.ndarray
    u_is_reverse: np.ndarray
    u_seq_off: np.ndarray
    u_seq: np.ndarray
    p_read_off: np.ndarray
    p_clipped_index: np.ndarray
    p_match: np.ndarray
    p_pos: np.ndarray
    p_ref_pos: np.ndarray
    p_seq_off: np.ndarray
    p_seq: np.ndarray
    p_qual: np.ndarray
    gap_ot_preset: Optional[np.ndarray] = None      # uint8 [n_gaps]; None = one reference process in batch order (figbird_hip.h)

    @property
    def n_gaps(self) -> int:
        return len(self.gap_len)

    def cstruct(self) -> FigGapBatch:
        b = FigGapBatch()
        b.n_gaps = self.n_gaps
        b.n_contigs = len(self.contig_off) - 1
        b.contig_off = _p(self.contig_off, c_i64_p)
        b.contig_seq = C.cast(self.contig_seq.ctypes.data, C.c_char_p)
        b.gap_contig = _p(self.gap_contig, c_i32_p)
        b.gap_start = _p(self.gap_start, c_i64_p)
        b.gap_len = _p(self.gap_len, c_i32_p)
        b.gap_stat2 = _p(self.gap_stat2, c_i32_p)
        b.gap_fillflag = _p(self.gap_fillflag, c_i32_p)
        b.u_read_off = _p(self.u_read_off, c_i64_p)
        b.u_anchor_pos = _p(self.u_anchor_pos, c_i32_p)
        b.u_is_reverse = _p(self.u_is_reverse, c_u8_p)
        b.u_seq_off = _p(self.u_seq_off, c_i64_p)
        b.u_seq = C.cast(self.u_seq.ctypes.data, C.c_char_p)
        b.p_read_off = _p(self.p_read_off, c_i64_p)
        b.p_clipped_index = _p(self.p_clipped_index, c_i32_p)
        b.p_match = _p(self.p_match, c_i32_p)
        b.p_pos = _p(self.p_pos, c_i32_p)
        b.p_ref_pos = _p(self.p_ref_pos, c_i32_p)
        b.p_seq_off = _p(self.p_seq_off, c_i64_p)
        b.p_seq = C.cast(self.p_seq.ctypes.data, C.c_char_p)
        b.p_qual = C.cast(self.p_qual.ctypes.data, C.c_char_p)
        b.gap_ot_preset = _p(self.gap_ot_preset, c_u8_p) if self.gap_ot_preset is not None else None
        return b


@dataclass
class FillResult:
    filled_len: np.ndarray
    gaptofill: np.ndarray
    strings: List[str]
    cand: Optional[list] = None     # per gap: list of (gapEstimate, iterations, valid_count, likelihood)
    n_place: Optional[np.ndarray] = None
    counts: Optional[np.ndarray] = None    # plane (i): [n_gaps, debug_cand, plane_cols, 5] countsGap after the candidate's last E-step
    read_maxlv: Optional[np.ndarray] = None  # plane (ii): [n_gaps, debug_cand, plane_reads] per-read E-step maximum
    str_off: Optional[np.ndarray] = None   # int64[n+1]: gap g's string is raw[str_off[g]:str_off[g+1]]
    raw: Optional[np.ndarray] = None       # uint8: all gap strings back to back, as the C ABI wrote them
    draw: Optional[tuple] = None           # (draw_pos, draw_isz, draw_len) planes of fig_gap_results, when requested
    support: Optional[np.ndarray] = None   # int32 [total, 5]: read counts (A, C, G, T, other) behind raw[i], i.e. base x of gap g at str_off[g] + x
    support_origin: Optional[np.ndarray] = None   # int32 [n_gaps]: SUP_* mask (fig_gap_support::origin)
    placement: Optional["Placement"] = None   # fig_read_placement of the fill's drawn unmapped reads, when requested
    quality: Optional[tuple] = None        # (loglik float64 [total, 4], phred uint8 [total], state uint8 [n_gaps]) of fig_gap_quality, indexed like raw
    indel: Optional["Indel"] = None        # fig_gap_indel of the fill's strings and drawn unmapped reads, when requested
    polish: Optional["Polish"] = None      # fig_gap_polish of the fill's strings and drawn unmapped reads, when requested
    recruit: Optional["Recruit"] = None    # fig_read_recruit of the fill's strings and undrawn unmapped reads, when requested
    alnqual: Optional["AlnQual"] = None    # fig_gap_alnqual of the end of the chain (fill, recruit, polish), when requested
    softqual: Optional["SoftQual"] = None  # fig_gap_softqual of the fill's strings, when requested

    @property
    def filled_bases(self) -> int:
        return int(sum(len(s) - s.count("N") for s in self.strings))


class Engine:
    """One `fig_ctx` (= one GPU)."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        self.ctx = C.c_void_p()
        rc = self.lib.fig_ctx_create(device, C.byref(self.ctx))
        if rc != 0:
            raise RuntimeError(f"fig_ctx_create failed: {self.lib.fig_strerror(rc).decode()} (no CPU fallback)")
        self._keep = []
        self.n_gaps = 0
        self.cap = 0

    def close(self):
        if self.ctx:
            self.lib.fig_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.lib.fig_strerror(rc).decode()}")

    def _need(self, symbol: str, what: str):
        if not hasattr(self.lib, symbol):
            raise RuntimeError(f"{what} needs {symbol}, which this library does not export")

    def _origin_arg(self, what: str, origin):
        """the `origin` argument of fig_batch_quality / fig_batch_placement -> (the array that keeps it alive, the pointer or None)"""
        if origin is None:
            return None, None
        org = np.ascontiguousarray(origin, dtype=np.int32)
        if len(org) < self.n_gaps:
            raise ValueError(f"{what}: one origin per gap of the resident batch")
        return org, (_p(org, c_i32_p) if len(org) else None)

    def set_model(self, model: Model):
        self._model = model
        self._cm = model.cstruct()
        self._check(self.lib.fig_ctx_set_model(self.ctx, C.byref(self._cm)), "fig_ctx_set_model")

    def set_model_struct(self, cm: "FigModel"):
        """Model given as a ready `fig_model` (pointers owned by the caller, e.g. libfighost's run handle)."""
        self._model = None
        self._cm = cm
        self._check(self.lib.fig_ctx_set_model(self.ctx, C.byref(self._cm)), "fig_ctx_set_model")

    def upload(self, batch: GapBatch):
        self._batch = batch
        self._cb = batch.cstruct()
        self.n_gaps = batch.n_gaps
        self.cap = int(self.lib.fig_results_capacity(C.byref(self._cm), C.byref(self._cb)))
        self._check(self.lib.fig_batch_upload(self.ctx, C.byref(self._cb)), "fig_batch_upload")

    def _fill_resident_call(self, r: "FigGapResults", n: int, cap: int, support: bool):
        """fig_fill_resident, or fig_fill_resident_ex with a support plane sized for `cap` string bytes; returns
        (counts [cap, 5], origin [n]) or (None, None)."""
        if not support:
            self._check(self.lib.fig_fill_resident(self.ctx, C.byref(r)), "fig_fill_resident")
            return None, None
        self._need("fig_fill_resident_ex", "support=True")
        sc = np.zeros((max(cap, 1), 5), dtype=np.int32); so = np.zeros(max(n, 1), dtype=np.int32)
        s = FigGapSupport(); s.counts = _p(sc, c_i32_p); s.origin = _p(so, c_i32_p)
        self._check(self.lib.fig_fill_resident_ex(self.ctx, C.byref(r), C.byref(s)), "fig_fill_resident_ex")
        return sc, so

    def _n_ureads(self) -> int:
        """unmapped reads of the resident batch as the library counts them: none under a model that is not unmapped-mode"""
        if not self._cm.unmapped_flag or self.n_gaps <= 0 or not self._cb.u_read_off:
            return 0
        return int(self._cb.u_read_off[self.n_gaps])

    def _filled_struct(self, what: str, res: FillResult):
        """fig_gap_results of the strings and draw planes in `res` (and the arrays that keep it alive)"""
        if res.draw is None:
            raise ValueError(f"{what}: the fill result carries no draw planes (fill with draw=True)")
        n = self.n_gaps
        fl = np.ascontiguousarray(res.filled_len, dtype=np.int32); so = np.ascontiguousarray(res.str_off, dtype=np.int64)
        if len(fl) < n or len(so) < n + 1:
            raise ValueError(f"{what}: one length and one offset per gap of the resident batch")
        fl = fl if n else np.zeros(1, dtype=np.int32)
        raw = np.ascontiguousarray(res.raw, dtype=np.uint8) if res.raw is not None and len(res.raw) else np.zeros(1, dtype=np.uint8)
        dpos, disz, dlen = (np.ascontiguousarray(a, dtype=np.int32) for a in res.draw)
        dpos, disz, dlen = (a if len(a) else np.zeros(1, dtype=np.int32) for a in (dpos, disz, dlen))
        r = FigGapResults()
        r.filled_len = _p(fl, c_i32_p); r.str_off = _p(so, c_i64_p); r.str = C.cast(raw.ctypes.data, C.c_char_p); r.str_capacity = len(raw)
        r.draw_pos = _p(dpos, c_i32_p); r.draw_isz = _p(disz, c_i32_p); r.draw_len = _p(dlen, c_i32_p)
        return r, (fl, so, raw, dpos, disz, dlen)

    def placement(self, res: FillResult, origin: Optional[np.ndarray] = None) -> "Placement":
        """fig_batch_placement of the strings and draw planes in `res` against the resident batch; `origin` as for quality().
        The buffers handed to the library start as 0xFF bytes, so that an element it failed to write shows."""
        self._need("fig_batch_placement", "placement")
        r, keep = self._filled_struct("placement", res)
        n, nu = self.n_gaps, self._n_ureads()
        if len(keep[3]) < nu:
            raise ValueError("placement: one drawn offset per unmapped read of the resident batch")
        org, org_p = self._origin_arg("placement", origin)
        rp, out = self._placement_buffers(n, nu)
        self._check(self.lib.fig_batch_placement(self.ctx, C.byref(r), org_p, C.byref(rp)), "fig_batch_placement")
        return out

    @staticmethod
    def _placement_buffers(n: int, nu: int):
        """a fig_read_placement over fresh 0xFF-filled arrays for n gaps and nu unmapped reads -> (the struct, the Placement of their views)"""
        m = max(nu, 1)
        d = [np.zeros(m) for _ in range(3)]
        for a in d:
            a.view(np.uint8)[...] = 0xFF
        off = np.full(m, -1, dtype=np.int32); nv = np.full(m, -1, dtype=np.int32)
        pq = np.full(m, 0xFE, dtype=np.uint8); stt = np.full(max(n, 1), 0xFF, dtype=np.uint8)
        rp = FigReadPlacement()
        rp.ll_drawn = _p(d[0], c_double_p); rp.ll_other = _p(d[1], c_double_p); rp.sum_other = _p(d[2], c_double_p)
        rp.off_other = _p(off, c_i32_p); rp.n_valid = _p(nv, c_i32_p); rp.pq = _p(pq, c_u8_p); rp.state = _p(stt, c_u8_p)
        return rp, Placement(d[0][:nu], d[1][:nu], d[2][:nu], off[:nu], nv[:nu], pq[:nu], stt[:n])

    def softqual(self, res: FillResult, origin: Optional[np.ndarray] = None, placement: bool = False) -> "SoftQual":
        """fig_batch_softqual of the strings and draw planes in `res` against the resident batch; `origin` as for quality().
        placement=True: the fig_read_placement of the same call as well (SoftQual.placement).  The buffers handed to the library
        start as 0xFF bytes, so that an element it failed to write shows."""
        self._need("fig_batch_softqual", "softqual")
        r, keep = self._filled_struct("softqual", res)
        n, nu = self.n_gaps, self._n_ureads()
        if len(keep[3]) < nu:
            raise ValueError("softqual: one drawn offset per unmapped read of the resident batch")
        total = int(keep[1][n])
        org, org_p = self._origin_arg("softqual", origin)
        wc = np.zeros((max(total, 1), 4)); wc.view(np.uint8)[...] = 0xFF
        el = np.zeros((max(total, 1), 4)); el.view(np.uint8)[...] = 0xFF
        ph = np.full(max(total, 1), 0xFF, dtype=np.uint8); stt = np.full(max(n, 1), 0xFF, dtype=np.uint8)
        sq = FigGapSoftqual(); sq.wcount = _p(wc, c_double_p); sq.eloglik = _p(el, c_double_p); sq.phred = _p(ph, c_u8_p); sq.state = _p(stt, c_u8_p)
        rp, plc = self._placement_buffers(n, nu) if placement else (None, None)
        self._check(self.lib.fig_batch_softqual(self.ctx, C.byref(r), org_p, C.byref(rp) if placement else None, C.byref(sq)), "fig_batch_softqual")
        return SoftQual(wc[:total], el[:total], ph[:total], stt[:n], plc)

    def indel(self, res: FillResult, origin: Optional[np.ndarray] = None) -> "Indel":
        """fig_batch_indel of the strings and draw planes in `res` against the resident batch; `origin` as for quality().  The buffers
        handed to the library start as 0xFF bytes, so that an element it failed to write shows."""
        self._need("fig_batch_indel", "indel")
        r, keep = self._filled_struct("indel", res)
        n, nu = self.n_gaps, self._n_ureads()
        if len(keep[3]) < nu:
            raise ValueError("indel: one drawn offset per unmapped read of the resident batch")
        total = int(keep[1][n])
        org, org_p = self._origin_arg("indel", origin)
        m, t, gm = max(nu, 1), max(total, 1), max(n, 1)
        d = [np.zeros(m) for _ in range(2)]
        for a in d:
            a.view(np.uint8)[...] = 0xFF
        ri = [np.full(m, -1, dtype=np.int32) for _ in range(4)]
        pl = [np.full(t, -1, dtype=np.int32) for _ in range(3)]
        ie = np.full(gm, -1, dtype=np.int32)
        call = np.full(t, 0xFF, dtype=np.uint8); ce = np.full(gm, 0xFF, dtype=np.uint8); stt = np.full(gm, 0xFF, dtype=np.uint8)
        gi = FigGapIndel()
        gi.ll_flat = _p(d[0], c_double_p); gi.ll_gapped = _p(d[1], c_double_p)
        gi.n_ins, gi.n_del, gi.d_end, gi.d_start = (_p(a, c_i32_p) for a in ri)
        gi.del_reads, gi.ins_reads, gi.cover = (_p(a, c_i32_p) for a in pl)
        gi.ins_end = _p(ie, c_i32_p); gi.call = _p(call, c_u8_p); gi.call_end = _p(ce, c_u8_p); gi.state = _p(stt, c_u8_p)
        self._check(self.lib.fig_batch_indel(self.ctx, C.byref(r), org_p, C.byref(gi)), "fig_batch_indel")
        return Indel(d[0][:nu], d[1][:nu], ri[0][:nu], ri[1][:nu], ri[2][:nu], ri[3][:nu], pl[0][:total], pl[1][:total], pl[2][:total], ie[:n],
                     call[:total], ce[:n], stt[:n])

    def polish(self, res: FillResult, origin: Optional[np.ndarray] = None, max_rounds: int = 0) -> "Polish":
        """fig_batch_polish of the strings and draw planes in `res` against the resident batch; `origin` as for quality(); max_rounds
        1..8, or 0 for the library's default.  The buffers handed to the library start as 0xFF bytes, so that an element it failed
        to write shows.  `res` is not changed."""
        self._need("fig_batch_polish", "polish")
        r, keep = self._filled_struct("polish", res)
        n, nu = self.n_gaps, self._n_ureads()
        if len(keep[3]) < nu:
            raise ValueError("polish: one drawn offset per unmapped read of the resident batch")
        total = int(keep[1][n])
        org, org_p = self._origin_arg("polish", origin)
        m, t, gm = max(nu, 1), max(total, 1), max(n, 1)
        ed = np.full(t, -1, dtype=np.int32); dp = np.full(m, -1, dtype=np.int32)
        gi = [np.full(gm, -1, dtype=np.int32) for _ in range(5)]
        d = [np.zeros(gm) for _ in range(2)]
        for a in d:
            a.view(np.uint8)[...] = 0xFF
        stt = np.full(gm, 0xFF, dtype=np.uint8)
        gp = FigGapPolish()
        gp.edit = _p(ed, c_i32_p); gp.draw_pos = _p(dp, c_i32_p)
        gp.edit_end, gp.polished_len, gp.n_ins, gp.n_del, gp.rounds = (_p(a, c_i32_p) for a in gi)
        gp.ll_before = _p(d[0], c_double_p); gp.ll_after = _p(d[1], c_double_p); gp.state = _p(stt, c_u8_p)
        self._check(self.lib.fig_batch_polish(self.ctx, C.byref(r), org_p, int(max_rounds), C.byref(gp)), "fig_batch_polish")
        return Polish(ed[:total], gi[0][:n], gi[1][:n], dp[:nu], gi[2][:n], gi[3][:n], gi[4][:n], d[0][:n], d[1][:n], stt[:n], filled=res)

    def recruit(self, res: FillResult, origin: Optional[np.ndarray] = None, min_margin: float = 0.0) -> "Recruit":
        """fig_batch_recruit of the strings and draw planes in `res` against the resident batch; `origin` as for quality(); min_margin
        finite and >= 0.  The buffers handed to the library start as 0xFF bytes, so that an element it failed to write shows.  `res`
        is not changed."""
        self._need("fig_batch_recruit", "recruit")
        r, keep = self._filled_struct("recruit", res)
        n, nu = self.n_gaps, self._n_ureads()
        if len(keep[3]) < nu or len(keep[4]) < nu:
            raise ValueError("recruit: one drawn offset and one insert size per unmapped read of the resident batch")
        org, org_p = self._origin_arg("recruit", origin)
        m, gm = max(nu, 1), max(n, 1)
        d = [np.zeros(m) for _ in range(5)]
        for a in d:
            a.view(np.uint8)[...] = 0xFF
        ri = [np.full(m, -1, dtype=np.int32) for _ in range(6)]
        gi = [np.full(gm, -1, dtype=np.int32) for _ in range(2)]
        rs = np.full(m, 0xFF, dtype=np.uint8); stt = np.full(gm, 0xFF, dtype=np.uint8)
        rr = FigReadRecruit()
        rr.ll_seed, rr.ll_second, rr.ll_flat, rr.ll_gapped, rr.score = (_p(a, c_double_p) for a in d)
        rr.off_seed, rr.off_second, rr.n_valid, rr.d_end, rr.draw_pos, rr.draw_isz = (_p(a, c_i32_p) for a in ri)
        rr.n_candidates, rr.n_recruited = (_p(a, c_i32_p) for a in gi)
        rr.read_state = _p(rs, c_u8_p); rr.state = _p(stt, c_u8_p)
        self._check(self.lib.fig_batch_recruit(self.ctx, C.byref(r), org_p, C.c_double(min_margin), C.byref(rr)), "fig_batch_recruit")
        return Recruit(d[0][:nu], d[1][:nu], d[2][:nu], d[3][:nu], d[4][:nu], ri[0][:nu], ri[1][:nu], ri[2][:nu], ri[3][:nu], rs[:nu], ri[4][:nu], ri[5][:nu],
                       gi[0][:n], gi[1][:n], stt[:n], filled=res)

    def alnqual(self, res: FillResult, origin: Optional[np.ndarray] = None) -> "AlnQual":
        """fig_batch_alnqual of the strings and draw planes in `res` against the resident batch; `origin` as for quality().  The buffers
        handed to the library start as 0xFF bytes, so that an element it failed to write shows.  `res` is not changed."""
        self._need("fig_batch_alnqual", "alnqual")
        r, keep = self._filled_struct("alnqual", res)
        n, nu = self.n_gaps, self._n_ureads()
        if len(keep[3]) < nu:
            raise ValueError("alnqual: one drawn offset per unmapped read of the resident batch")
        total = int(keep[1][n])
        org, org_p = self._origin_arg("alnqual", origin)
        m, t, gm = max(nu, 1), max(total, 1), max(n, 1)
        ll = np.zeros((t, 4)); ll.view(np.uint8)[...] = 0xFF
        lg = np.zeros(m); lg.view(np.uint8)[...] = 0xFF
        pl = [np.full(t, -1, dtype=np.int32) for _ in range(3)]
        ri = [np.full(m, -1, dtype=np.int32) for _ in range(4)]
        ph = np.full(t, 0xFF, dtype=np.uint8); stt = np.full(gm, 0xFF, dtype=np.uint8)
        aq = FigGapAlnqual()
        aq.loglik = _p(ll, c_double_p); aq.ll_gapped = _p(lg, c_double_p)
        aq.depth, aq.agree, aq.skip = (_p(a, c_i32_p) for a in pl)
        aq.n_ins, aq.n_del, aq.d_end, aq.d_start = (_p(a, c_i32_p) for a in ri)
        aq.phred = _p(ph, c_u8_p); aq.state = _p(stt, c_u8_p)
        self._check(self.lib.fig_batch_alnqual(self.ctx, C.byref(r), org_p, C.byref(aq)), "fig_batch_alnqual")
        return AlnQual(ll[:total], pl[0][:total], pl[1][:total], pl[2][:total], ph[:total], lg[:nu], ri[0][:nu], ri[1][:nu], ri[2][:nu], ri[3][:nu], stt[:n],
                       filled=res)

    def quality(self, res: FillResult, origin: Optional[np.ndarray] = None, placement: Optional["Placement"] = None, min_pq: Optional[int] = None):
        """fig_batch_quality of the strings and draw planes in `res` against the resident batch; `origin` is
        FillResult.support_origin, or None for no origin test.  Returns (loglik [total, 4], phred [total], state [n_gaps]) with
        total = str_off[n_gaps]: base x of gap g at str_off[g] + x.  The buffers handed to the library start as 0xFF bytes, so
        that an element it failed to write shows.  placement=P, min_pq=k: the call sees a copy of the draw plane in which the
        scored reads of P with pq < k are not drawn (INT32_MIN)."""
        if (placement is None) != (min_pq is None):
            raise ValueError("quality: placement and min_pq go together")
        if placement is not None and res.draw is not None:
            dpos = np.array(res.draw[0], dtype=np.int32)
            pq = np.asarray(placement.pq)
            drop = np.flatnonzero((pq != PLACE_NONE) & (pq < min_pq))
            dpos[drop] = np.iinfo(np.int32).min
            res = dc_replace(res, draw=(dpos, res.draw[1], res.draw[2]))
        self._need("fig_batch_quality", "quality")
        r, keep = self._filled_struct("quality", res)
        n = self.n_gaps
        total = int(keep[1][n])
        org, org_p = self._origin_arg("quality", origin)
        ll = np.full((max(total, 1), 4), np.nan); ll.view(np.uint8)[...] = 0xFF
        ph = np.full(max(total, 1), 0xFF, dtype=np.uint8); stt = np.full(max(n, 1), 0xFF, dtype=np.uint8)
        gq = FigGapQuality(); gq.loglik = _p(ll, c_double_p); gq.phred = _p(ph, c_u8_p); gq.state = _p(stt, c_u8_p)
        self._check(self.lib.fig_batch_quality(self.ctx, C.byref(r), org_p, C.byref(gq)), "fig_batch_quality")
        return ll[:total], ph[:total], stt[:n]

    def _implied(self, support: bool, draw: bool, quality: bool, placement: bool, softqual: bool = False, indel: bool = False, polish: bool = False,
                 recruit: bool = False, alnqual: bool = False):
        """quality, placement, softqual, indel, polish, recruit and alnqual need their calls, the draw planes and the support call (for the origins) -> (draw, support)"""
        if recruit:
            self._need("fig_batch_recruit", "recruit=True")
            draw = support = True
        if alnqual:
            self._need("fig_batch_alnqual", "alnqual=True")
            draw = support = True
        if polish:
            self._need("fig_batch_polish", "polish=True")
            draw = support = True
        if quality:
            self._need("fig_batch_quality", "quality=True")
        if placement:
            self._need("fig_batch_placement", "placement=True")
        if softqual:
            self._need("fig_batch_softqual", "softqual=True")
        if indel:
            self._need("fig_batch_indel", "indel=True")
        return draw or quality or placement or softqual or indel, support or quality or placement or softqual or indel

    def _result_arrays(self, n: int, cap: int, nr: Optional[int], draw: bool):
        """Fresh result arrays for n gaps and cap string bytes and, unless nr is None, draw planes for nr reads, behind a
        fig_gap_results that carries the planes iff `draw` -> (r, filled_len, gaptofill, str_off, str, planes or None)"""
        fl = np.zeros(max(n, 1), dtype=np.int32); gt = np.zeros(max(n, 1), dtype=np.int32)
        so = np.zeros(n + 1, dtype=np.int64); st = np.zeros(max(cap, 1), dtype=np.uint8)
        r = FigGapResults()
        r.filled_len = _p(fl, c_i32_p); r.gaptofill = _p(gt, c_i32_p); r.str_off = _p(so, c_i64_p)
        r.str = C.cast(st.ctypes.data, C.c_char_p); r.str_capacity = len(st)
        planes = None
        if nr is not None:
            planes = (np.full(max(nr, 1), np.iinfo(np.int32).min, dtype=np.int32), np.zeros(max(nr, 1), dtype=np.int32), np.full(max(2 * n, 1), -1, dtype=np.int32))
        if draw:
            r.draw_pos = _p(planes[0], c_i32_p); r.draw_isz = _p(planes[1], c_i32_p); r.draw_len = _p(planes[2], c_i32_p)
        return r, fl, gt, so, st, planes

    def _post_fill(self, filled: FillResult, placement: bool, quality: bool, min_pq: Optional[int] = None, softqual: bool = False, indel: bool = False):
        """the passes beside a fill whose batch is still resident, with its origins -> (Placement or None, quality or None, SoftQual or
        None, Indel or None)"""
        plc = self.placement(filled, filled.support_origin) if placement else None
        qual = None
        if quality:
            qual = self.quality(filled, filled.support_origin, placement=plc if min_pq is not None else None, min_pq=min_pq)
        return plc, qual, (self.softqual(filled, filled.support_origin) if softqual else None), (self.indel(filled, filled.support_origin) if indel else None)

    def fill_resident(self, debug_cand: int = 0, plane_cols: int = 0, plane_reads: int = 0, support: bool = False, draw: bool = False, quality: bool = False,
                      placement: bool = False, softqual: bool = False, indel: bool = False, polish: bool = False, recruit: bool = False,
                      recruit_margin: float = 0.0, alnqual: bool = False) -> FillResult:
        """quality=True implies draw=True and support=True and also fills FillResult.quality (fig_batch_quality with the origins);
        placement=True likewise fills FillResult.placement (fig_batch_placement with the origins), softqual=True
        FillResult.softqual (fig_batch_softqual with the origins), indel=True FillResult.indel (fig_batch_indel with the origins),
        polish=True FillResult.polish (fig_batch_polish with the origins), recruit=True FillResult.recruit (fig_batch_recruit with the
        origins and recruit_margin; the other passes see the fill's own draw planes), alnqual=True FillResult.alnqual
        (fig_batch_alnqual with the origins, on the end of the chain: Recruit.result() with recruit=True, Polish.result() with
        polish=True)."""
        draw, support = self._implied(support, draw, quality, placement, softqual, indel, polish, recruit, alnqual)
        n = self.n_gaps
        nr = int(self._batch.u_read_off[-1]) + int(self._batch.p_read_off[-1]) if draw else None
        r, fl, gt, so, st, planes = self._result_arrays(n, self.cap, nr, draw)
        if debug_cand > 0:
            dn = np.zeros(max(n, 1), dtype=np.int32); di = np.zeros(max(n, 1) * debug_cand * 3, dtype=np.int32)
            dl = np.zeros(max(n, 1) * debug_cand)
            dp = np.zeros(max(n, 1), dtype=np.int32)
            r.dbg_max_cand = debug_cand; r.dbg_n_cand = _p(dn, c_i32_p); r.dbg_cand_i = _p(di, c_i32_p); r.dbg_cand_lik = _p(dl, c_double_p); r.dbg_n_place = _p(dp, c_i32_p)
            if plane_cols > 0:
                pc = np.zeros((max(n, 1), debug_cand, plane_cols, 5))
                r.dbg_plane_cols = plane_cols; r.dbg_counts = _p(pc, c_double_p)
            if plane_reads > 0:
                pr = np.zeros((max(n, 1), debug_cand, plane_reads))
                r.dbg_plane_reads = plane_reads; r.dbg_read_maxlv = _p(pr, c_double_p)
        sup_c, sup_o = self._fill_resident_call(r, n, len(st), support)
        raw = st.tobytes()
        strings = [raw[so[g]:so[g + 1]].decode() for g in range(n)]
        cand = None
        if debug_cand > 0:
            cand = []
            for g in range(n):
                k = min(int(dn[g]), debug_cand)
                base = g * debug_cand
                cand.append([(int(di[(base + j) * 3]), int(di[(base + j) * 3 + 1]), int(di[(base + j) * 3 + 2]), float(dl[base + j])) for j in range(k)])
        res = FillResult(fl[:n].copy(), gt[:n].copy(), strings, cand, str_off=so, raw=st)
        res.n_place = dp[:n].copy() if debug_cand > 0 else None
        if debug_cand > 0 and plane_cols > 0:
            res.counts = pc[:n]
        if debug_cand > 0 and plane_reads > 0:
            res.read_maxlv = pr[:n]
        if draw:
            res.draw = (planes[0][:nr], planes[1][:nr], planes[2][:2 * n])
        if support:
            res.support = sup_c[:int(so[n])]; res.support_origin = sup_o[:n]
        res.placement, res.quality, res.softqual, res.indel = self._post_fill(res, placement, quality, softqual=softqual, indel=indel)
        if polish:
            res.polish = self.polish(res, res.support_origin)
        if recruit:
            res.recruit = self.recruit(res, res.support_origin, recruit_margin)
        if alnqual:
            end = res.polish.result() if polish else res.recruit.result() if recruit else res
            res.alnqual = self.alnqual(end, res.support_origin)
        return res

    def free_batch(self):
        self.lib.fig_batch_free(self.ctx)

    def probe_reach(self) -> np.ndarray:
        """uint8[n_gaps] of the resident batch: 1 = the gap's candidate loop gets to Figbird.cpp:6317 (fig_batch_probe_reach)."""
        r = np.zeros(max(self.n_gaps, 1), dtype=np.uint8)
        if self.n_gaps > 0:
            self._check(self.lib.fig_batch_probe_reach(self.ctx, _p(r, c_u8_p)), "fig_batch_probe_reach")
        return r[:self.n_gaps]

    def set_ot_preset(self, preset: np.ndarray):
        """Replace `gap_ot_preset` of the resident batch (fig_batch_set_ot_preset)."""
        a = np.ascontiguousarray(preset, dtype=np.uint8)
        if len(a) != self.n_gaps:
            raise ValueError("set_ot_preset: one entry per gap of the resident batch")
        if self.n_gaps > 0:
            self._check(self.lib.fig_batch_set_ot_preset(self.ctx, _p(a, c_u8_p)), "fig_batch_set_ot_preset")

    def upload_struct(self, cbatch: "FigGapBatch"):
        """fig_batch_upload of a caller-built `fig_gap_batch` (e.g. a shard view from libfighost's run handle)."""
        self._cb = cbatch
        self.n_gaps = int(cbatch.n_gaps)
        self.cap = int(self.lib.fig_results_capacity(C.byref(self._cm), C.byref(cbatch))) if self.n_gaps > 0 else 1
        if self.n_gaps > 0:
            self._check(self.lib.fig_batch_upload(self.ctx, C.byref(cbatch)), "fig_batch_upload")

    def fill_struct(self, cbatch: "FigGapBatch", n_ureads: int, n_preads: int, draw: bool = True, resident: bool = False, support: bool = False, quality: bool = False,
                    keep_resident: bool = False, placement: bool = False, min_pq: Optional[int] = None, softqual: bool = False, indel: bool = False,
                    polish: bool = False, polish_rounds: int = 0, recruit: bool = False, recruit_margin: float = 0.0,
                    alnqual: bool = False) -> FillResult:
        """fig_fill_gaps on a caller-built `fig_gap_batch` (e.g. a shard view from libfighost's run handle), with the
        per-read draw planes; returns a FillResult whose `draw` field holds (draw_pos, draw_isz, draw_len).
        resident=True: the batch was uploaded with upload_struct (fig_fill_resident + fig_batch_free).  support=True: the per-base
        read support as well (fields `support`, `support_origin`).  quality=True implies draw and support and runs
        fig_batch_quality before the batch is freed (field `quality`).  keep_resident=True leaves an uploaded batch resident
        for a further call.  placement=True likewise runs fig_batch_placement (field `placement`); with min_pq as well the
        quality leaves out the scored reads below that pq (Engine.quality).  softqual=True likewise runs fig_batch_softqual (field
        `softqual`), indel=True fig_batch_indel (field `indel`), polish=True fig_batch_polish with polish_rounds (field `polish`),
        recruit=True fig_batch_recruit with recruit_margin (field `recruit`): the indel pass and the polish then see the merged draw
        planes (Recruit.result()), every other pass the fill's own.  alnqual=True runs fig_batch_alnqual (field `alnqual`) on the end
        of that chain: the merged planes after a recruit, Polish.result() after a polish."""
        draw, support = self._implied(support, draw, quality, placement or min_pq is not None, softqual, indel, polish, recruit, alnqual)
        placement = placement or min_pq is not None
        qual = plc = sq = ind = pol = rec = alq = None
        n = int(cbatch.n_gaps)
        cap = int(self.lib.fig_results_capacity(C.byref(self._cm), C.byref(cbatch))) if n > 0 else 1
        nr = n_ureads + n_preads
        r, fl, gt, so, st, (dpos, disz, dlen) = self._result_arrays(n, cap, nr, draw)
        sup_c = sup_o = None
        if support:
            self._need("fig_fill_resident_ex", "support=True")
        if n > 0 and not resident and support:            # (fig_fill_gaps has no support argument: upload, then the resident call)
            self._check(self.lib.fig_batch_upload(self.ctx, C.byref(cbatch)), "fig_batch_upload")
            resident = True
        if n > 0 and resident:
            try:
                sup_c, sup_o = self._fill_resident_call(r, n, len(st), support)
                own = FillResult(fl, gt, None, str_off=so, raw=st, draw=(dpos, disz, dlen), support_origin=sup_o)
                if placement or quality or softqual or (indel and not recruit):
                    self.n_gaps = n; self._cb = cbatch
                    plc, qual, sq, ind = self._post_fill(own, placement, quality, min_pq, softqual, indel and not recruit)
                merged = own
                if recruit:
                    self.n_gaps = n; self._cb = cbatch
                    rec = self.recruit(own, sup_o, recruit_margin)
                    merged = rec.result()
                    if indel:
                        ind = self.indel(merged, sup_o)
                if polish:
                    self.n_gaps = n; self._cb = cbatch
                    pol = self.polish(merged, sup_o, polish_rounds)
                if alnqual:
                    self.n_gaps = n; self._cb = cbatch
                    alq = self.alnqual(pol.result() if polish else merged, sup_o)
            finally:
                if not keep_resident:
                    self.lib.fig_batch_free(self.ctx)
        elif n > 0:
            self._check(self.lib.fig_fill_gaps(self.ctx, C.byref(cbatch), C.byref(r)), "fig_fill_gaps")
        res = FillResult(fl[:n].copy(), gt[:n].copy(), None, None, str_off=so, raw=st)
        res.draw = (dpos[:nr], disz[:nr], dlen[:2 * n])
        if support:
            res.support = sup_c[:int(so[n])] if sup_c is not None else np.zeros((0, 5), dtype=np.int32)
            res.support_origin = sup_o[:n] if sup_o is not None else np.zeros(0, dtype=np.int32)
        if quality:
            res.quality = qual if qual is not None else (np.zeros((0, 4)), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
        if placement:
            z = np.zeros(0)
            res.placement = plc if plc is not None else Placement(z, z, z, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
        if softqual:
            res.softqual = sq if sq is not None else SoftQual(np.zeros((0, 4)), np.zeros((0, 4)), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
        if indel:
            zi, zb = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8)
            res.indel = ind if ind is not None else Indel(np.zeros(0), np.zeros(0), zi, zi, zi, zi, zi, zi, zi, zi, zb, zb, zb)
        if polish:
            zi = np.zeros(0, dtype=np.int32)
            res.polish = pol if pol is not None else Polish(zi, zi, zi, zi, zi, zi, zi, np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8), filled=res)
        if recruit:
            zi, zb, zd = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0)
            res.recruit = rec if rec is not None else Recruit(zd, zd, zd, zd, zd, zi, zi, zi, zi, zb, zi, zi, zi, zi, zb, filled=res)
        if alnqual:
            zi, zb, zd = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0)
            res.alnqual = alq if alq is not None else AlnQual(np.zeros((0, 4)), zi, zi, zi, zb, zd, zi, zi, zi, zi, zb, filled=res)
        return res

    def fill(self, batch: GapBatch, debug_cand: int = 0, plane_cols: int = 0, plane_reads: int = 0, support: bool = False, draw: bool = False, quality: bool = False,
             placement: bool = False, softqual: bool = False, indel: bool = False, polish: bool = False, recruit: bool = False,
             recruit_margin: float = 0.0, alnqual: bool = False) -> FillResult:
        self.upload(batch)
        try:
            return self.fill_resident(debug_cand, plane_cols, plane_reads, support, draw, quality, placement, softqual, indel, polish, recruit, recruit_margin, alnqual)
        finally:
            self.free_batch()

    def stats(self) -> dict:
        s = FigStats()
        self.lib.fig_get_stats(self.ctx, C.byref(s))
        return {k: getattr(s, k) for k, _ in FigStats._fields_}
