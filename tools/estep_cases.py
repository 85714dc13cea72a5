#!/usr/bin/env python3
"""Directed cases for the shared-factor form of the unmapped E-step (figbird_amd/csrc/fig_engine_shared.h), next to the random
generator of tools/fuzz_ref.py.  Every case is synth.make_case plus an edit: the reads of a gap cut to an exact count, N
bases written into chosen mates, a gap moved to the contig start.  All are unmapped mode (two partial-mode cases pin
fig_partial_fast's copy of the contig-start guard) with read counts small enough that the CPU oracle takes about a second.

The arithmetic of fig_hot_estep_sh's phase A (which fig_sh_unit<NS> instantiation the left-over (chunk, tile) items of a
super-chunk run in) and the predicate of fig_sh_applies are restated here in integers, so that the tests can say which code
a case reaches without running it (tests/test_estep_forms.py).

  python3 tools/estep_cases.py            # list the cases, their read counts and the split instantiations they reach
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from figbird_amd import synth  # noqa: E402

FIG_SH_C, FIG_SH_SC = 32, 4          # fig_types.h: reads per chunk, chunks per super-chunk
CLASS_CAPS = (448, 1216, 1600)       # fig_pack.h, ClsDef defs[]: longest candidate (columns) of the 256- and the 512-thread classes

READ_COUNTS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 257]      # dimension a
CHUNK_REPEATS = [(33, 1), (33, 2), (33, 3), (129, 1), (129, 2), (129, 3)]         # (reads, FIG_SH_CHUNKS) repeated on both gaps
A_GAPS = {405: 256, 500: 512}        # gap length -> threads of its launch class (7 tiles x 4 waves, 9 tiles x 8 waves at L = 36)
N_SLOTS = {                          # dimension b: which of the 70 reads carry an N base
    "slot0": [0], "slot31": [31], "slot32": [32], "rowgroup": [8, 9, 10, 11], "chunk1": list(range(32, 64)), "last": [69],
    "all": list(range(70)),
}
E_STARTS = {"Lm2": -2, "Lm1": -1, "L": 0, "60": None}       # dimension e: gap start relative to L (None: at 60)


# ---- the integer arithmetic of the device code, restated ---------------------------------------------------------------------
def nt_of_class(gmax):
    """Threads of the launch class of a gap whose longest candidate is gmax columns (fig_pack.h, defs[])."""
    return 256 if gmax <= CLASS_CAPS[0] else 512


def split_plan(nU, G, L, nt, chunks=FIG_SH_SC):
    """fig_hot_estep_sh, phase A (fig_engine_shared.h:309-331): per super-chunk (nT, nc, nfull, mleft, fsplit); fsplit = 0 when
    no item is left over, else the left-over items run fig_sh_unit<32 / fsplit>."""
    nw = nt // 64
    Wn = G + L - 1
    nT = (Wn + 63) >> 6
    scn = max(1, min(FIG_SH_SC, chunks))
    out = []
    for c0 in range(0, nU, scn * FIG_SH_C):
        nrd = min(nU - c0, scn * FIG_SH_C)
        nc = (nrd + FIG_SH_C - 1) // FIG_SH_C
        nit = nT * nc
        nfull = nit // nw
        mleft = nit - nfull * nw
        fsplit = 0
        if mleft > 0:
            fsplit = 1
            while fsplit * 2 * mleft <= nw and fsplit < 8:
                fsplit *= 2
        out.append((nT, nc, nfull, mleft, fsplit))
    return out


def sh_applies(G, L, nt, nteams, gap_start, D, estep_pair=False):
    """fig_sh_applies (fig_engine_shared.h:573-579) for an LDS class without tiles: may the E-step of candidate length G take
    the shared-factor form?  S.left is min(D, gap start) (fig_engine.h:425), xoff = L - 1, cpl as fig_hot_estep_dispatch
    computes it (fig_engine_hot.h:857-859).  The capW term holds by construction whenever nteams >= 4 (fig_pack.h:283)."""
    nw = nt // 64
    cpl = ((G + 63) // 64 + (nw >> 2) - 1) // (nw >> 2)
    if estep_pair or nteams < 4 or cpl > 8 or cpl < 1 or L < 32:
        return False
    if min(D, gap_start) < L - 1:
        return False
    return G + L - 1 <= 2 * nt


# ---- case edits --------------------------------------------------------------------------------------------------------------
def truncate(case, gi, n):
    g = case.gaps[gi]
    assert len(g.unmapped) >= n, (case.name, gi, len(g.unmapped), n)
    g.unmapped = g.unmapped[:n]
    return case


def write_n(case, gi, slots, at=None):
    """An N base into the mates `slots` of gap gi (position `at`, default: one that moves with the slot)."""
    g = case.gaps[gi]
    for s in slots:
        r = g.unmapped[s]
        j = (7 * s + 3) % len(r.mate_seq_fastq) if at is None else at
        r.mate_seq_fastq = r.mate_seq_fastq[:j] + "N" + r.mate_seq_fastq[j + 1:]
    return case


def drop_gap(case, gi):
    """The case without gap gi: its N run gets the true sequence back (every N run of a scaffold needs its gapInfo line)."""
    g = case.gaps[gi]
    assert len(g.truth) == g.length
    s = case.scaffolds[0]
    case.scaffolds[0] = s[:g.start] + g.truth + s[g.start + g.length:]
    del case.gaps[gi]
    return case


def _one_gap(name, seed, g0, L, n, start=1500, insert=600.0, coverage=30.0, **kw):
    c = synth.make_case(name, seed, "unmapped", [(start, g0)], contig_len=start + g0 + 1500, read_len=L, insert_mean=insert, insert_sd=30,
                        coverage=coverage, err=0.005, n_model_pairs=400, partial_reads_in_unmapped=False, **kw)
    return truncate(c, 0, n)


# ---- the dimensions ----------------------------------------------------------------------------------------------------------
def case_a(g0, n):
    """a. read count: one gap of 405 bp (256 threads, 7 tiles) or 500 bp (512 threads, 9 tiles) at L = 36 with exactly n reads."""
    return _one_gap(f"a{g0}_{n}", 1000 + g0, g0, 36, n)


def case_b(which):
    """b. irregular reads: the 405-bp gap with 70 reads, N bases in the mates N_SLOTS[which]."""
    return write_n(_one_gap(f"b_{which}", 1405, 405, 36, 70), 0, N_SLOTS[which])


def case_c(n):
    """c. a 12-bp gap at L = 36 with n reads: a candidate sweep up to 70 columns (Wn just over one tile of 64 placements)."""
    return _one_gap(f"c12_{n}", 1012, 12, 36, n, coverage=70.0)


def case_d(nt):
    """d. form boundary, one candidate each: L = 101, gaps of 412 | 413 bp (Wn = 512 | 513, 256 threads) or 924 | 925 bp
    (Wn = 1024 | 1025, 512 threads) in one batch, about 30 reads each."""
    a, b = (412, 413) if nt == 256 else (924, 925)
    c = synth.make_case(f"d{nt}", 2000 + nt, "unmapped", [(1500, a), (1500 + a + 1800, b)], contig_len=1500 + a + 1800 + b + 1800, read_len=101,
                        insert_mean=700.0, insert_sd=30, coverage=12.0 if nt == 256 else 6.0, err=0.005, n_model_pairs=400, partial_reads_in_unmapped=False)
    for gi in (0, 1):
        truncate(c, gi, min(30, len(c.gaps[gi].unmapped)))
    return c


def case_e(which, mode="unmapped"):
    """e. contig start: one 420-bp gap at L = 36 whose gap start is L - 2, L - 1, L or 60 (S.left < xoff = L - 1 is the guard of
    fig_sh_applies; gap start L - 2 is the one that must fall back).  mode "partial": a 40-bp gap with the same starts, for the
    identical guard of fig_partial_fast (fig_engine_partial.h:212)."""
    L = 36
    start = 60 if E_STARTS[which] is None else L + E_STARTS[which]
    if mode == "partial":
        return synth.make_case(f"e_p{which}", 3100, "partial", [(start, 40)], contig_len=start + 40 + 1500, read_len=L, insert_mean=180.0, insert_sd=10,
                               coverage=30.0, err=0.005, n_model_pairs=400)
    return _one_gap(f"e_{which}", 3000, 420, L, 60, start=start)


F_MATE = 1200


def case_f(with_mate):
    """f. batch-mates: a 600-bp gap at L = 200, alone or in one batch with a gap of F_MATE bp (same launch class, whose geometry
    follows its longest gap).  Both variants come from ONE make_case, so the 600-bp gap and the model are the same."""
    c = synth.make_case("f_mate" if with_mate else "f_alone", 4000, "unmapped", [(1500, 600), (4000, F_MATE)], contig_len=4000 + F_MATE + 1800, read_len=200,
                        insert_mean=700.0, insert_sd=30, coverage=12.0, err=0.005, n_model_pairs=400, partial_reads_in_unmapped=False)
    for gi in (0, 1):
        truncate(c, gi, min(40, len(c.gaps[gi].unmapped)))
    return c if with_mate else drop_gap(c, 1)


def all_cases():
    """{id: builder} of every directed case (the CPU suite runs a-e against the oracle; the GPU suite runs them all)."""
    out = {}
    for g0 in A_GAPS:
        for n in READ_COUNTS:
            out[f"a{g0}_{n}"] = (lambda g0=g0, n=n: case_a(g0, n))
    for w in N_SLOTS:
        out[f"b_{w}"] = (lambda w=w: case_b(w))
    for n in (33, 65):
        out[f"c12_{n}"] = (lambda n=n: case_c(n))
    for nt in (256, 512):
        out[f"d{nt}"] = (lambda nt=nt: case_d(nt))
    for w in E_STARTS:
        out[f"e_{w}"] = (lambda w=w: case_e(w))
    for w in ("Lm2", "Lm1"):
        out[f"e_p{w}"] = (lambda w=w: case_e(w, "partial"))
    out["f_alone"] = lambda: case_f(False)
    out["f_mate"] = lambda: case_f(True)
    return out


if __name__ == "__main__":
    for cid, mk in all_cases().items():
        c = mk()
        info = []
        for g in c.gaps:
            nt = nt_of_class(g.length)
            n = len(g.unmapped) if c.mode == "unmapped" else len(g.partial)
            sp = sorted(set(32 // p[4] if p[4] else 0 for p in split_plan(n, g.length, c.read_len, nt))) if c.mode == "unmapped" else []
            info.append(f"G0={g.length} start={g.start} reads={n} units={sp}")
        print(cid, c.mode, f"L={c.read_len}", "; ".join(info))
