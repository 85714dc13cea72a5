#!/usr/bin/env python3
"""Directed cases for the search paths of the MLE pass (fig_hot_mle, figbird_amd/csrc/fig_engine_hot.h), next to
tools/estep_cases.py and tools/partial_cases.py.

The pass finds, per unmapped read, the placement with the greatest product ("first maximum wins", in the reference's
order), and it does so by pruning: hints, a 32-base record sweep and at most two deferred survivors per read in the
lane-per-read path; a swept filter, pruned pair-chain rounds with a survivor hand-over, or a plain chain (reads with N) in
the wave-per-read path.  Random sequence almost never gives a read a second placement near the maximum, so a search that
just returns its hint passes every random case.  The cases here are built so that it does not:

  a  tandem gaps: the truth between start - 3p and start + G0 + 3p is a repeat of period p, so placements one period apart
     have bit-equal products and reads have 0, 1, 2 and more survivors beyond their hints
  b  the same on read lengths either side of the 32-base words and records; reads shorter than the model's L mixed in
  c  reads with N (plain chain) among full-length reads; read counts either side of a wave and of a workgroup
  d  gaps of at most 30 bp (the ucoverf / umaxleftf / umaxrightf flags), N-free reads and reads with an N
  e  error models from 0.5 % to 85 %, one whose best products lie below 1e-290, one that is not monotone
  f  one-candidate gaps in every memory form behind fig_mle_dispatch

Every case is synth.make_case plus an edit, written and read through the normal files; the model comes from the case's own
myout.sam.  The predicates of the pass (fig_engine_hot.h:979-996, :1571-1572) and of fig_model_fmm (fig_pack.h:49-63) are
restated here in integers, so that a test can say which form a case reaches (tests/test_mle_forms.py).

  python3 tools/mle_cases.py            # per case: reads, routes, oracle seconds, restated predicates (class table of fig_pack.h)
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from figbird_amd import synth  # noqa: E402
from tools import estep_cases as ec  # noqa: E402
from tools import partial_cases as pc  # noqa: E402

FIG_MLE_FB = 208                     # fig_types.h: doubles of the per-wave factor buffer
TANDEM_FLANK = 3                     # periods of the repeat that reach into either flank

# a: name -> (G0, period, error rate, seed).  Up to 133 bp the candidates end at 3 L = 108 columns, so a 120-bp gap can only be
# filled shorter by whole periods; the seeds are ones at which the oracle's fill stays periodic across the gap's ends, so that the
# ties can be read off its string (tests/test_mle_forms.py: twins)
A_TANDEMS = {"p7": (90, 7, 0.005, 5007), "p20": (100, 20, 0.005, 5020), "p20_e8": (120, 20, 0.08, 5020), "p40": (90, 40, 0.005, 5042), "p50": (120, 50, 0.005, 5050)}
B_LENGTHS = [31, 32, 33, 47, 48, 49, 63, 64, 65]
C_COUNTS = {"t": (100, [63, 64, 65]), "w256": (405, [1, 255, 256, 257]), "w512": (500, [511, 512, 513])}
D_GAPS = [12, 20, 30]
D_N_SLOTS = [0, 5, 33]
E_RATES = {"e005": 0.005, "e08": 0.08, "e30": 0.30, "e60": 0.60, "e85": 0.85}
E_BIASED = ("e60", "e85")            # every substitution of one type per base, so that fmm_up = e (>= 0.5), not e / 3
B_MATE = 420                         # b: a one-candidate gap beside the 60-bp one, so that the class has room for the filter's tables
B_SHORT = {3: 1, 10: 2, 17: 5, 24: 4, 31: 3, 38: 16, 45: 1, 52: 7}      # slot -> bases cut off the mate
C_SHORT = {1: 2, 40: 3, 68: 5}       # c: three shorter mates as well (the oracle accepts no read with N here, so these are the wave path's accepted reads)
NONMONO_AT = (10, 22)                # the read positions that get e = del = 1 in the non-monotone model


def b_period(L):
    """b: period 7 up to L = 49; 20 from L = 63 (where the oracle's fill of the period-7 gap keeps an N core, so no tie can be read off it)."""
    return 7 if L < 60 else 20


# ---- the arithmetic of the device code, restated -----------------------------------------------------------------------------
def model_fmm(model):
    """fig_model_fmm (fig_pack.h:49-63): the upper bound of a mismatch factor, 2.0 for a model with a factor outside [0, 1]."""
    e, ins, dele, T = (np.asarray(x, dtype=np.float64) for x in (model.e, model.ins, model.dele, model.T))
    m3 = 1 - e - ins - dele
    if not (((e >= 0) & (e <= 1) & (m3 >= 0) & (m3 <= 1)).all() and ((T >= 0) & (T <= 1)).all()):
        return 2.0
    tmax = max(T[f * 5 + t] for f in range(5) for t in range(4) if f != t)
    f = float(e.max()) * float(tmax) * (1.0 + 1e-9)
    if not f > 0:
        f = 1.0
    return f if f < 1.0 else 1.0


def tiled_mle_doubles(ncolE, nw):
    """FIG_TILED_MLE_DOUBLES (fig_types.h:23)."""
    return 7 * ncolE + nw * FIG_MLE_FB + (ncolE + 15) // 16 + 16 + 8


def mle_form(cls, G, fmm, state_bytes=pc.STATE_BYTES):
    """The memory form of one MLE pass over a candidate of G columns in a launch class `cls` (the fields of the library's
    `[figsched] class:` line: capGl, ncolE, Wcap, nt, nteams, lds_tab, tiles, tile_cols) under a model with fig_model_fmm = fmm
    -> dict(lds, use_serial, nci_lds, use_kf, lane_path).  fig_mle_dispatch (:1571-1572) picks the template argument and, in the
    tiled class, the "one weight row" behind the records; fig_hot_mle (:979-996) the rest.  lds_tw: fig_eng_carve (fig_engine.h)."""
    nw = cls["nt"] // 64
    ncolE, nteams, Wcap = cls["ncolE"], cls["nteams"], cls["Wcap"]
    if cls["tiles"] > 0:
        fixed = state_bytes + cls["capGl"] + pc.FIG_MAX_READLEN + 64 + pc.FIG_PLB_BYTES
        tiled_max = (pc.LDS_MAX - fixed) // 8
        mle = tiled_mle_doubles(ncolE, nw)
        lds_tw = 9 * cls["tile_cols"] + nteams * Wcap
        if lds_tw < mle <= tiled_max:
            lds_tw = mle
        lds = mle <= lds_tw
        if lds:
            nteams, Wcap = 1, lds_tw - 7 * ncolE
    else:
        lds = bool(cls["lds_tab"])
    nrows = min(nteams, nw)
    use_serial = nrows * Wcap >= nw * FIG_MLE_FB
    fb = nw * FIG_MLE_FB if use_serial else 0
    nci = (5 * G + 1) // 2 + 1
    nci_lds = lds and nrows * Wcap - fb >= nci
    kwords = (ncolE + 15) // 16 + 16
    use_kf = lds and fmm < 0.5 and nrows * Wcap - fb - (nci if nci_lds else 0) >= kwords + 1
    return dict(lds=lds, use_serial=use_serial, nci_lds=nci_lds, use_kf=use_kf, lane_path=use_kf and fmm <= 1.0)


def with_tile_cols(cls, L):
    """A class of partial_cases.class_table with the tile_cols field of the library's log line (fig_pack.h:260-261)."""
    step = ((cls["ncolE"] + cls["tiles"] - 1) // cls["tiles"] + 7) & ~7 if cls["tiles"] else 0
    return dict(cls, tile_cols=(step + L + 8 + 7) & ~7 if cls["tiles"] else 0)


def gmax_unmapped(G0, partial_len, unm_limit=400):
    """Longest candidate (columns) of an unmapped-mode gap: gap_alloc of fig_gaprules.h (float32 as there) and fig_pack.h:218-220,
    where the probes of checkGapReads (70 columns below 30 bp, else 3 G0) count up to the gap's allocation."""
    factor = 3 * partial_len
    if G0 <= unm_limit // 3:
        f2, alloc = np.float32(factor) / np.float32(G0), factor * 3
    elif G0 <= unm_limit:
        f2, alloc = np.float32(2.5), G0 * 3
    else:
        f2, alloc = np.float32(1.0), G0
    gm = max(G0, int(np.float32(G0) * f2))
    if G0 <= unm_limit:
        gm = max(gm, 70 if G0 < 30 else 3 * G0)
    return min(gm, alloc)


def probe_lengths(G0):
    """The gap lengths checkGapReads probes before the candidate loop (Figbird.cpp:6121-6153): all of them when no probe places
    enough reads, which is also when the loop never starts."""
    if G0 < 30:
        return list(range(0, 80, 10 if G0 < 15 else 20))
    return [G0 // 2, G0, 2 * G0, 3 * G0]


def classes_of(case):
    """The launch classes of a case as fig_pack.h lays them out (partial_cases.class_table), with tile_cols -> ([class], class per gap)."""
    classes, cls_of = pc.class_table([gmax_unmapped(g.length, case.partial_len) for g in case.gaps], case.read_len)
    return [with_tile_cols(c, case.read_len) for c in classes], cls_of


def emu_class(cls):
    """The same class as the one-lane emulation runs it (tools/emu/fig_emu_abi.cpp): one wave of one lane, one weight row, always
    the LDS code path with the whole table (mle_form then says whether the emulation takes the lane path, which is what the
    CPU tests of the pruning rest on)."""
    return dict(cls, nt=64, nteams=1, lds_tab=1, tiles=0, tile_cols=0)


def route(r, L):
    """The static part of the routing predicate of fig_hot_mle (:1067, :1203): "lane" for a read of the model's length without N
    (lane-per-read path when it has a hint in its window, else the pair-chain rounds), "chain" for a read with N (plain chain, no
    pruning), "wave" for a shorter read (wave-per-read path with mt_rev offset)."""
    s = r.mate_seq_fastq
    if set(s) - set("ACGT"):
        return "chain"
    return "lane" if len(s) == L else "wave"


def window(model, anchor_pos1, gap_start, G, rlen, gapoffset=0):
    """fig_window_u (fig_engine_hot.h:452-469): the placements lo .. hi of a read against a string of G columns."""
    lo, hi = -(rlen - 1), G - 1
    if anchor_pos1 < gap_start:
        tis0 = gap_start - anchor_pos1 + rlen
        return max(lo, model.Tmin - tis0), min(hi, model.Tmax - tis0)
    tis0 = anchor_pos1 + gapoffset - gap_start + rlen
    return max(lo, tis0 - model.Tmax), min(hi, tis0 - model.Tmin)


# ---- case builders -----------------------------------------------------------------------------------------------------------
def _unit(seed, p):
    """A repeat unit of p bases that has no shorter period and all four bases (from its own generator)."""
    rng = np.random.default_rng(np.random.PCG64(100003 * seed + p))
    while True:
        u = synth._rand_seq(rng, p)
        if len(set(u)) == 4 and not any(u == u[k:] + u[:k] for k in range(1, p)):
            return u


def make_tandem_case(name, seed, gap_specs, periods, **kw):
    """synth.make_case(name, seed, "unmapped", gap_specs, **kw) on a truth in which gap i lies in a tandem repeat of period
    periods[i] (None: left random) from TANDEM_FLANK periods before it to as many after it.  The sequence generator is wrapped
    for this one call: its first draw is the truth, which gets the repeats before the scaffold, the model pairs and the reads
    are made from it.  one_type: the error generator is wrapped as well, so that every substitution -- in the model pairs and in
    the reads alike -- turns a base into the next of ACGT: errorTypeProbs then has a 1 per row and fig_model_fmm = max e."""
    orig, orig_mut, first = synth._rand_seq, synth._mutate, []
    one_type = kw.pop("one_type", False)

    def mutate(rng, s, rate):
        b = bytearray(s.encode())
        hits = [int(h) for h in np.nonzero(rng.random(len(b)) < rate)[0] if chr(b[h]) in "ACGT"]
        for h in hits:
            b[h] = ord("ACGT"[("ACGT".index(chr(b[h])) + 1) % 4])
        return b.decode(), hits

    def rand_seq(rng, n):
        s = orig(rng, n)
        if not first:
            first.append(n)
            assert n == kw["contig_len"]
            for (ts, tl), p in zip(sorted(gap_specs), periods):
                if p:
                    a, b = ts - TANDEM_FLANK * p, ts + tl + TANDEM_FLANK * p
                    assert a >= 0 and b <= n
                    s = s[:a] + (_unit(seed, p) * ((b - a) // p + 1))[:b - a] + s[b:]
        return s

    synth._rand_seq = rand_seq
    if one_type:
        synth._mutate = mutate
    try:
        return synth.make_case(name, seed, "unmapped", gap_specs, **kw)
    finally:
        synth._rand_seq, synth._mutate = orig, orig_mut


def _one(name, seed, g0, L, n, period=None, err=0.005, start=1500, insert=600.0, coverage=30.0, **kw):
    c = make_tandem_case(name, seed, [(start, g0)], [period], contig_len=start + g0 + 1500, read_len=L, insert_mean=insert, insert_sd=30,
                         coverage=coverage, err=err, n_model_pairs=400, partial_reads_in_unmapped=False, **kw)
    return ec.truncate(c, 0, n) if n is not None else c


def shorten(case, gi, cuts):
    """Mates `cuts` = {slot: k} of gap gi lose their last k bases as placed (the file keeps the FASTQ orientation)."""
    for s, k in cuts.items():
        r = case.gaps[gi].unmapped[s]
        r.mate_seq_fastq = r.mate_seq_fastq[:-k] if r.anchor_reverse else r.mate_seq_fastq[k:]
    return case


def case_a(which):
    """a. ties and survivor counts: a tandem gap at L = 36 with 65 reads (period 7, 20, 40, or 50 > L; 0.5 % or 8 % error)."""
    g0, p, err, seed = A_TANDEMS[which]
    return _one(f"a_{which}", seed, g0, 36, 65, period=p, err=err)


def case_b(L):
    """b. read-length masks: a 60-bp gap in a repeat of period 7 (20 from L = 63) at L = 31 .. 65 (Lfull >= 32, rs.len >= 32, mlo / mhi / lml).
    Alone its class would be 180 columns wide, whose weight rows leave no room for the packed consensus (use_kf off: no lane
    path, on the device and in the emulation alike); a gap of B_MATE bp with 6 reads in the same class makes the room."""
    c = make_tandem_case(f"b_L{L}", 5100 + L, [(1500, 60), (3500, B_MATE)], [b_period(L), None], contig_len=3500 + B_MATE + 1500, read_len=L, insert_mean=600.0,
                         insert_sd=30, coverage=40.0, err=0.005, n_model_pairs=400, partial_reads_in_unmapped=False)
    ec.truncate(c, 1, 6)
    return ec.truncate(c, 0, 50 if L < 60 else 36)


def case_b_short():
    """b. reads shorter than the model's L = 36 among full-length ones in the period-20 gap (wave path, mt_rev offset)."""
    return shorten(_one("b_short", 5020, 100, 36, 65, period=20), 0, B_SHORT)


def case_c_slots(which):
    """c. reads with N (estep_cases.N_SLOTS) and three shorter reads (C_SHORT) among 70 reads of the period-20 gap: the wave path's
    accept copy and the lane path's feed the counts and the pile-up of one pass."""
    c = shorten(_one(f"c_{which}", 5020, 100, 36, 70, period=20, coverage=40.0), 0, C_SHORT)
    return ec.write_n(c, 0, ec.N_SLOTS[which])


def case_c_count(kind, n):
    """c. read counts: 63, 64, 65 on the period-20 gap; 1 and nt - 1, nt, nt + 1 on a one-candidate gap of 405 bp (256 threads) or
    500 bp (512 threads), both inside a repeat of period 20 as well.  The last read of each large case carries an N.  (One read
    on a gap of 109 .. 133 bp is outside the oracle's domain: with fewer than 3 reads placed checkGapReads probes 3 G0 columns,
    past the 9 L = 324 the reference allocates for such a gap, and the oracle's tables with it.)"""
    g0 = C_COUNTS[kind][0]
    c = _one(f"c_{kind}_{n}", 5200 + g0, g0, 36, n, period=20, coverage=30.0 if kind == "t" else 45.0)
    return ec.write_n(c, 0, [n - 1]) if n > 1 else c


def case_d(g0):
    """d. short gaps (G0 <= 30) in a repeat of period 7, 40 reads of L = 36 spanning the gap, three of them with an N."""
    return ec.write_n(_one(f"d_{g0}", 5300 + g0, g0, 36, 40, period=7, coverage=70.0), 0, D_N_SLOTS)


def case_e(which):
    """e. error models: an 80-bp gap in a repeat of period 20, L = 36, model pairs and reads at the error rate E_RATES[which];
    for E_BIASED every substitution, in pairs and reads, is of one type per base (fmm_up >= 0.5: no mismatch filter, prefix pruning only)."""
    return _one(f"e_{which}", 5400, 80, 36, 60, period=20, err=E_RATES[which], coverage=40.0, one_type=which in E_BIASED)


def case_e_denorm():
    """e. best products below 1e-290: L = 200, error-free reads under a model from pairs with 97 % substitutions (a match factor
    is 0.03, so a perfect read's product is about 1e-305).  Both make_case calls share seed and truth; only myout.sam is taken
    from the second."""
    kw = dict(g0=60, L=200, n=16, period=20, insert=700.0, coverage=14.0)
    c = _one("e_denorm", 5500, err=0.0, **kw)
    c.myout = _one("e_denorm", 5500, err=0.97, **kw).myout
    c.n_pairs = len(c.myout) // 2
    return c


def case_e_nonmono():
    """e. the non-monotone marker: every model pair gets, at the two read positions NONMONO_AT (mirrored in the reverse mate, so
    that both mates count at the same positions of the model), a one-base deletion in front and a substitution.  errorPosDist and
    delPosDist are both 1 there and 1 - e - ins - del = -1: fig_model_fmm returns 2.0 and the pass evaluates every placement in
    full.  Two positions, so that the product of the factors of a whole read is positive again.  (The oracle still accepts fewer
    than 3 reads in every probe of checkGapReads under this model and never starts its candidate loop: the case pins the MLE passes
    of the probes.  The MD tags written here name only these two substitutions, so the model has e = 0 everywhere else.)"""
    c = _one("e_nonmono", 5600, 80, 36, 60, period=20, coverage=40.0)
    L, out = c.read_len, []
    for ln in c.myout:
        f = ln.split("\t")
        a, b = NONMONO_AT if int(f[1]) == 99 else tuple(L - 1 - x for x in reversed(NONMONO_AT))
        ra, rb = ("ACGT"[("ACGT".index(f[6][x]) + 1) % 4] for x in (a, b))
        f[4] = f"{a}M1D{b - a}M1D{L - b}M"
        f[8] = f"MD:Z:{a}^A0{ra}{b - a - 1}^A0{rb}{L - b - 1}"
        out.append("\t".join(f))
    c.myout = out
    return c


F_SHAPES = {                         # name: (G0, L, insert mean, reads, error rate; 0.85: substitutions of one type, fmm_up >= 0.5)
    "f_lds": (405, 36, 600.0, 20, 0.005),           # 256 threads, 4 weight rows: factor buffers and filter in LDS, the pile-up of 405 columns not
    "f_1250": (1250, 36, 600.0, 20, 0.005),         # the 1217-1600-column class with 4 weight rows: all three in LDS
    "f_1400_L200": (1400, 200, 700.0, 12, 0.005),   # the same class with ONE weight row of 1600 doubles: no factor buffers, no LDS pile-up
    "f_tiled": (2000, 36, 600.0, 20, 0.005),        # LDS-tiled class, MLE pass in its LDS form
    "f_slab": (2600, 36, 600.0, 20, 0.005),         # LDS-tiled class whose MLE table no longer fits: fig_hot_mle<false>
    "f_lds_e85": (405, 36, 600.0, 20, 0.85),        # the first three again without the filter's tables
    "f_1250_e85": (1250, 36, 600.0, 20, 0.85),
    "f_1400_L200_e85": (1400, 200, 700.0, 12, 0.85),
    "f_short_e85": (20, 36, 600.0, 20, 0.85),       # a class of 72 columns (no factor buffers) without the filter's tables
}


def case_f(name):
    """f. memory forms: one gap, one candidate (G0 > 400; f_short_e85: a 20-bp gap, whose class is 72 columns wide), few reads."""
    g0, L, insert, n, err = F_SHAPES[name]
    c = _one(name, 5700 + g0, g0, L, None, period=20 if g0 > 400 else 7, insert=insert, coverage=8.0 if g0 > 400 else 70.0, err=err, one_type=err > 0.5)
    return ec.truncate(c, 0, min(n, len(c.gaps[0].unmapped)))


def candidate_range(G0, partial_len, unm_limit=400):
    """The candidate lengths of an unmapped-mode gap, first and last (gap_alloc / gap_range of fig_gaprules.h, float32 as there)."""
    if G0 <= unm_limit // 3:
        f1, f2 = np.float32(.3), np.float32(3 * partial_len) / np.float32(G0)
    elif G0 <= unm_limit:
        f1, f2 = np.float32(.5), np.float32(2.5)
    else:
        f1 = f2 = np.float32(1.0)
    lo, hi = int(np.float32(G0) * f1), int(np.float32(G0) * f2)
    return lo, max(lo, hi)


def all_cases():
    """{id: builder} of every directed case."""
    out = {}
    for w in A_TANDEMS:
        out[f"a_{w}"] = (lambda w=w: case_a(w))
    for L in B_LENGTHS:
        out[f"b_L{L}"] = (lambda L=L: case_b(L))
    out["b_short"] = case_b_short
    for w in ec.N_SLOTS:
        out[f"c_{w}"] = (lambda w=w: case_c_slots(w))
    for kind, (_, ns) in C_COUNTS.items():
        for n in ns:
            out[f"c_{kind}_{n}"] = (lambda kind=kind, n=n: case_c_count(kind, n))
    for g0 in D_GAPS:
        out[f"d_{g0}"] = (lambda g0=g0: case_d(g0))
    for w in E_RATES:
        out[f"e_{w}"] = (lambda w=w: case_e(w))
    out["e_denorm"] = case_e_denorm
    out["e_nonmono"] = case_e_nonmono
    for name in F_SHAPES:
        out[name] = (lambda name=name: case_f(name))
    return out


TANDEM_IDS = [f"a_{w}" for w in A_TANDEMS] + [f"b_L{L}" for L in B_LENGTHS] + ["b_short"]
POPULATION_IDS = [f"c_{w}" for w in ec.N_SLOTS] + [f"c_{k}_{n}" for k, (_, ns) in C_COUNTS.items() for n in ns]
FORM_IDS = list(F_SHAPES)


def period_of(cid):
    """The repeat period of a case's (only) gap."""
    if cid.startswith("a_"):
        return A_TANDEMS[cid[2:]][1]
    if cid.startswith("b_L"):
        return b_period(int(cid[3:]))
    return 7 if cid.startswith(("d_", "f_short")) else 20


def model_of_case(case, root):
    """The host model of a written case (the same call as tests/test_planes.model_of)."""
    from figbird_amd import api
    return api.model_from_files(os.path.join(root, "scf.fa"), os.path.join(root, "tmp") + "/", os.path.join(root, "tmp", "myout.sam"), partial_flag=0,
                                unmapped_flag=1, script_itr=case.script_itr, max_distance=case.max_distance, read_length=case.read_len,
                                neg_overlap=case.neg_overlap, partial_len=case.partial_len)


if __name__ == "__main__":
    oracle = pc.ORACLE
    only = sys.argv[1:]
    for cid, mk in all_cases().items():
        if only and not any(cid.startswith(o) for o in only):
            continue
        c = mk()
        g = c.gaps[0]
        routes = [route(r, c.read_len) for r in g.unmapped]
        with tempfile.TemporaryDirectory() as d:
            p = synth.write_case(c, d)
            fmm = model_fmm(model_of_case(c, d))
            t0 = time.time()
            r = subprocess.run([oracle, "fillgaps"] + synth.fillgaps_argv(c, p), capture_output=True, text=True)
            secs = time.time() - t0
            assert r.returncode == 0, r.stderr
            filled = open(p["tmp"] + "gapout.txt").read().split("\t")[4]
        classes, cls_of = classes_of(c)
        cl = classes[cls_of[0]]
        f, fe = mle_form(cl, g.length, fmm), mle_form(emu_class(cl), g.length, fmm)
        print(f"{cid}: L={c.read_len} G0={g.length} period={period_of(cid)} reads={len(g.unmapped)} lane/wave/chain={routes.count('lane')}/{routes.count('wave')}/{routes.count('chain')} "
              f"fwd/rev={sum(r.anchor_reverse for r in g.unmapped)}/{sum(not r.anchor_reverse for r in g.unmapped)} filled={filled} oracle={secs:.1f}s fmm={fmm:.4g} "
              f"class(capGl={cl['capGl']} nt={cl['nt']} nteams={cl['nteams']} lds_tab={cl['lds_tab']} tiles={cl['tiles']}) "
              f"form(G={g.length}): " + " ".join(f"{k}={int(v)}" for k, v in f.items()) + f" emulation lane_path={int(fe['lane_path'])}")
