"""Recruiting of the reads the fill rejected (fig_batch_recruit, include/figbird_hip.h: fig_read_recruit).

The restatement below is numpy and independent of fig_recruit_host.h: test_read_placement's scoring over all offsets of a read at
once (one vectorised addition per read base in ascending j), the first maximum by argmax, the exclusion window by a mask, and
test_indel_evidence's band at the seed.  Integers of the device are compared with it for equality and doubles on their int64 view:
the device only adds table entries and compares.
"""
import copy
import ctypes as C
import math
import os
import socket
import subprocess

import numpy as np
import pytest

import util
from figbird_amd import api
import test_read_placement as trp
import test_indel_evidence as tie
import test_polish as tpo
from test_base_support import CODE, INT_MIN, Fill, _gapout, _open_run, _take

NINF = -math.inf
W = 7
OFF, KEPT, NONE, BELOW, AMBIGUOUS, RECRUITED = 0, 1, 2, 3, 4, 5
F_, O_ = api.SUP_FINAL, api.SUP_ORIGINAL
ACGT = tie.ACGT
PAD = tie.PAD
CHARS = {OFF: "~", KEPT: ".", NONE: "~", BELOW: "-", AMBIGUOUS: "=", RECRUITED: "+"}


# ------------------------------------------------------------------------------------- the restatement
def tables(cm):
    """fig_model struct -> (placement tables (lm, le, lt, li, Tmin, Tmax, MI), indel tables (lm, le, lt, lI, lD))"""
    return trp.place_tables(cm), tie.indel_tables(cm)


def score_all(S, n, seq, rev, pos, gap_start, G0, ptabs, check_valid=True):
    """Lr of every valid placement of one read at once -> (o, isz, Lr); S: tie.columns of the gap (element PAD + x is column x)"""
    lm, le, lt, li, Tmin, Tmax, MI = ptabs
    ln = len(seq)
    o = np.arange(-(ln - 1), n, dtype=np.int64)
    isz = trp.isz_of(pos, gap_start, G0, n, ln, o)
    if check_valid:
        ok = (isz >= Tmin) & (isz <= Tmax) & (isz >= 0) & (isz < MI)
        o, isz = o[ok], isz[ok]
        Lr = li[isz].copy()
    else:
        Lr = np.zeros(len(o))
    s = CODE[seq]
    for j in range(ln):
        if s[j] > 3:
            continue
        k = ln - 1 - j if rev else j
        c = S[PAD + o + j]
        with np.errstate(invalid="raise"):
            Lr = Lr + np.where(c > 3, tie.LQ, np.where(c == s[j], lm[k], le[k] + lt[c & 3, s[j]]))
    assert not np.isnan(Lr).any()
    return o, isz, Lr


def restate_gap(S, n, reads, gap_start, G0, tabs, cutoff, margin):
    """reads: [(seq, rev, pos)], the candidates of one gap -> per-read dicts of the header's outputs"""
    ptabs, itabs = tabs
    li = ptabs[3]
    out, seeded = [], []
    for a, (seq, rev, pos) in enumerate(reads):
        r = dict(ll_seed=NINF, ll_second=0.0, ll_flat=0.0, ll_gapped=0.0, score=0.0, off_seed=INT_MIN, off_second=INT_MIN, n_valid=0, d_end=0,
                 read_state=NONE, draw_pos=INT_MIN, draw_isz=0)
        out.append(r)
        if len(seq) == 0:
            continue
        o, isz, Lr = score_all(S, n, seq, rev, pos, gap_start, G0, ptabs)
        r["n_valid"] = int(len(o))
        if not len(o):
            continue
        i = int(np.argmax(Lr))                                  # the first of equal maxima = the smallest offset
        if Lr[i] == NINF:
            continue
        r["ll_seed"], r["off_seed"], r["isz"] = float(Lr[i]), int(o[i]), int(isz[i])
        far = np.abs(o - o[i]) > W
        if far.any():
            i2 = int(np.argmax(Lr[far]))
            r["ll_second"], r["off_second"] = float(Lr[far][i2]), int(o[far][i2])
        else:
            r["ll_second"] = NINF
        seeded.append(a)
    if seeded:
        H, _, flat = tie.band(S, [(reads[a][0], reads[a][1], out[a]["off_seed"]) for a in seeded], itabs)
        for b, a in enumerate(seeded):
            r = out[a]
            best, d_end = NINF, 0
            for dd in tie.END_ORDER:
                if H[b, dd + W] > best:
                    best, d_end = float(H[b, dd + W]), dd
            r["ll_flat"], r["ll_gapped"], r["d_end"] = float(flat[b]), best, d_end
            r["score"] = float(li[r["isz"]] + np.float64(best))
            if not -r["score"] < float(cutoff):
                r["read_state"] = BELOW
            elif not (r["ll_second"] == NINF or r["ll_seed"] - r["ll_second"] > margin):
                r["read_state"] = AMBIGUOUS
            else:
                r["read_state"] = RECRUITED
                r["draw_pos"], r["draw_isz"] = r["off_seed"], r["isz"]
    return out


FIELDS_D = ("ll_seed", "ll_second", "ll_flat", "ll_gapped", "score")
FIELDS_I = ("off_seed", "off_second", "n_valid", "d_end", "read_state", "draw_pos", "draw_isz", "n_candidates", "n_recruited", "state")


def expected(H, margin=0.0, tabs=None, state=None, cutoff=None, gaps=None):
    """The restatement of a whole case (an RCase, a trp.HandPlace or a golden view) -> dict of the arrays of fig_read_recruit.  gaps: the
    gaps to restate (default all); the others keep the defaults and are not to be compared."""
    tabs = tabs or tables(H.model.cstruct())
    cutoff = H.model.cutoff if cutoff is None else cutoff
    state = H.state if state is None else state
    NU, ng = H.NU, len(H.filled_len)
    w = dict(ll_seed=np.zeros(NU), ll_second=np.zeros(NU), ll_flat=np.zeros(NU), ll_gapped=np.zeros(NU), score=np.zeros(NU), off_seed=np.full(NU, INT_MIN, np.int32),
             off_second=np.full(NU, INT_MIN, np.int32), n_valid=np.zeros(NU, np.int32), d_end=np.zeros(NU, np.int32), read_state=np.zeros(NU, np.uint8),
             draw_pos=np.array(H.draw_pos[:NU], dtype=np.int32), draw_isz=np.array(H.draw_isz[:NU], dtype=np.int32), n_candidates=np.zeros(ng, np.int32),
             n_recruited=np.zeros(ng, np.int32), state=np.asarray(state, dtype=np.uint8))
    for g in (range(ng) if gaps is None else gaps):
        if not state[g]:
            continue
        k0, k1 = int(H.u_off[g]), int(H.u_off[g + 1])
        n = int(H.filled_len[g]); a = int(H.str_off[g])
        contig, start, G0 = H.geometry(g) if hasattr(H, "geometry") else (H.contig, int(H.starts[g]), trp.G0)
        S = tie.columns(contig, start, G0, H.raw[a:a + n])
        cand = [k for k in range(k0, k1) if H.draw_pos[k] == INT_MIN]
        for k in range(k0, k1):
            w["read_state"][k] = KEPT
        rs = restate_gap(S, n, [(H.seqs[k], int(H.rev[k]), int(H.pos[k])) for k in cand], start, G0, tabs, cutoff, margin)
        for k, r in zip(cand, rs):
            for f in FIELDS_D + FIELDS_I[:7]:
                w[f][k] = r[f]
        w["n_candidates"][g] = len(cand)
        w["n_recruited"][g] = sum(1 for r in rs if r["read_state"] == RECRUITED)
    return w


def compare(R, want, reads=None):
    """every array of the device against the restatement's: doubles on their int64 view, everything else equal.  reads: a mask of the
    reads to compare (default all; then the per-gap arrays are compared as well)"""
    sel = slice(None) if reads is None else reads
    for f in FIELDS_D:
        got, wt = np.asarray(getattr(R, f))[sel], np.asarray(want[f])[sel]
        bad = np.flatnonzero(got.view(np.int64) != wt.view(np.int64))
        assert not len(bad), f"{f}: reads {bad[:8]}: got {got[bad[:4]]}, want {wt[bad[:4]]}"
    for f in FIELDS_I:
        if reads is not None and f in ("n_candidates", "n_recruited", "state"):
            continue
        got, wt = np.asarray(getattr(R, f)), np.asarray(want[f])
        assert got.shape == wt.shape and got.dtype == wt.dtype, f
        if f not in ("n_candidates", "n_recruited", "state"):
            got, wt = got[sel], wt[sel]
        bad = np.flatnonzero(got != wt)
        assert not len(bad), f"{f}: elements {bad[:8]}: got {got[bad[:4]]}, want {wt[bad[:4]]}"


# ------------------------------------------------------------------------------------- hand-made cases
class RCase(tie.Case):
    """tie.Case whose reads may carry a fourth element, the anchor relative to the gap's start (default -300: a left anchor); the drawn
    reads get an insert size of their own in the caller's plane, so that a carried value shows"""

    def __init__(self, gaps, model, seed=1):
        super().__init__([dict(gp, reads=[r[:3] for r in gp["reads"]]) for gp in gaps], model, seed)
        self.pos = [int(self.starts[g]) + (int(r[3]) if len(r) > 3 else -300) for g, gp in enumerate(gaps) for r in gp["reads"]]
        self.batch.u_anchor_pos = np.asarray(self.pos if self.pos else [0], dtype=np.int32)
        self.draw_isz = np.where(self.draw_pos != INT_MIN, 1000 + np.arange(len(self.draw_pos)), 0).astype(np.int32)

    def merged(self, draw_pos, draw_isz):
        """a view of this case whose draw planes are the given ones (the restatements of the indel pass and the polish read them)"""
        M = copy.copy(self)
        M.draw_pos = np.array(draw_pos, dtype=np.int32); M.draw_isz = np.array(draw_isz, dtype=np.int32)
        return M


# The withheld case's cutoff.  Over the withheld spanning reads of both gaps the restatement gives: the greatest -score 13.375 (a read
# with two substitutions beside its indel) and the smallest best ungapped -Lr 14.318 (a read that starts eight columns before the
# extra base and is drawn shifted, so that only those eight columns mismatch).  An integer cutoff c holds every asserted condition
# iff 13.375 < c <= 14.318: 14 is the one value.
CUTOFF = 14
SPAN_MARGIN = 8
SITES = {1: tie.HOMO_AT, 2: tie.UNIQUE_AT}


def withheld_case():
    """tie.planted_case()'s three gaps and reads.  In gap 1 (the homopolymer one base short, site 45) and gap 2 (a base too many, site
    52) only the reads that do not reach within 8 columns of the site stay drawn -- FAR: they end before site - 8 or start after
    site + 8 -- plus the first SPANNING read, one that covers at least 8 columns either side of the site.  Every other read is passed
    undrawn: the other SPANNING reads, of which the test asserts that the fill would have rejected them, and the EDGE reads that end or
    start within 8 columns of the site (they overlap the error by too few columns to lose the cutoff ungapped: their best ungapped
    -Lr goes down to 3.2, a read without a mismatch, so no cutoff rejects them, and the conditions on rejection are stated for the
    SPANNING reads).  Gap 0, the unedited string, keeps all its reads drawn: a gap that is on with no candidate.
    -> (RCase, kinds per read: 'far' | 'span' | 'edge', the truth)"""
    P = tie.planted_case()
    model = tie.clean_model()
    model.cutoff = CUTOFF
    gaps, kinds = [], []
    for g in range(3):
        st = int(P.starts[g]); a = int(P.str_off[g]); n = int(P.filled_len[g])
        reads, kept_one = [], False
        for k in range(int(P.u_off[g]), int(P.u_off[g + 1])):
            o, ln = int(P.draw_pos[k]), len(P.seqs[k])
            if g == 0:
                kind, keep = "far", True
            else:
                site = SITES[g]
                far = o + ln - 1 < site - SPAN_MARGIN or o > site + SPAN_MARGIN
                span = o <= site - SPAN_MARGIN and o + ln - 1 >= site + SPAN_MARGIN
                kind = "far" if far else "span" if span else "edge"
                keep = far or (span and not kept_one)
                kept_one = kept_one or span
            kinds.append(kind)
            reads.append((P.seqs[k], int(P.rev[k]), o if keep else INT_MIN))
        gaps.append(dict(string=np.array(P.raw[a:a + n]), reads=reads, left=np.array(P.contig[max(st - 300, 0):st]), right=np.array(P.contig[st + trp.G0:st + trp.G0 + 300])))
    H = RCase(gaps, model)
    assert H.contig.tobytes() == P.contig.tobytes()
    return H, kinds, np.array(P.raw[:101])


@pytest.fixture(scope="module")
def withheld():
    H, kinds, truth = withheld_case()
    return H, expected(H), kinds, truth


def edge_model(**kw):
    """clean_model() with a stretch of the insert-size table set to 0 (li = -inf over 700 .. 759) and a cutoff that lets a long read
    with a few substitutions through"""
    m = tie.clean_model(**kw)
    m.insd = m.insd.copy()
    m.insd[700:760] = 0.0
    m.cutoff = 40
    return m


EDGE_LENS = (1, 16, 17, 31, 199, 200)
UNIT = trp.UNIT
EDGE_NAMES = ("c1", "c63", "c64", "c65", "nochunk", "n1", "n57", "n58", "n313", "n314", "ends", "tiles", "p3", "p12", "p12sub", "invalid", "li0", "none", "ncols")


def _copy_read(rng, S, ln, t, sub=0.02, indel=False):
    """a read of ln bases copied from the columns t .. of a gap, N columns filled at random, `sub` substitutions, with `indel` one base
    removed or added in its middle"""
    src = np.frombuffer(b"ACGTN", dtype=np.uint8)[S[PAD + t + np.arange(ln + 2)]].copy()
    src[src == ord("N")] = rng.choice(ACGT, size=int((src == ord("N")).sum()))
    if indel and ln > 20:
        cut = int(rng.integers(8, ln - 8))
        src = np.delete(src, cut) if rng.integers(0, 2) else np.insert(src, cut, rng.choice(ACGT))
    return tie.mutate(rng, src[:ln], sub)


def edge_case():
    """One gap per edge (EDGE_NAMES): 1, 63, 64 and 65 candidates among a few drawn reads; 70 reads whose first chunk holds no
    candidate; n = 1, 57, 58, 313 and 314 (offsets start at -199: one tile, two, two and three); reads copied from the columns at
    o = -(len-1) and at o = n-1; reads copied from o = 56 and o = 57, the last lane of the first tile and the first of the next; a
    tandem repeat of period 3 whose equal placements lie inside the window; one of period 12 whose equal placements lie outside it; the
    same with one substitution in the string; reads whose best ungapped offset is invalid by Tmin and by Tmax; a read whose true
    offset has the insert size whose table entry is 0; a read with no valid placement and one whose every valid placement is -inf; N
    bases first and last and N columns under the seed.  The lengths 1, 16, 17, 31, 199 and 200 are dealt in turn."""
    rng = np.random.default_rng(20261201)
    uniq = tpo.unique_truth
    pre = []
    for name, n in (("c1", 40), ("c63", 60), ("c64", 60), ("c65", 60), ("nochunk", 50), ("n1", 1), ("n57", 57), ("n58", 58), ("n313", 313), ("n314", 314), ("ends", 90), ("tiles", 120)):
        pre.append(dict(name=name, string=rng.choice(ACGT, size=n).copy(), reads=[], left=uniq(rng, 300), right=uniq(rng, 300)))
    rep3 = np.frombuffer(b"ACG" * 9, dtype=np.uint8)
    pre.append(dict(name="p3", string=np.concatenate([uniq(rng, 20), rep3, uniq(rng, 20)]), reads=[(np.frombuffer(b"ACG" * 7, dtype=np.uint8).copy(), 0, INT_MIN)] * 2,
                    left=uniq(rng, 300), right=uniq(rng, 300)))
    u12 = np.tile(UNIT, 6)
    rd12 = np.tile(UNIT, 3)
    pre.append(dict(name="p12", string=np.concatenate([uniq(rng, 20), u12, uniq(rng, 20)]), reads=[(rd12.copy(), 0, INT_MIN), (rd12.copy(), 1, INT_MIN)], left=uniq(rng, 300), right=uniq(rng, 300)))
    sub12 = u12.copy(); sub12[3 * 12 + 5] = ord("A") if sub12[3 * 12 + 5] != ord("A") else ord("C")
    pre.append(dict(name="p12sub", string=np.concatenate([uniq(rng, 20), sub12, uniq(rng, 20)]), reads=[(rd12.copy(), 0, INT_MIN)], left=uniq(rng, 300), right=uniq(rng, 300)))
    for name, n in (("invalid", 80), ("li0", 80), ("none", 12), ("ncols", 80)):
        s = rng.choice(ACGT, size=n).copy()
        if name == "ncols":
            s[[30, 31, 44]] = ord("N")
        pre.append(dict(name=name, string=s, reads=[], left=uniq(rng, 300), right=uniq(rng, 300)))
    shell = RCase(pre, edge_model())                             # the contig the reads are copied from
    col = {gp["name"]: tie.columns(shell.contig, int(shell.starts[g]), trp.G0, gp["string"]) for g, gp in enumerate(pre)}
    by = {gp["name"]: gp for gp in pre}
    turn = [0]

    def ln_next():
        turn[0] += 1
        return EDGE_LENS[turn[0] % len(EDGE_LENS)]

    def some(name, count, drawn_every=0, indel_every=3):
        n = len(by[name]["string"])
        for r in range(count):
            ln = ln_next()
            t = int(rng.integers(-(ln - 1), n))
            s = _copy_read(rng, col[name], ln, t, indel=(r % indel_every == 1))
            if r % 5 == 3:
                s[0] = ord("N")
            if r % 7 == 5:
                s[-1] = ord("N")
            by[name]["reads"].append((s, r % 2, t if (drawn_every and r % drawn_every == 0) else INT_MIN, -300 if r % 4 else n - trp.G0 + 300))
    some("c1", 5, drawn_every=1); by["c1"]["reads"][2] = by["c1"]["reads"][2][:2] + (INT_MIN,) + by["c1"]["reads"][2][3:]
    for name, cnt in (("c63", 63), ("c64", 64), ("c65", 65)):
        some(name, cnt)
        for r in range(3):                                       # three drawn reads behind the candidates
            ln = ln_next(); t = int(rng.integers(0, 20))
            by[name]["reads"].append((_copy_read(rng, col[name], ln, t), r % 2, t))
    some("nochunk", 64, drawn_every=1); some("nochunk", 6)
    for name in ("n1", "n57", "n58", "n313", "n314"):
        some(name, 12)
    n = 90
    for ln in EDGE_LENS[1:]:                                     # exact copies at either end of the placement range
        by["ends"]["reads"].append((_copy_read(rng, col["ends"], ln, -(ln - 1), sub=0.0), 0, INT_MIN))
        by["ends"]["reads"].append((_copy_read(rng, col["ends"], ln, n - 1, sub=0.0), 1, INT_MIN))
    for ln in (31, 200):
        for t in (56, 57):
            by["tiles"]["reads"].append((_copy_read(rng, col["tiles"], ln, t, sub=0.0), 0, INT_MIN))
    # the true offset 20 of a 31-base read has insert size 149 (below Tmin = 150) under the anchor 31 + 20 - 149 = -98, and 1001 (above
    # Tmax = 1000) under 31 + 20 - 1001 = -950: the best placement over all offsets is not valid
    by["invalid"]["reads"] += [(_copy_read(rng, col["invalid"], 31, 20, sub=0.0), 0, INT_MIN, -98), (_copy_read(rng, col["invalid"], 31, 20, sub=0.0), 0, INT_MIN, -950)]
    # insert size 500 at the true offset under the anchor 31 + 20 - 500 = -449: the model's table is 0 there
    by["li0"]["reads"].append((_copy_read(rng, col["li0"], 31, 20, sub=0.0), 0, INT_MIN, -449))
    # n = 12, 31 bases: offsets -30 .. 11; anchor -715 gives the insert sizes 716 .. 757, all inside the zeroed stretch: every valid
    # placement is -inf; anchor -5000 gives no valid placement at all
    by["none"]["reads"] += [(_copy_read(rng, col["none"], 31, -5, sub=0.0), 0, INT_MIN, -715), (_copy_read(rng, col["none"], 31, -5, sub=0.0), 1, INT_MIN, -5000)]
    for ln, t in ((31, 20), (17, 28), (200, -100)):               # seeds over the N columns 30, 31 and 44
        s = _copy_read(rng, col["ncols"], ln, t, sub=0.0); s[0] = ord("N"); s[-1] = ord("N")
        by["ncols"]["reads"].append((s, 0, INT_MIN))
    return RCase(pre, edge_model())


@pytest.fixture(scope="module")
def edges():
    H = edge_case()
    return H, expected(H)


def flat_case():
    """ins = del = 0: lI and lD are -inf, the band has one finite diagonal per start and ll_gapped == ll_flat"""
    rng = np.random.default_rng(20261202)
    s = rng.choice(ACGT, size=70).copy()
    shell = RCase([dict(string=s, reads=[])], edge_model(ins=0.0, dele=0.0))
    S = tie.columns(shell.contig, int(shell.starts[0]), trp.G0, s)
    reads = [(_copy_read(rng, S, ln, int(rng.integers(-(ln - 1), 70)), indel=(r % 2 == 1)), r % 2, INT_MIN) for r, ln in enumerate((31, 60, 77, 16, 200, 64))]
    return RCase([dict(string=s, reads=reads)], edge_model(ins=0.0, dele=0.0))


def maxinsert_case():
    """Tmax = max_insert = 1200, the greatest the library takes: the true offset 20 of a 31-base read has insert size 1200 under the anchor
    31 + 20 - 1200, which passes Tmax and lies outside the table"""
    rng = np.random.default_rng(20261203)
    m = edge_model(); m.Tmax = 1200
    s = rng.choice(ACGT, size=80).copy()
    shell = RCase([dict(string=s, reads=[])], m)
    S = tie.columns(shell.contig, int(shell.starts[0]), trp.G0, s)
    m2 = edge_model(); m2.Tmax = 1200
    return RCase([dict(string=s, reads=[(_copy_read(rng, S, 31, 20, sub=0.0), 0, INT_MIN, -1149)])], m2)


def _gap_index(name):
    return EDGE_NAMES.index(name)


def _reads_of(H, g):
    return range(int(H.u_off[g]), int(H.u_off[g + 1]))


# ------------------------------------------------------------------------------------- CPU
def test_rules_by_hand():
    """fig_recruit_host.h through the host library: the three-way rule with a -inf second; the margin at equality (not recruited); the
    cutoff at equality (not recruited); the exclusion window at |d| = 7 and |d| = 8; the order of the seed; seeded; the caller's margin;
    the merge; the writer's characters"""
    h = api.load_host_library()
    rule = h.fighost_recruit_rule
    assert rule(-10.0, 15, -9.0, NINF, 0.0) == RECRUITED and rule(-10.0, 15, -9.0, NINF, 1e300) == RECRUITED
    assert rule(-15.0, 15, -9.0, NINF, 0.0) == BELOW and rule(math.nextafter(-15.0, 0.0), 15, -9.0, NINF, 0.0) == RECRUITED and rule(-15.5, 15, -9.0, -900.0, 0.0) == BELOW
    assert rule(NINF, 15, -9.0, NINF, 0.0) == BELOW and rule(-20.0, 15, -9.0, -9.0, 0.0) == BELOW                # the cutoff comes first
    assert rule(-10.0, 15, -9.0, -9.0, 0.0) == AMBIGUOUS and rule(-10.0, 15, -9.0, -9.5, 0.5) == AMBIGUOUS and rule(-10.0, 15, -9.0, -9.5, 0.25) == RECRUITED
    assert rule(-10.0, 15, -9.0, math.nextafter(-9.0, NINF), 0.0) == RECRUITED and rule(-10.0, 15, -9.5, -9.0, 0.0) == AMBIGUOUS
    assert rule(-10.0, -3, -9.0, NINF, 0.0) == BELOW and rule(2.0, -1, 3.0, NINF, 0.0) == RECRUITED                 # a negative cutoff is the model's business
    out = h.fighost_recruit_outside
    assert [out(10 + d, 10) for d in (-8, -7, 0, 7, 8)] == [1, 0, 0, 0, 1] and out(INT_MIN + 8, 2 ** 31 - 1) == 1
    bef = h.fighost_recruit_before
    assert bef(-1.0, 5, -2.0, 0) == 1 and bef(-2.0, 0, -1.0, 5) == 0 and bef(-1.0, 4, -1.0, 5) == 1 and bef(-1.0, 5, -1.0, 5) == 0 and bef(NINF, 3, NINF, 2 ** 31 - 1) == 1
    assert h.fighost_recruit_seeded(0, -1.0) == 0 and h.fighost_recruit_seeded(3, NINF) == 0 and h.fighost_recruit_seeded(1, -1e300) == 1
    assert h.fighost_recruit_candidate(INT_MIN) == 1 and h.fighost_recruit_candidate(0) == 0 and h.fighost_recruit_candidate(-5) == 0
    assert h.fighost_recruit_score(-3.0, -4.5) == -7.5 and h.fighost_recruit_score(-3.0, NINF) == NINF
    ok = h.fighost_recruit_margin_ok
    assert [ok(v) for v in (0.0, 1.5, 1e308, -0.0, -1e-300, math.inf, -math.inf, math.nan)] == [1, 1, 1, 1, 0, 0, 0, 0]
    pair = np.zeros(2, dtype=np.int32)
    for st, want in ((OFF, (7, 9)), (KEPT, (7, 9)), (RECRUITED, (-3, 411)), (NONE, (INT_MIN, 0)), (BELOW, (INT_MIN, 0)), (AMBIGUOUS, (INT_MIN, 0))):
        h.fighost_recruit_merge(st, 7, 9, -3, 411, api._p(pair, api.c_i32_p))
        assert tuple(pair) == want, st
    assert "".join(chr(h.fighost_recruit_char(s)) for s in range(6)) == "".join(CHARS[s] for s in range(6)) == "~.~-=+"
    st = np.zeros(4, dtype=np.uint8)
    fl = np.array([5, 5, 0, 5], dtype=np.int32); dl = np.array([5, -1, 5, -1, 0, -1, -1, 5], dtype=np.int32); org = np.array([F_, F_ | O_, F_, F_], dtype=np.int32)
    h.fighost_recruit_gaps_on(1, 4, api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p), api._p(st, api.c_u8_p))
    assert list(st) == [1, 0, 0, 0]
    h.fighost_recruit_gaps_on(0, 4, api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p), api._p(st, api.c_u8_p))
    assert list(st) == [0, 0, 0, 0]


def test_abi_surface(tmp_path):
    """the header declares the call and the struct, the version stays 1, the Python struct has the header's fifteen pointers in its
    order and its size, the constants agree, and the call is in EXPORTS"""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert "#define FIG_ABI_VERSION 1" in hdr
    assert "int fig_batch_recruit(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, double min_margin, fig_read_recruit *out);" in hdr
    body = hdr[hdr.index("typedef struct fig_read_recruit {"):hdr.index("} fig_read_recruit;")]
    names = [ln.split(";")[0].split("*")[-1].strip() for ln in body.splitlines()[1:] if "*" in ln.split("/*")[0]]
    assert names == [f for f, _ in api.FigReadRecruit._fields_] and len(names) == 15
    assert "fig_batch_recruit" in api.EXPORTS and "recruit" in api.FillResult.__dataclass_fields__
    consts = ("FIG_RECRUIT_OFF", "FIG_RECRUIT_ON", "FIG_RECRUIT_READ_OFF", "FIG_RECRUIT_KEPT", "FIG_RECRUIT_NONE", "FIG_RECRUIT_BELOW", "FIG_RECRUIT_AMBIGUOUS", "FIG_RECRUIT_RECRUITED")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu", sizeof(fig_read_recruit), sizeof(fig_gap_results));'
           + "".join(f'printf(" %d", {c});' for c in consts) + "".join(f'printf(" %zu", offsetof(fig_read_recruit, {f}));' for f in names) + 'printf("\\n");return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert out == [C.sizeof(api.FigReadRecruit), C.sizeof(api.FigGapResults), api.RECRUIT_OFF, api.RECRUIT_ON, api.RECRUIT_READ_OFF, api.RECRUIT_KEPT, api.RECRUIT_NONE,
                   api.RECRUIT_BELOW, api.RECRUIT_AMBIGUOUS, api.RECRUIT_RECRUITED] + [getattr(api.FigReadRecruit, f).offset for f in names]
    assert (OFF, KEPT, NONE, BELOW, AMBIGUOUS, RECRUITED) == (api.RECRUIT_READ_OFF, api.RECRUIT_KEPT, api.RECRUIT_NONE, api.RECRUIT_BELOW, api.RECRUIT_AMBIGUOUS, api.RECRUIT_RECRUITED)
    assert C.sizeof(api.FigGapResults) == 128


def test_withheld_case_is_not_vacuous(withheld):
    """The restatement alone.  Every withheld spanning read's best ungapped -Lr is at least the cutoff -- the fill would have rejected it
    -- and every undrawn read's -score is below it: all of them are RECRUITED.  CUTOFF lies between the two extremes the comment beside
    it names.  On the fill's plane (the far reads and one spanning read) the indel restatement makes no call and the polish restatement
    no edit; on the merged plane it calls exactly 'I' at 45 in gap 1 and 'D' at 52 in gap 2, and the polish ends every gap equal to the
    truth."""
    H, Wt, kinds, truth = withheld
    und = np.array([H.draw_pos[k] == INT_MIN for k in range(H.NU)])
    span = np.array([k == "span" for k in kinds]) & und
    edge = np.array([k == "edge" for k in kinds])
    assert list(H.state) == [1, 1, 1] and not und[:40].any() and list(Wt["n_candidates"]) == [0, int(und[40:80].sum()), int(und[80:].sum())]
    assert span[40:80].sum() >= 10 and span[80:].sum() >= 10 and (edge == (und & ~span)).all() and edge[40:80].sum() >= 5
    for g in (1, 2):
        ks = list(_reads_of(H, g))
        assert sum(1 for k in ks if kinds[k] == "span" and not und[k]) == 1 and all(not und[k] for k in ks if kinds[k] == "far")
    lo, hi = float((-Wt["score"][span]).max()), float((-Wt["ll_seed"][span]).min())
    print(f"withheld spanning reads {int(span.sum())}: greatest -score {lo:.4f}, smallest best ungapped -Lr {hi:.4f}; edge reads {int(edge.sum())}: "
          f"smallest -Lr {float((-Wt['ll_seed'][edge]).min()):.4f}, greatest -score {float((-Wt['score'][edge]).max()):.4f}")
    assert abs(lo - 13.375) < 1e-3 and abs(hi - 14.318) < 1e-3 and lo < CUTOFF <= hi
    assert (-Wt["ll_seed"][span] >= CUTOFF).all() and (-Wt["score"][und] < CUTOFF).all()
    assert (Wt["read_state"][und] == RECRUITED).all() and (Wt["read_state"][~und] == KEPT).all() and list(Wt["n_recruited"]) == list(Wt["n_candidates"])
    assert (Wt["ll_gapped"][span] > Wt["ll_flat"][span]).all() and (-Wt["ll_seed"][edge]).min() < 4.0
    assert (Wt["draw_pos"][und] == Wt["off_seed"][und]).all() and (Wt["draw_pos"][~und] == H.draw_pos[:H.NU][~und]).all() and (Wt["draw_isz"][~und] == H.draw_isz[:H.NU][~und]).all()
    assert (Wt["draw_isz"][und] == 300 + np.array([len(s) for s in H.seqs])[und] + Wt["off_seed"][und]).all()
    own = tie.expected(H)
    assert own["call"].tobytes() == b"." * len(own["call"]) and own["call_end"].tobytes() == b"..."
    M = H.merged(Wt["draw_pos"], Wt["draw_isz"])
    mer = tie.expected(M)
    calls = {int(i): chr(c) for i, c in enumerate(mer["call"]) if c != ord(".")}
    assert calls == {int(H.str_off[1]) + tie.HOMO_AT: "I", int(H.str_off[2]) + tie.UNIQUE_AT: "D"} and mer["call_end"].tobytes() == b"..."
    pol_own, pol_mer = tpo.expected(H), tpo.expected(M)
    assert not pol_own["edit"].any() and list(pol_own["state"]) == [tpo.ON] * 3
    assert [s.tobytes() for s in pol_mer["strings"]] == [truth.tobytes()] * 3 and list(pol_mer["state"]) == [tpo.ON, tpo.ON | tpo.EDITED, tpo.ON | tpo.EDITED]


def test_edge_case_is_not_vacuous(edges):
    """The restatement alone, on the edge case: what each gap was built for happens"""
    H, Wt = edges
    g = {name: i for i, name in enumerate(EDGE_NAMES)}
    ks = lambda name: list(_reads_of(H, g[name]))
    assert [int(Wt["n_candidates"][g[nm]]) for nm in ("c1", "c63", "c64", "c65", "nochunk")] == [1, 63, 64, 65, 6]
    assert all(H.draw_pos[k] != INT_MIN for k in ks("nochunk")[:64]) and len(ks("nochunk")) == 70
    assert [int(H.filled_len[g[nm]]) for nm in ("n1", "n57", "n58", "n313", "n314")] == [1, 57, 58, 313, 314]
    for nm in ("c65", "n57", "n313"):
        assert {len(H.seqs[k]) for k in ks(nm)} == set(EDGE_LENS), nm
    assert set(int(s) for s in Wt["read_state"]) == {KEPT, NONE, BELOW, AMBIGUOUS, RECRUITED}
    # either end of the placement range, and the two sides of a tile boundary
    lens = np.array([len(s) for s in H.seqs])
    e = np.array(ks("ends"))
    assert (Wt["off_seed"][e[0::2]] == -(lens[e[0::2]] - 1)).all() and (Wt["off_seed"][e[1::2]] == 89).all()
    assert list(Wt["off_seed"][ks("tiles")]) == [56, 57, 56, 57] and list(Wt["read_state"][ks("tiles")]) == [RECRUITED] * 4
    # period 3: the equal placements 20, 23, 26 lie inside the window of the seed 20, so the second is far below
    tabs = tables(H.model.cstruct())
    for nm, want_seed in (("p3", 20), ("p12", 20), ("p12sub", 20)):
        k = ks(nm)[0]; gi = g[nm]
        S = tie.columns(H.contig, int(H.starts[gi]), trp.G0, H.raw[int(H.str_off[gi]):int(H.str_off[gi + 1])])
        o, _, Lr = score_all(S, int(H.filled_len[gi]), H.seqs[k], int(H.rev[k]), H.pos[k], int(H.starts[gi]), trp.G0, tabs[0])
        at = {int(a): float(b) for a, b in zip(o, Lr)}
        assert Wt["off_seed"][k] == want_seed
        if nm == "p3":
            assert at[20] == at[23] == at[26] and Wt["ll_second"][k] < Wt["ll_seed"][k] - 2 and Wt["read_state"][k] == RECRUITED
        elif nm == "p12":
            assert at[20] == at[32] == at[44] and Wt["ll_second"][k] == Wt["ll_seed"][k] and Wt["off_second"][k] == 32 and Wt["read_state"][k] == AMBIGUOUS
        else:
            assert at[20] > at[32] and Wt["off_second"][k] == 32 and 2.0 < Wt["ll_seed"][k] - Wt["ll_second"][k] < 3.5 and Wt["read_state"][k] == RECRUITED
    # the best offset over all placements is not valid: the seed is the best valid one
    gi = g["invalid"]
    S = tie.columns(H.contig, int(H.starts[gi]), trp.G0, H.raw[int(H.str_off[gi]):int(H.str_off[gi + 1])])
    for k, side in zip(ks("invalid"), (1, -1)):
        o, _, Lr = score_all(S, 80, H.seqs[k], 0, H.pos[k], int(H.starts[gi]), trp.G0, tabs[0], check_valid=False)
        assert int(o[int(np.argmax(Lr))]) == 20 and Wt["off_seed"][k] != 20 and (Wt["off_seed"][k] - 20) * side > 0 and Wt["n_valid"][k] < 80 + 30
    k = ks("li0")[0]
    assert tabs[0][3][500] == NINF and Wt["off_seed"][k] != 20 and Wt["ll_seed"][k] > NINF
    k0, k1 = ks("none")
    assert (Wt["n_valid"][k0], Wt["n_valid"][k1]) == (42, 0) and Wt["ll_seed"][k0] == NINF and Wt["ll_seed"][k1] == NINF and list(Wt["read_state"][[k0, k1]]) == [NONE, NONE]
    assert list(Wt["off_seed"][[k0, k1]]) == [INT_MIN, INT_MIN] and list(Wt["score"][[k0, k1]]) == [0.0, 0.0]
    kn = ks("ncols")
    assert list(Wt["off_seed"][kn]) == [20, 28, -100] and all(H.seqs[k][0] == ord("N") and H.seqs[k][-1] == ord("N") for k in kn)
    Fc = flat_case(); Wf = expected(Fc)
    seeded = Wf["read_state"] != NONE
    assert seeded.sum() == 6 and Wf["ll_gapped"].view(np.int64).tolist() == Wf["ll_flat"].view(np.int64).tolist() and not Wf["d_end"].any()
    Mc = maxinsert_case(); Wm = expected(Mc)
    assert Wm["off_seed"][0] < 20 and Wm["n_valid"][0] == 50                # the offsets -30 .. 19: 1150 .. 1199


def _flanks(S, n):
    return "".join(str(int(S[PAD - 1 - i])) for i in range(208)) + "".join(str(int(S[PAD + n + i])) for i in range(208))


def _program_case(H, tabs):
    """the case file of tests/recruit_read_main.cpp: every candidate of every gap of H that is on -> (lines, [read index])"""
    (lm, le, lt, li, Tmin, Tmax, MI), (_, _, _, lI, lD) = tabs
    hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v).reshape(-1))
    lines = [str(len(lm)), hx(lm), hx(le), hx(lt), hx(lI), hx(lD), str(MI), hx(li), f"{Tmin} {Tmax}"]
    on = [g for g in range(len(H.filled_len)) if H.state[g]]
    lines.append(str(len(on)))
    index = []
    for g in on:
        n = int(H.filled_len[g]); a = int(H.str_off[g])
        S = tie.columns(H.contig, int(H.starts[g]), trp.G0, H.raw[a:a + n])
        ks = [k for k in _reads_of(H, g) if H.draw_pos[k] == INT_MIN and len(H.seqs[k])]
        lines += [f"{n} {int(H.starts[g])} {trp.G0} {len(ks)}", _flanks(S, n), H.raw[a:a + n].tobytes().decode()]
        for k in ks:
            lines += [f"{int(H.pos[k])} {len(H.seqs[k])} {int(H.rev[k])}", H.seqs[k].tobytes().decode()]
        index += ks
    return lines, index


def test_kernel_pieces_on_the_cpu(withheld, edges, tmp_path):
    """The __host__ __device__ pieces of fig_recruit.h, fig_recruit_host.h, fig_placement.h and fig_band.h (the band in
    tests/band_form.h's form) compiled as plain C++ into a program of its own with AddressSanitizer and UBSan (tests/recruit_read_main.cpp; run directly), over the withheld, the edge, the
    ins = del = 0 and the max_insert case: inside the program the kernel's form -- tiles, per-wave slots, two passes, the 16-lane band
    -- equals a sequential restatement in every output bit for bit; its output equals the numpy restatement."""
    exe = str(tmp_path / "recruit_read_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "recruit_read_main.cpp")])
    total = 0
    Fc = flat_case(); Mc = maxinsert_case()
    for tag, H, Wt in (("withheld", withheld[0], withheld[1]), ("edges", edges[0], edges[1]), ("flat", Fc, expected(Fc)), ("maxinsert", Mc, expected(Mc))):
        lines, index = _program_case(H, tables(H.model.cstruct()))
        case = tmp_path / f"{tag}.txt"
        case.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(case)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("R ")]
        assert len(rows) == len(index)
        dbl = lambda t: np.array([int(t, 16)], dtype=np.uint64).view(np.float64)[0]
        for k, t in zip(index, rows):
            assert int(t[1]) == Wt["n_valid"][k] and int(t[2]) == Wt["off_seed"][k] and dbl(t[3]).hex() == float(Wt["ll_seed"][k]).hex(), (tag, k, t)
            if Wt["read_state"][k] == NONE:
                continue
            assert int(t[4]) == Wt["off_second"][k] and int(t[8]) == Wt["d_end"][k], (tag, k, t)
            for i, f in ((5, "ll_second"), (6, "ll_flat"), (7, "ll_gapped")):
                assert dbl(t[i]).hex() == float(Wt[f][k]).hex(), (tag, k, f)
            if Wt["read_state"][k] == RECRUITED:
                assert int(t[9]) == Wt["draw_isz"][k]
            total += 1
    assert total > 300


def test_recruit_writer_format(tmp_path):
    """fighost_run_write_recruit on hand-made arrays: `g contig start G0 n n_candidates n_recruited C O`, one character per unmapped read,
    the recruited offsets in read order"""
    root = util.extract_golden("unmapped_small", str(tmp_path))
    exp = _gapout(root)
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        glen = np.zeros(max(n, 1), dtype=np.int32); nu = np.zeros(max(n, 1), dtype=np.int64); npp = np.zeros(max(n, 1), dtype=np.int64)
        host.fighost_run_sizes(h, api._p(glen, api.c_i32_p), api._p(nu, api.c_i64_p), api._p(npp, api.c_i64_p))
        uo = np.concatenate([[0], np.cumsum(nu[:n])]).astype(np.int64)
        NU = int(uo[-1])
        fl = np.arange(3, 3 + n, dtype=np.int32)
        rs = (np.arange(NU) % 6).astype(np.uint8); off = (np.arange(NU) * 7 - 40).astype(np.int32)
        ncand = np.arange(n, dtype=np.int32) + 2; nrec = np.arange(n, dtype=np.int32)
        err = C.create_string_buffer(512)
        cwd = os.getcwd(); os.chdir(root)
        try:
            rc = host.fighost_run_write_recruit(h, api._p(fl, api.c_i32_p), api._p(rs, api.c_u8_p), api._p(off, api.c_i32_p), api._p(ncand, api.c_i32_p), api._p(nrec, api.c_i32_p), err, 512)
            got = util.read(os.path.join(root, "tmp", "gaprecruit.txt"))
        finally:
            os.chdir(cwd)
    finally:
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    want = ""
    for g in range(n):
        ks = range(int(uo[g]), int(uo[g + 1]))
        want += "\t".join(exp[g][:4]) + f"\t{fl[g]}\t{ncand[g]}\t{nrec[g]}\t" + "".join(CHARS[int(rs[k])] for k in ks) + "\t" + ",".join(str(int(off[k])) for k in ks if rs[k] == RECRUITED) + "\n"
    assert n >= 2 and NU >= 12 and got == want and "+" in got and "," in got


def test_figfill_names_a_missing_call(tmp_path):
    """FIGFILL_RECRUIT=1 on a library without fig_batch_recruit (the one-lane emulation) is an error that names the call, before anything
    is filled or written; Python refuses likewise; a margin that is no finite number >= 0 is an error that names the variable; the host
    library has the bindings"""
    host = api.load_host_library()
    for fn in ("fighost_recruit_gaps_on", "fighost_recruit_candidate", "fighost_recruit_outside", "fighost_recruit_before", "fighost_recruit_seeded", "fighost_recruit_score",
               "fighost_recruit_rule", "fighost_recruit_margin_ok", "fighost_recruit_merge", "fighost_recruit_char", "fighost_run_write_recruit"):
        assert hasattr(host, fn), fn
    root = util.extract_golden("unmapped_small", str(tmp_path))
    argv = util.meta(root)["fillgaps_argv"]
    r = util.run([util.EMU] + argv, root, {"FIGFILL_RECRUIT": "1"})
    assert r.returncode != 0 and "fig_batch_recruit" in r.stderr
    for bad in ("abc", "1.5x", "-1", "inf", "nan", "", "1e999"):
        r = util.run([util.FIGFILL] + argv, root, {"FIGFILL_RECRUIT": "1", "FIGFILL_RECRUIT_MARGIN": bad})
        assert r.returncode != 0 and "FIGFILL_RECRUIT_MARGIN" in r.stderr, bad
    for fn in ("gaprecruit.txt", "gapout.txt"):
        assert not os.path.exists(os.path.join(root, "tmp", fn)), fn
    emu = C.CDLL(util.EMULIB)
    assert not hasattr(emu, "fig_batch_recruit")
    eng = api.Engine(0, lib_path=util.EMULIB)
    try:
        eng.n_gaps = 0
        with pytest.raises(RuntimeError, match="fig_batch_recruit"):
            eng.fill_resident(recruit=True)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------- GPU
_Eng = tpo._Eng


def _no_call(I):
    return I.call.tobytes() == b"." * len(I.call) and I.call_end.tobytes() == b"." * len(I.call_end)


@pytest.mark.gpu
def test_withheld_reads_are_recruited_and_the_truth_restored(withheld):
    """fig_batch_recruit on the withheld case: every field the restatement's, bit for bit; Engine.indel on Recruit.result() calls exactly
    the two sites and Engine.polish on it ends every gap equal to the truth; on the unrecruited result Engine.indel makes no call and
    Engine.polish no edit"""
    H, Wt, kinds, truth = withheld
    with _Eng(H) as eng:
        res = H.result()
        I0 = eng.indel(res, H.origin)
        P0 = eng.polish(res, H.origin)
        assert _no_call(I0) and not P0.edit.any() and not P0.edit_end.any() and [s.tobytes() for s in P0.strings()] == [H.raw[int(H.str_off[g]):int(H.str_off[g + 1])].tobytes() for g in range(3)]
        R = eng.recruit(res, H.origin)
        compare(R, Wt)
        assert list(R.n_recruited) == list(Wt["n_candidates"]) and R.n_recruited[1] >= 15 and R.n_recruited[2] >= 15
        M = R.result()
        assert M.draw[0][:H.NU].tobytes() == R.draw_pos.tobytes() and M.raw is res.raw
        I1 = eng.indel(M, H.origin)
        calls = {int(i): chr(c) for i, c in enumerate(I1.call) if c != ord(".")}
        assert calls == {int(H.str_off[1]) + tie.HOMO_AT: "I", int(H.str_off[2]) + tie.UNIQUE_AT: "D"} and I1.call_end.tobytes() == b"..."
        tie.compare(I1, tie.expected(H.merged(Wt["draw_pos"], Wt["draw_isz"])))
        P1 = eng.polish(M, H.origin)
        assert [s.tobytes() for s in P1.strings()] == [truth.tobytes()] * 3 and list(P1.state) == [tpo.ON, tpo.ON | tpo.EDITED, tpo.ON | tpo.EDITED]
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_edges_on_the_device(edges):
    """the edge case, the ins = del = 0 case and the max_insert case: every field the restatement's, bit for bit, over buffers that came
    in as 0xFF bytes; the period-12 repeat with one substitution under margins just below, at and just above the difference"""
    H, Wt = edges
    with _Eng(H) as eng:
        R = eng.recruit(H.result(), H.origin)
        compare(R, Wt)
        k = int(H.u_off[_gap_index("p12sub")])
        D = float(Wt["ll_seed"][k] - Wt["ll_second"][k])
        for margin, want in ((math.nextafter(D, 0.0), RECRUITED), (D, AMBIGUOUS), (math.nextafter(D, math.inf), AMBIGUOUS)):
            Rm = eng.recruit(H.result(), H.origin, min_margin=margin)
            compare(Rm, expected(H, margin=margin))
            assert Rm.read_state[k] == want and (Rm.draw_pos[k] == 20) == (want == RECRUITED)
    for case in (flat_case(), maxinsert_case()):
        with _Eng(case) as eng:
            compare(eng.recruit(case.result(), case.origin), expected(case))


@pytest.mark.gpu
def test_off_means_off_and_every_einval():
    """trp.HandPlace's gap list with its off states (by origin, by header, partial evidence) under a cutoff of 10: the restatement over
    the gaps that are on; reads of off gaps are OFF with the caller's draw values; without origins the ORIGINAL gap is on too; a
    partial-mode model recruits nothing; a NULL member, a NULL draw_isz, a margin that is negative, infinite or NaN, a drawn offset of
    2^20 in a gap that is on and a freed batch are FIG_EINVAL."""
    H = trp.HandPlace()
    H.model.cutoff = 10
    H.draw_isz = np.where(H.draw_pos != INT_MIN, 500 + np.arange(len(H.draw_pos)), 0).astype(np.int32)
    Wt = expected(H)
    assert (Wt["read_state"] == RECRUITED).any() and (Wt["read_state"] == NONE).any() and (Wt["read_state"] == BELOW).any()
    with _Eng(H) as eng:
        R = eng.recruit(H.result(), H.origin)
        compare(R, Wt)
        assert list(R.state) == trp.STATE
        for g in np.flatnonzero(R.state == 0):
            ks = list(_reads_of(H, g))
            assert not R.read_state[ks].any() and list(R.draw_pos[ks]) == list(H.draw_pos[ks]) and list(R.draw_isz[ks]) == list(H.draw_isz[ks]) and R.n_candidates[g] == 0
        kept = R.read_state == KEPT
        assert kept.any() and R.draw_pos[kept].tobytes() == H.draw_pos[:H.NU][kept].tobytes() and R.draw_isz[kept].tobytes() == H.draw_isz[:H.NU][kept].tobytes()
        M = R.result()
        assert M.draw[0][H.NU:].tobytes() == H.draw_pos[H.NU:].tobytes() and M.draw[2].tobytes() == H.draw_len.tobytes()        # the partial part and the headers
        compare(eng.recruit(H.result(), None), expected(H, state=[1, 1, 1, 1, 1, 0, 0, 1, 1]))
        r, keep = eng._filled_struct("recruit", H.result())
        nu, n = H.NU, len(H.filled_len)
        bufs = {f: np.zeros(n if f in ("n_candidates", "n_recruited", "state") else nu, dtype=np.float64 if t is api.c_double_p else np.uint8 if t is api.c_u8_p else np.int32)
                for f, t in api.FigReadRecruit._fields_}

        def call(skip=None, margin=0.0, filled=r):
            rr = api.FigReadRecruit()
            for f, typ in api.FigReadRecruit._fields_:
                if f != skip:
                    setattr(rr, f, api._p(bufs[f], typ))
            return eng.lib.fig_batch_recruit(eng.ctx, C.byref(filled), None, C.c_double(margin), C.byref(rr))
        assert call() == 0
        for f, _ in api.FigReadRecruit._fields_:
            assert call(skip=f) == -1, f
        for bad in (-1.0, -1e-300, math.inf, -math.inf, math.nan):
            assert call(margin=bad) == -1, bad
        assert call(margin=1e300) == 0
        r2, keep2 = eng._filled_struct("recruit", H.result())
        r2.draw_isz = None
        assert call(filled=r2) == -1
        assert eng.lib.fig_batch_recruit(eng.ctx, C.byref(r), None, C.c_double(0.0), None) == -1 and eng.lib.fig_batch_recruit(eng.ctx, None, None, C.c_double(0.0), None) == -1
        for k, v, ok in ((int(H.u_off[2]) + 1, 1 << 20, False), (int(H.u_off[2]) + 1, -(1 << 20), False), (int(H.u_off[2]) + 1, (1 << 20) - 1, True), (int(H.u_off[6]) + 1, 1 << 20, True)):
            B = trp.HandPlace()
            B.draw_pos[k] = v
            if ok:
                eng.recruit(B.result(), B.origin)
            else:
                with pytest.raises(RuntimeError):
                    eng.recruit(B.result(), B.origin)
        with pytest.raises(RuntimeError):
            eng.recruit(H.result(), H.origin, min_margin=-0.5)
        eng.free_batch()
        with pytest.raises(RuntimeError):
            eng.recruit(H.result(), H.origin)
    Pm = trp.HandPlace(mode="partial")
    with _Eng(Pm) as eng:
        R = eng.recruit(Pm.result(), Pm.origin)
        assert len(R.draw_pos) == 0 and not R.state.any() and not R.n_candidates.any() and not R.n_recruited.any()


@pytest.mark.gpu
def test_deterministic_and_read_only(withheld, edges):
    """a second call returns the same bytes; fig_batch_indel on the caller's `filled` before and after the call returns the same bytes;
    the caller's `filled` is unchanged"""
    for H in (withheld[0], edges[0]):
        with _Eng(H) as eng:
            res = H.result()
            before = [np.array(a).tobytes() for a in (res.filled_len, res.str_off, res.raw) + tuple(res.draw)]
            I0 = eng.indel(res, H.origin)
            R0 = eng.recruit(res, H.origin)
            I1 = eng.indel(res, H.origin)
            R1 = eng.recruit(res, H.origin)
            for f, _ in api.FigGapIndel._fields_:
                assert np.asarray(getattr(I0, f)).tobytes() == np.asarray(getattr(I1, f)).tobytes(), f
            for f, _ in api.FigReadRecruit._fields_:
                assert np.asarray(getattr(R0, f)).tobytes() == np.asarray(getattr(R1, f)).tobytes(), f
            assert before == [np.array(a).tobytes() for a in (res.filled_len, res.str_off, res.raw) + tuple(res.draw)]


class _GoldenView:
    """a golden's fill under the attribute names expected() reads"""

    def __init__(self, F, state):
        self.NU, self.filled_len, self.str_off, self.raw, self.u_off, self.draw_pos, self.draw_isz, self.rev, self.pos = F.nu, F.filled_len, F.str_off, F.raw, F.u_off, F.draw_pos, F.draw_isz, F.u_rev, F.u_pos
        self.seqs = [F.u_seq[int(F.u_seq_off[k]):int(F.u_seq_off[k + 1])] for k in range(F.nu)]
        self.state = state
        self.F = F

    def geometry(self, g):
        F = self.F
        c = int(F.gap_contig[g])
        return F.contig[int(F.contig_off[c]):int(F.contig_off[c + 1])], int(F.start[g]), int(F.G0[g])


def run_golden_recruit(root):
    """A golden filled as figfill fills it (draw and support planes), then the recruit and, on its merged plane, the indel pass and the
    polish while the batch is resident, then a second plain fill -> Fill with .R, .I, .P, .second and what the restatement needs"""
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        ids = np.arange(max(n, 1), dtype=np.int64)
        cm = api.FigModel(); host.fighost_run_model(h, C.byref(cm))
        cb = api.FigGapBatch(); su = C.c_int64(); sp = C.c_int64()
        assert host.fighost_run_shard(h, api._p(ids, api.c_i64_p), n, C.byref(cb), C.byref(su), C.byref(sp)) == 0
        F = Fill()
        nu = int(su.value)
        F.G0 = np.ctypeslib.as_array(cb.gap_len, shape=(n,)).copy(); F.start = np.ctypeslib.as_array(cb.gap_start, shape=(n,)).copy()
        F.gap_contig = np.ctypeslib.as_array(cb.gap_contig, shape=(n,)).copy()
        nc = int(cb.n_contigs)
        F.contig_off = np.ctypeslib.as_array(cb.contig_off, shape=(nc + 1,)).copy()
        F.contig = np.frombuffer(cb.contig_seq or b"", dtype=np.uint8)
        F.u_off = np.ctypeslib.as_array(cb.u_read_off, shape=(n + 1,)).copy()
        F.u_seq_off = np.ctypeslib.as_array(cb.u_seq_off, shape=(nu + 1,)).copy()
        F.u_seq = np.frombuffer(cb.u_seq or b"", dtype=np.uint8)
        F.u_rev = np.ctypeslib.as_array(cb.u_is_reverse, shape=(nu,)).copy()
        F.u_pos = np.ctypeslib.as_array(cb.u_anchor_pos, shape=(nu,)).copy()
        F.tabs = tables(cm); F.unmapped = bool(cm.unmapped_flag); F.nu = nu; F.cutoff = int(cm.gap_prob_cutoff)
        eng = api.Engine(0)
        try:
            eng.set_model_struct(cm)
            eng.upload_struct(cb)
            reach = np.zeros(max(n, 1), dtype=np.uint8); reach[:n] = eng.probe_reach()
            preset = np.zeros(max(n, 1), dtype=np.uint8)
            host.fighost_run_ot_presets(h, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
            eng.set_ot_preset(preset[:n])
            res = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, recruit=True, indel=True, polish=True, keep_resident=True)
            F.second = _take(Fill(), eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.R, F.I, F.P = res.recruit, res.indel, res.polish
        return F
    finally:
        host.fighost_run_close(h)


@pytest.fixture(scope="module")
def rfills(tmp_path_factory):
    """name -> golden filled with the draw and support planes, the recruit and the passes on its merged plane; computed once per module"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden_recruit(util.extract_golden(name, str(tmp_path_factory.mktemp(name))))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "bench_b160"])
def test_goldens_end_to_end(name, rfills):
    """A golden filled as figfill fills it, then the recruit: states by the rule and every field the restatement's, bit for bit -- over
    all gaps of unmapped_small and over the first four gaps of bench_b160, where the device runs on all gaps; the counts by state are
    printed; a second fill of the still resident batch returns the bytes of the first."""
    F = rfills(name)
    assert F.unmapped
    state = []
    for g in range(F.n):
        n = int(F.filled_len[g]); org = int(F.origin[g])
        state.append(int(n > 0 and int(F.draw_len[2 * g]) == n and int(F.draw_len[2 * g + 1]) < 0 and bool(org & F_) and not org & O_))
    assert list(F.R.state) == state and sum(state) > 0
    V = _GoldenView(F, state)
    gaps = None if name == "unmapped_small" else list(range(min(4, F.n)))
    Wt = expected(V, tabs=F.tabs, cutoff=F.cutoff, gaps=gaps)
    if gaps is None:
        compare(F.R, Wt)
    else:
        mask = np.zeros(F.nu, dtype=bool)
        for g in gaps:
            mask[int(F.u_off[g]):int(F.u_off[g + 1])] = True
        compare(F.R, Wt, reads=mask)
        assert list(F.R.n_candidates[gaps]) == list(Wt["n_candidates"][gaps]) and list(F.R.n_recruited[gaps]) == list(Wt["n_recruited"][gaps])
    cnt = np.bincount(F.R.read_state, minlength=6)
    print(f"{name}: gaps on {sum(state)} of {F.n}, cutoff {F.cutoff}, reads {F.nu}: off {cnt[OFF]}, kept {cnt[KEPT]}, none {cnt[NONE]}, below {cnt[BELOW]}, ambiguous {cnt[AMBIGUOUS]}, "
          f"recruited {cnt[RECRUITED]}; columns called on the merged plane {int((F.I.call != ord('.')).sum())}, polish inserted {int(F.P.n_ins.sum())}, removed {int(F.P.n_del.sum())}")
    assert int(F.R.n_candidates.sum()) == int(cnt[NONE] + cnt[BELOW] + cnt[AMBIGUOUS] + cnt[RECRUITED]) and int(F.R.n_recruited.sum()) == int(cnt[RECRUITED])
    for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
        assert np.array_equal(getattr(F, f), getattr(F.second, f)), f


@pytest.mark.gpu
def test_gaprecruit_file_is_the_same_from_every_host_path(rfills, tmp_path, monkeypatch):
    """unmapped_small with FIGFILL_RECRUIT=1, FIGFILL_INDEL=1 and FIGFILL_POLISH=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0
    and two-rank figfill_mp leave the same gaprecruit.txt, which is the file of Engine.recruit's result, and the gapindel.txt and
    gappolished.txt of the API composition recruit -> indel / polish; the reference's files stay byte-identical in every run; without
    the variable the file is absent and gapout.txt, draw.txt and filledContigs.fa are what the runs with it wrote."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    name = "unmapped_small"
    for v in ("FIGFILL_SUPPORT", "FIGFILL_QUALITY", "FIGFILL_PLACEMENT", "FIGFILL_QUALITY_MINPQ", "FIGFILL_SOFTQUALITY", "FIGFILL_INDEL", "FIGFILL_POLISH", "FIGFILL_POLISH_ROUNDS",
              "FIGFILL_RECRUIT", "FIGFILL_RECRUIT_MARGIN"):
        monkeypatch.delenv(v, raising=False)
    roots = [util.extract_golden(name, str(tmp_path / f"r{k}")) for k in range(4)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    on = {"FIGFILL_RECRUIT": "1", "FIGFILL_INDEL": "1", "FIGFILL_POLISH": "1"}
    r = util.run([util.FIGFILL] + argv, roots[3])
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[0], on)
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[1], dict(on, FIGFILL_DEVICES="0,0"))
    assert r.returncode == 0, r.stderr
    for k, v in on.items():
        monkeypatch.setenv(k, v)                                  # the spawned ranks inherit them
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_mp_worker, args=(k, 2, port, roots[2], name, q, None)) for k in range(2)]
    for p in ps:
        p.start()
    outs = [q.get(timeout=600) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(rc == 0 for _, rc in outs)
    F = rfills(name)
    exp = _gapout(roots[0])
    for fn in ("gaprecruit.txt", "gapindel.txt", "gappolished.txt"):
        files = [util.read(os.path.join(root, "tmp", fn)) for root in roots[:3]]
        assert files[0] == files[1] == files[2], fn
    lines = util.read(os.path.join(roots[0], "tmp", "gaprecruit.txt")).splitlines()
    assert len(lines) == len(exp) == F.n
    for g, (ln, e) in enumerate(zip(lines, exp)):
        f = ln.split("\t")
        ks = range(int(F.u_off[g]), int(F.u_off[g + 1]))
        assert len(f) == 9 and f[:5] == e[:5] and f[5:7] == [str(int(F.R.n_candidates[g])), str(int(F.R.n_recruited[g]))]
        assert f[7] == "".join(CHARS[int(F.R.read_state[k])] for k in ks) and f[8] == ",".join(str(int(F.R.off_seed[k])) for k in ks if F.R.read_state[k] == RECRUITED)
    strs = F.P.strings()
    for g, (li_, lp) in enumerate(zip(util.read(os.path.join(roots[0], "tmp", "gapindel.txt")).splitlines(), util.read(os.path.join(roots[0], "tmp", "gappolished.txt")).splitlines())):
        a, n = int(F.str_off[g]), max(int(F.filled_len[g]), 0)
        assert li_.split("\t")[5:] == [str(int(F.I.state[g])), F.I.call[a:a + n].tobytes().decode(), chr(int(F.I.call_end[g]))], g
        assert lp.split("\t")[5:] == [str(int(F.P.polished_len[g])), str(int(F.P.state[g])), str(int(F.P.n_ins[g])), str(int(F.P.n_del[g])), strs[g].tobytes().decode()], g
    for k, root in enumerate(roots):
        assert os.path.exists(os.path.join(root, "tmp", "gaprecruit.txt")) == (k < 3)
        assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
        for fn in ("gapout.txt", "draw.txt", "filledContigs.fa"):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(roots[3], "tmp", fn)), (root, fn)
