"""Placement confidence per drawn unmapped read (fig_read_placement / fig_batch_placement, include/figbird_hip.h).

There is no reference for this feature; the header's definition is the specification.  The comparisons use a numpy restatement of
it: per read, the offsets -(len-1) .. n-1 as one vector, the closed-form insert size and the validity rule on it, then
`Lr = li[isz]` and one vectorised `Lr = Lr + t_j` per read base in ascending j (np.sum would reorder and is not used).  The tables
come from fighost_quality_tables and fighost_placement_li, the code the library runs.  The device only adds table entries in that
order and compares, so ll_drawn, ll_other, off_other, n_valid and state are compared with no tolerance (doubles on the int64 view).

sum_other is a sum of at most 800 positive terms that the device may add in any order with its own exp10: the bound is
|d| <= 1e-11 * want + 1e-300 (any exp10 good to a few ulp -- even exp(x * ln 10) at |x| <= 700 -- stays below 2e-13 relative, so
1e-11 leaves a factor of 50; the absolute term covers denormal sums).  The restatement sums with math.fsum."""
import ctypes as C
import math
import os
import re
import socket
import subprocess
import tempfile

import numpy as np
import pytest

import util
from figbird_amd import api
import test_base_quality as tbq
from test_base_support import CODE, INT_MIN, Fill, _gapout, _open_run, _take

NINF = -math.inf
LQ = float.fromhex("-0x1.34413509f79ffp-1")
FLANK = 208
READ_LENS = (31, 77, 150, 200)
F_, O_, T_ = api.SUP_FINAL, api.SUP_ORIGINAL, api.SUP_TIEBREAK


# ------------------------------------------------------------------------------------- the restatement
def place_tables(cm):
    """fig_model struct -> (lm, le, lt [4, 4], li [max_insert], Tmin, Tmax, max_insert)"""
    host = api.load_host_library()
    lm, le, lt = tbq.tables(cm)
    li = np.zeros(int(cm.max_insert_size))
    assert host.fighost_placement_li(C.byref(cm), api._p(li, api.c_double_p)) == 0
    return lm, le, lt, li, int(cm.insert_threshold_min), int(cm.insert_threshold_max), int(cm.max_insert_size)


def isz_of(pos, gap_start, G0, n, ln, o):
    """the closed form of the header, on an int64 vector of offsets (or one offset)"""
    o = np.asarray(o, dtype=np.int64)
    return gap_start - pos + ln + o if pos < gap_start else pos + (n - G0) - gap_start + ln - o


def columns(contig, gap_start, G0, string):
    """codes of the columns -199 .. n+198 of a gap: element 199 + x is column x"""
    n = len(string)
    x = np.arange(-199, n + 199, dtype=np.int64)
    p = np.where(x < 0, gap_start + x, gap_start + G0 + (x - n))
    inside = (p >= 0) & (p < len(contig))
    S = np.where(inside, CODE[contig[np.clip(p, 0, len(contig) - 1)]], 4)
    S[199:199 + n] = CODE[string]
    return S


def phred_of(ll_drawn, ll_other, sum_other):
    host = api.load_host_library()
    a, b, c = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (ll_drawn, ll_other, sum_other))
    out = np.full(max(len(a), 1), 0xFF, dtype=np.uint8)
    if len(a):
        host.fighost_placement_phred(len(a), api._p(a, api.c_double_p), api._p(b, api.c_double_p), api._p(c, api.c_double_p), api._p(out, api.c_u8_p))
    return out[:len(a)]


def restate_read(S, n, seq, rev, pos, ostar, gap_start, G0, tabs):
    """one scored read -> dict of the header's outputs and `q` = -10 log10(perr) + 0.5 before the floor (None where pq is not
    taken from it)"""
    lm, le, lt, li, Tmin, Tmax, MI = tabs
    ln = len(seq)
    o = np.arange(-(ln - 1), n, dtype=np.int64)
    isz = isz_of(pos, gap_start, G0, n, ln, o)
    ok = (isz >= Tmin) & (isz <= Tmax) & (isz >= 0) & (isz < MI)
    o, isz = o[ok], isz[ok]
    Lr = li[isz].copy()
    s = CODE[seq]
    for j in range(ln):
        if s[j] > 3:
            continue
        k = ln - 1 - j if rev else j
        c = S[199 + o + j]
        with np.errstate(invalid="raise"):
            Lr = Lr + np.where(c > 3, LQ, np.where(c == s[j], lm[k], le[k] + lt[c & 3, s[j]]))
    assert not np.isnan(Lr).any()
    drawn = o == ostar
    ll_drawn = float(Lr[drawn][0]) if drawn.any() else NINF
    oth, Lo = o[~drawn], Lr[~drawn]
    if len(oth):
        i = int(np.argmax(Lo))                                  # the first of equal maxima = the smallest offset
        ll_other, off_other = float(Lo[i]), int(oth[i])
    else:
        ll_other, off_other = NINF, INT_MIN
    M = max(ll_drawn, ll_other)
    sum_other = 0.0 if M == NINF else math.fsum(float(10.0 ** (v - M)) for v in Lo if v > NINF)
    q = None
    if ll_drawn > NINF:
        perr = sum_other / (sum_other + 10.0 ** (ll_drawn - M))
        q = None if perr == 0 else -10 * math.log10(perr) + 0.5
    pq = int(phred_of(ll_drawn, ll_other, sum_other)[0])
    return dict(ll_drawn=ll_drawn, ll_other=ll_other, off_other=off_other, n_valid=int(len(o)), sum_other=sum_other, pq=pq, q=q)


def unscored(nu):
    return dict(ll_drawn=np.zeros(nu), ll_other=np.zeros(nu), sum_other=np.zeros(nu), off_other=np.full(nu, INT_MIN, dtype=np.int32),
                n_valid=np.zeros(nu, dtype=np.int32), pq=np.full(nu, 255, dtype=np.uint8), q=[None] * nu)


def same_bits(a, b):
    return tbq.same_bits(a, b)


def compare(P, want, scored):
    """the device's arrays against the restatement's: the exact ones bit for bit over ALL reads, sum_other inside its bound, pq the
    host function of the returned arrays and the restatement's wherever that is not within 1e-9 of a rounding boundary"""
    for f in ("ll_drawn", "ll_other"):
        bad = np.flatnonzero(np.asarray(getattr(P, f)).view(np.int64) != np.asarray(want[f]).view(np.int64))
        assert not len(bad), f"{f}: reads {bad[:8]}: got {getattr(P, f)[bad[:4]]}, want {want[f][bad[:4]]}"
    for f in ("off_other", "n_valid"):
        bad = np.flatnonzero(np.asarray(getattr(P, f)) != want[f])
        assert not len(bad), f"{f}: reads {bad[:8]}: got {getattr(P, f)[bad[:4]]}, want {want[f][bad[:4]]}"
    d = np.abs(P.sum_other - want["sum_other"])
    lim = 1e-11 * want["sum_other"] + 1e-300
    rel = d[scored] / np.maximum(want["sum_other"][scored], 1e-300)
    print(f"sum_other: {int(scored.sum())} scored reads, largest |d| / want = {rel.max() if len(rel) else 0:.3e}")
    assert (d[~scored] == 0).all() and (P.sum_other[~scored] == 0).all()
    assert (d <= lim).all(), f"reads {np.flatnonzero(d > lim)[:8]}"
    assert np.array_equal(P.pq[scored], phred_of(P.ll_drawn[scored], P.ll_other[scored], P.sum_other[scored]))
    assert (P.pq[~scored] == 255).all() and (P.pq[scored] <= 60).all()
    far = np.array([scored[r] and (want["q"][r] is None or abs(want["q"][r] - round(want["q"][r])) > 1e-9) for r in range(len(scored))], dtype=bool)
    assert np.array_equal(P.pq[far], want["pq"][far])
    return far


# ------------------------------------------------------------------------------------- the hand-made case
def place_model(mode="unmapped"):
    """tbq.hand_model's e[k] (all different, e[17] = 0) and matrix (distinct off-diagonals, C->G = 0); a flat insert-size table
    of 1200 entries, one of them 0, with the thresholds 150 and 1000 inside it"""
    m = tbq.hand_model(mode)
    insd = np.full(1200, 1.0 / 1200)
    insd[500] = 0.0
    m.insd, m.Tmin, m.Tmax = insd, 150, 1000
    return m


UNIT = np.frombuffer(b"ACGGTCATTGCA", dtype=np.uint8)          # the period-12 unit of the tandem gap: no shorter period
G0 = 50
# (n, unmapped reads, partial reads, evidence, draw header, origin, what)
GAPS = [(1, 3, 0, "u", 1, F_, "start"), (65, 70, 0, "u", 65, F_ | T_, ""), (257, 130, 0, "u", 257, F_, ""), (600, 40, 0, "u", 600, F_, ""),
        (100, 5, 0, "u", 100, F_ | O_, ""), (100, 5, 3, "p", 100, F_, ""), (100, 5, 0, "u", 101, F_, ""), (12, 6, 0, "u", 12, F_, "tandem"),
        (300, 20, 0, "u", 300, F_, "end")]
STATE = [1, 1, 1, 1, 0, 0, 0, 1, 1]
SEED = 20261019


class HandPlace:
    """A resident batch and a `filled` made by hand, no fill.  Gap 0 lies 120 bases from the contig start, the last gap ends 100
    bases before the contig end (both fewer than len - 1 for the longer reads: N columns beyond the contig).  A read is a copy of
    the gap's sequence at a true offset with a few substitutions, its anchor chosen so that the true offset has a given insert
    size; most reads are drawn at the true offset.  gaps / state: another gap list than GAPS (which alone gets the repeat of gap
    2, the Ns beside gap 3 and the all -inf read) and the states it is to have; lens: the read lengths, dealt in turn; last_n: the
    first read of every length ends in an N."""

    def __init__(self, seed=SEED, mode="unmapped", gaps=GAPS, state=STATE, lens=READ_LENS, last_n=False):
        rng = np.random.default_rng(seed)
        self.model = place_model(mode)
        self.gaps = gaps
        ng = len(gaps)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        starts, p = [], 120
        for g in range(ng):
            starts.append(p); p += G0 + 420
        clen = starts[-1] + G0 + 100
        contig = rng.choice(acgt, size=clen).copy()
        if gaps is GAPS:
            contig[starts[3] - 40] = ord("N"); contig[starts[3] + G0 + 7] = ord("N")       # N in either flank of gap 3
        self.starts = np.array(starts, dtype=np.int64)
        self.filled_len = np.array([g[0] for g in gaps], dtype=np.int32)
        self.str_off = np.concatenate([[0], np.cumsum(self.filled_len)]).astype(np.int64)
        self.raw = rng.choice(np.frombuffer(b"ACGTACGTACGTACGTACGTN", dtype=np.uint8), size=int(self.str_off[-1])).copy()
        a = int(self.str_off[2]) if gaps is GAPS else None
        if a is not None:                # gap 2: the second half of the string repeats the first but for five bases, so that reads
            self.raw[a + 128:a + 256] = self.raw[a:a + 128]                    # there have a second placement one or two substitutions away
            for x in (5, 40, 47, 90, 121):
                self.raw[a + 128 + x] = acgt[(int(CODE[self.raw[a + x]]) + 1 + x % 3) % 4]
        ph = lambda x: UNIT[np.mod(x, 12)]
        for tg in [g for g in range(ng) if gaps[g][6] == "tandem"]:
            contig[starts[tg] - 300:starts[tg]] = ph(np.arange(-300, 0))
            contig[starts[tg] + G0:starts[tg] + G0 + 300] = ph(gaps[tg][0] + np.arange(300))
            self.raw[int(self.str_off[tg]):int(self.str_off[tg + 1])] = ph(np.arange(gaps[tg][0]))
        for st in starts:
            contig[st:st + G0] = ord("N")
        self.contig = contig
        self.S = [columns(contig, starts[g], G0, self.raw[int(self.str_off[g]):int(self.str_off[g + 1])]) for g in range(ng)]
        u_off, p_off, seqs, pos, rev, draw, pseqs = [0], [0], [], [], [], [], []
        for g, (n, nu, npart, ev, dl, org, what) in enumerate(gaps):
            for r in range(nu):
                ln = (31, 31, 31, 77, 77, 31)[r] if what == "tandem" else lens[r % len(lens)]
                t = int(rng.integers(-(ln - 1), n))
                s = np.frombuffer(b"ACGTN", dtype=np.uint8)[self.S[g][199 + t + np.arange(ln)]].copy()
                s[s == ord("N")] = rng.choice(acgt, size=int((s == ord("N")).sum()))
                left = (r // 2) % 2 == 0
                if what == "tandem":
                    I = 800
                else:
                    s[rng.choice(ln, size=min(ln, int(rng.integers(0, 4))), replace=False)] = rng.choice(acgt)
                    if r % 5 == 4:
                        s[rng.choice(ln, size=min(ln, 2), replace=False)] = ord("N")
                    if last_n and r < len(lens):
                        s[-1] = ord("N")
                    I = int(rng.integers(150, 1001))
                    if r % 17 == 16:
                        I = 5000                                      # no valid placement at all
                # the anchor that gives the true offset insert size I (and keeps the side: left anchors lie before the gap)
                a = starts[g] + ln + t - I if left else I - (n - G0) + starts[g] - ln + t
                if left and a >= starts[g]:
                    a = starts[g] - 1 - int(rng.integers(0, 50))
                if not left and a < starts[g]:
                    a = starts[g] + int(rng.integers(0, 50))
                o = t
                if what != "tandem":
                    if r % 7 == 6:
                        o = INT_MIN                                   # not drawn
                    elif r % 11 == 10:
                        o = n + 2                                     # drawn where no placement is
                    elif r % 13 == 12:
                        o = -(ln + 1)
                    elif r % 9 == 8:
                        o = int(rng.integers(-(ln - 1), n))           # drawn somewhere else
                seqs.append(s); pos.append(int(a)); rev.append(r % 2); draw.append(o)
            u_off.append(u_off[-1] + nu)
            for r in range(npart):
                pseqs.append(rng.choice(acgt, size=77).copy())
            p_off.append(p_off[-1] + npart)
        # the read whose every valid placement is -inf: read 1 of gap 0 (n = 1, length 77, reversed: k = 17 is base 59, left
        # anchor) gets the anchor that leaves it the three placements -2, -1, 0 (insert sizes 150, 151, 152), is drawn at 0, and
        # gets at base 59 a base that differs from the three columns under it: e[17] = 0 makes each of them -inf
        if gaps is GAPS:
            assert len(seqs[1]) == 77 and rev[1] == 1
            pos[1] = starts[0] + 77 - 152; draw[1] = 0
            under = {int(c) for c in self.S[0][199 + 59 + np.array([-2, -1, 0])]}
            assert 4 not in under
            seqs[1][59] = acgt[min(set(range(4)) - under)]
            seqs[1][seqs[1] == ord("N")] = ord("A")
        self.NU, NP = u_off[-1], p_off[-1]
        cat = lambda v: np.concatenate(v) if v else np.zeros(1, dtype=np.uint8)
        soff = lambda v: np.concatenate([[0], np.cumsum([len(s) for s in v])]).astype(np.int64)
        i32 = lambda v: np.asarray(v if len(v) else [0], dtype=np.int32)
        self.seqs, self.pos, self.rev = seqs, pos, np.asarray(rev, dtype=np.uint8)
        self.u_off, self.p_off = np.asarray(u_off, dtype=np.int64), np.asarray(p_off, dtype=np.int64)
        self.batch = api.GapBatch(
            contig_off=np.array([0, clen], dtype=np.int64), contig_seq=contig,
            gap_contig=np.zeros(ng, dtype=np.int32), gap_start=self.starts, gap_len=np.full(ng, G0, dtype=np.int32),
            gap_stat2=np.zeros(3 * ng, dtype=np.int32), gap_fillflag=np.ones(ng, dtype=np.int32),
            u_read_off=self.u_off, u_anchor_pos=i32(pos), u_is_reverse=self.rev, u_seq_off=soff(seqs), u_seq=cat(seqs),
            p_read_off=self.p_off, p_clipped_index=i32([10] * NP), p_match=i32([1 + r % 4 for r in range(NP)]), p_pos=i32([100] * NP),
            p_ref_pos=i32([-1] * NP), p_seq_off=soff(pseqs), p_seq=cat(pseqs), p_qual=np.full(max(int(soff(pseqs)[-1]), 1), ord("I"), dtype=np.uint8),
            gap_ot_preset=np.zeros(ng, dtype=np.uint8) if mode == "partial" else None)
        nu_planes = self.NU if mode == "unmapped" else 0       # a partial-mode upload packs no unmapped reads
        self.draw_pos = i32((draw if nu_planes else []) + [5] * NP)
        self.draw_isz = np.zeros(len(self.draw_pos), dtype=np.int32)
        self.draw_len = np.full(2 * ng, -1, dtype=np.int32)
        for g, (n, _, _, ev, dl, _, _) in enumerate(gaps):
            self.draw_len[2 * g + (1 if ev == "p" else 0)] = dl
        self.origin = np.array([g[5] for g in gaps], dtype=np.int32)
        self.state = np.array(state if mode == "unmapped" else [0] * ng, dtype=np.uint8)

    def scored(self):
        out = np.zeros(self.NU, dtype=bool)
        for g in range(len(self.gaps)):
            if self.state[g]:
                for k in range(int(self.u_off[g]), int(self.u_off[g + 1])):
                    out[k] = self.draw_pos[k] != INT_MIN
        return out

    def expected(self):
        """the restatement over every scored read -> dict of arrays (q: list)"""
        tabs = place_tables(self.model.cstruct())
        w = unscored(self.NU)
        sc = self.scored()
        for g in range(len(self.gaps)):
            for k in range(int(self.u_off[g]), int(self.u_off[g + 1])):
                if sc[k]:
                    r = restate_read(self.S[g], int(self.filled_len[g]), self.seqs[k], int(self.rev[k]), self.pos[k], int(self.draw_pos[k]), int(self.starts[g]), G0, tabs)
                    for f, v in r.items():
                        w[f][k] = v
        return w

    def result(self):
        return api.FillResult(self.filled_len, np.zeros_like(self.filled_len), None, str_off=self.str_off, raw=self.raw,
                              draw=(self.draw_pos, self.draw_isz, self.draw_len))


@pytest.fixture(scope="module")
def hand():
    """the hand-made case and its restatement: built once, never modified"""
    H = HandPlace()
    return H, H.expected()


EDGE_LENS = tbq.EDGE_LENS


@pytest.fixture(scope="module")
def hand_edge():
    """One gap of 40 columns with 65 unmapped reads (one chunk boundary) of the lengths at which a staged read's layout changes
    (tbq.hand_edge_lengths), the first read of every length ending in an N; and its restatement.  Built once, never modified."""
    H = HandPlace(seed=20261020, gaps=[(40, 65, 0, "u", 40, F_, "")], state=[1], lens=EDGE_LENS, last_n=True)
    return H, H.expected()


def test_edge_length_case_is_valid(hand_edge):
    """Every length of the edge-length case has a scored read drawn on the string with a valid drawn placement, and a read whose
    last base is N."""
    H, W = hand_edge
    sc = H.scored()
    assert list(H.state) == [1] and H.NU == 65 and {len(s) for s in H.seqs} == set(EDGE_LENS)
    for ln in EDGE_LENS:
        ks = [k for k in range(65) if len(H.seqs[k]) == ln]
        assert any(sc[k] and -(ln - 1) <= H.draw_pos[k] <= 39 and np.isfinite(W["ll_drawn"][k]) and W["n_valid"][k] > 1 for k in ks), f"no scored read of length {ln} on the string"
        assert any(H.seqs[k][-1] == ord("N") for k in ks), f"no read of length {ln} ends in N"


def test_hand_case_is_not_vacuous(hand):
    """The hand-made case holds what it is meant to exercise, and no read of the restatement lies within 1e-9 of a rounding
    boundary of its Phred (the seed is chosen so)."""
    H, W = hand
    sc = H.scored()
    nplace = np.array([H.filled_len[g] + len(H.seqs[k]) - 1 for g in range(len(GAPS)) for k in range(int(H.u_off[g]), int(H.u_off[g + 1]))])
    gap_of = np.repeat(np.arange(len(GAPS)), np.diff(H.u_off))
    assert list(H.state) == STATE and sc.sum() > 200 and (~sc).sum() > 30
    assert {len(s) for s in H.seqs} == set(READ_LENS) and set(H.rev[sc]) == {0, 1}
    left = np.array([H.pos[k] < H.starts[gap_of[k]] for k in range(H.NU)])
    assert left[sc].any() and (~left[sc]).any()
    assert np.isneginf(W["ll_drawn"][sc]).any() and np.isfinite(W["ll_drawn"][sc]).any()
    assert np.isneginf(W["ll_other"][sc]).any() and np.isfinite(W["ll_other"][sc]).any()
    assert ((W["n_valid"] > 0) & np.isneginf(W["ll_drawn"]) & np.isneginf(W["ll_other"]) & sc).any(), "a read whose placements are all -inf"
    assert ((W["n_valid"] == 0) & sc).any() and (W["off_other"][(W["n_valid"] == 0) & sc] == INT_MIN).all()
    assert ((W["n_valid"] > 0) & (W["n_valid"] < nplace) & sc).any() and ((W["n_valid"] == nplace) & sc).any()      # thresholds cut / do not cut
    cut_lo = cut_hi = False
    cm = H.model.cstruct()
    for k in np.flatnonzero(sc):
        g = gap_of[k]; n = int(H.filled_len[g]); ln = len(H.seqs[k])
        i = isz_of(H.pos[k], int(H.starts[g]), G0, n, ln, np.array([-(ln - 1), n - 1]))
        cut_lo |= bool(i.min() < cm.insert_threshold_min <= i.max()); cut_hi |= bool(i.min() <= cm.insert_threshold_max < i.max())
    assert cut_lo and cut_hi
    drawn_invalid = sc & np.isneginf(W["ll_drawn"]) & np.array([not (-(len(H.seqs[k]) - 1) <= H.draw_pos[k] <= H.filled_len[gap_of[k]] - 1) for k in range(H.NU)])
    assert drawn_invalid.any() and (W["pq"][drawn_invalid] == 0).all()
    assert any((s == ord("N")).any() for k, s in enumerate(H.seqs) if sc[k]) and (H.raw == ord("N")).any()
    assert (H.S[0][:199 - 120] == 4).all() and (H.S[-1][199 + 300 + 100:] == 4).all() and (H.S[3] == 4).sum() >= 2     # beyond the contig; N in the flanks
    assert (W["ll_other"] > W["ll_drawn"])[sc].any() and (W["ll_other"] < W["ll_drawn"])[sc].any()
    assert len(set(W["pq"][sc])) > 5 and (W["sum_other"][sc] > 0).any()
    assert all(q is None or abs(q - round(q)) > 1e-9 for q in W["q"])
    assert not sc[int(H.u_off[4]):int(H.u_off[7])].any()


def test_tandem_repeat_by_hand(hand):
    """In the period-12 gap every read is an exact copy and the insert-size table is flat over its placements: the copies a
    multiple of 12 away score the same bits, off_other is the first of them, and the Phred is that of c equal placements,
    floor(-10 log10((c - 1) / c) + 0.5) -- the other placements carry at least four substitutions each (< 1e-9 of a copy)."""
    H, W = hand
    g = [i for i in range(len(GAPS)) if GAPS[i][6] == "tandem"][0]
    n = GAPS[g][0]
    for k in range(int(H.u_off[g]), int(H.u_off[g + 1])):
        ln, o = len(H.seqs[k]), int(H.draw_pos[k])
        copies = [x for x in range(-(ln - 1), n) if (x - o) % 12 == 0]
        c = len(copies)
        assert W["n_valid"][k] == n + ln - 1 and c >= 3
        assert same_bits([W["ll_other"][k]], [W["ll_drawn"][k]]) and np.isfinite(W["ll_drawn"][k])
        assert W["off_other"][k] == [x for x in copies if x != o][0]
        assert abs(W["sum_other"][k] - (c - 1)) < 1e-6
        assert W["pq"][k] == math.floor(-10 * math.log10((c - 1) / c) + 0.5)
    assert {1, 2} >= set(W["pq"][int(H.u_off[g]):int(H.u_off[g + 1])]) and (W["pq"][int(H.u_off[g]):int(H.u_off[g + 1])] == 1).any()


# ------------------------------------------------------------------------------------- CPU
def test_placement_abi_surface(tmp_path):
    """The call is declared with exactly its prototype, bound and exported; fig_read_placement is seven pointers, 56 bytes;
    fig_gap_results did not grow and the version did not move; the emulation library, which lacks the call, still loads -- and
    asking it for a placement is an error that names the call, in Python and through figfill (before anything is written)."""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert re.search(r"^int fig_batch_placement\(fig_ctx \*ctx, const fig_gap_results \*filled, const int32_t \*origin, fig_read_placement \*p\);", hdr, flags=re.M)
    assert "fig_batch_placement" in api.EXPORTS
    assert hasattr(C.CDLL(util.pbuild.LIB), "fig_batch_placement")
    assert re.search(r"#define FIG_ABI_VERSION 1\b", hdr)
    names = ["ll_drawn", "ll_other", "sum_other", "off_other", "n_valid", "pq", "state"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu %d %d %d %d", sizeof(fig_read_placement), sizeof(fig_gap_results), '
           'FIG_PLACE_OFF, FIG_PLACE_ON, FIG_PLACE_NONE, FIG_PLACE_MAX_PQ);' + "".join(f'printf(" %zu", offsetof(fig_read_placement, {f}));' for f in names) + 'printf("\\n");return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert out[0] == C.sizeof(api.FigReadPlacement) == 56
    assert out[1] == C.sizeof(api.FigGapResults) == 128
    assert out[2:6] == [api.PLACE_OFF, api.PLACE_ON, api.PLACE_NONE, api.PLACE_MAX_PQ] == [0, 1, 255, 60]
    assert out[6:] == [getattr(api.FigReadPlacement, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 48]
    emu = api.load_library(util.EMULIB)
    assert not hasattr(emu, "fig_batch_placement") and emu.fig_version() == 1
    eng = api.Engine(0, lib_path=util.EMULIB)
    try:
        eng.n_gaps = 0
        with pytest.raises(RuntimeError, match="fig_batch_placement"):
            eng.placement(api.FillResult(np.zeros(1, np.int32), np.zeros(1, np.int32), None, str_off=np.zeros(1, np.int64)))
        with pytest.raises(RuntimeError, match="fig_batch_placement"):
            eng.fill_resident(placement=True)
    finally:
        eng.close()
    host = api.load_host_library()
    for fn in ("fighost_placement_li", "fighost_placement_isz", "fighost_placement_valid", "fighost_placement_phred", "fighost_placement_gaps_on", "fighost_run_write_placement"):
        assert hasattr(host, fn), fn
    for env in ({"FIGFILL_PLACEMENT": "1"}, {"FIGFILL_QUALITY": "1", "FIGFILL_QUALITY_MINPQ": "3"}):
        root = util.extract_golden("partial_small", str(tmp_path / ("r" + str(len(env)))))
        r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, env)
        assert r.returncode != 0 and "fig_batch_placement" in r.stderr
        for fn in ("gapplacement.txt", "gapquality.txt", "gapout.txt"):
            assert not os.path.exists(os.path.join(root, "tmp", fn)), fn


_DRAW_HDR = re.compile(r"^ *=+\+Gap = (\d+) starting,length = (-?\d+)=+$")
_DRAW_READ = re.compile(r"^ *([A-Za-z]+)\[(\d+) (-?\d+) isz = (-?\d+) ([IEP])\]$")
ISZ_GOLDENS = ["unmapped_small", "unmapped_L31", "unmapped_L75", "unmapped_mid_err", "bench_b25", "bench_b160"]
ISZ_READS = []


@pytest.mark.parametrize("name", ISZ_GOLDENS)
def test_insert_size_closed_form_against_the_reference(name, tmp_path):
    """Every read line of the reference's draw.txt: read number k of the gap, its offset o, the insert size the reference's finalize
    computed (tempInsertSize) and the side letter.  isz(o) of the header, from the anchor, the gap start, G0 and the header length
    n, equals it read by read, through fighost_placement_isz and through the restatement's vector form; the side letter is I for
    pos < gap_start."""
    root = util.extract_golden(name, str(tmp_path))
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        ids = np.arange(max(n, 1), dtype=np.int64)
        cb = api.FigGapBatch(); su = C.c_int64(); sp = C.c_int64()
        assert host.fighost_run_shard(h, api._p(ids, api.c_i64_p), n, C.byref(cb), C.byref(su), C.byref(sp)) == 0
        u_off = np.ctypeslib.as_array(cb.u_read_off, shape=(n + 1,)).copy()
        pos = np.ctypeslib.as_array(cb.u_anchor_pos, shape=(int(su.value),)).copy()
        soff = np.ctypeslib.as_array(cb.u_seq_off, shape=(int(su.value) + 1,)).copy()
        start = np.ctypeslib.as_array(cb.gap_start, shape=(n,)).copy(); G = np.ctypeslib.as_array(cb.gap_len, shape=(n,)).copy()
    finally:
        host.fighost_run_close(h)
    count, g, hl = 0, None, None
    for ln in open(os.path.join(root, "ref", "draw.txt")):
        m = _DRAW_HDR.match(ln.rstrip("\n"))
        if m:
            g, hl = int(m.group(1)), int(m.group(2))
            continue
        m = _DRAW_READ.match(ln.rstrip("\n"))
        if not m:
            continue
        assert m.group(5) != "P"
        k = int(u_off[g]) + int(m.group(2)); o = int(m.group(3)); rl = int(soff[k + 1] - soff[k])
        assert rl == len(m.group(1)) and k < u_off[g + 1]
        want = int(m.group(4))
        assert int(host.fighost_placement_isz(int(pos[k]), int(start[g]), int(G[g]), hl, rl, o)) == want, (name, g, k)
        assert int(isz_of(int(pos[k]), int(start[g]), int(G[g]), hl, rl, o)) == want
        assert m.group(5) == ("I" if pos[k] < start[g] else "E")
        count += 1
    assert count > 0
    ISZ_READS.append(count)
    if len(ISZ_READS) == len(ISZ_GOLDENS):
        assert sum(ISZ_READS) == 1533


@pytest.mark.parametrize("ll_drawn,ll_other,sum_other,want", [
    (-7.0, -7.0, 3.0, 1),              # four equal placements: perr = 0.75, 1.25
    (-7.0, -7.0, 1.0, 3),              # two equal: perr = 0.5, 3.01
    (-7.0, NINF, 0.0, 60),             # nothing else: perr == 0
    (-2.0, -900.0, 0.0, 60),           # the others underflowed
    (NINF, -3.0, 1.0, 0),              # the drawn placement is impossible or not a placement
    (NINF, NINF, 0.0, 0),
    (-10.0, -7.0, 1.0, 0),             # another placement better by 3 decades: perr = 1 / 1.001
    (-7.0, -10.0, 0.001, 30),          # the drawn one better by 3 decades: 30.004
    (-7.0, -9.0, 0.03, 15),            # 0.03 / 1.03: 15.36
    (-7.0, -20.0, 1e-13, 60),          # 130 clamps to 60
])
def test_phred_by_hand(ll_drawn, ll_other, sum_other, want):
    """Cases far from a rounding boundary of floor(-10*log10(perr) + 0.5)."""
    assert list(phred_of(ll_drawn, ll_other, sum_other)) == [want]


def test_on_off_rule():
    """ON iff the model is unmapped-mode, the unmapped header is there and the partial one is not, and the quality's rule holds:
    the partial-evidence gap, ORIGINAL, a header != n and a partial-mode model are all off."""
    host = api.load_host_library()
    rows = [(n, hdr, org) for n in (0, -3, 1, 57) for hdr in [(-1, -1), (n, -1), (-1, n), (n + 1, -1), (n, n), (n, 0), (0, -1)] for org in [None] + list(range(8))]
    for given in (False, True):
        sel = [r for r in rows if (r[2] is not None) == given]
        fl = np.array([r[0] for r in sel], dtype=np.int32); dl = np.array([h for r in sel for h in r[1]], dtype=np.int32)
        org = np.array([r[2] or 0 for r in sel], dtype=np.int32)
        for unm in (1, 0):
            st = np.full(len(sel), 0xFF, dtype=np.uint8)
            host.fighost_placement_gaps_on(unm, len(sel), api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p) if given else None, api._p(st, api.c_u8_p))
            want = [1 if (unm and n > 0 and lu == n and lp < 0 and (o is None or (o & 1 and not o & 2))) else 0 for n, (lu, lp), o in sel]
            assert list(st) == want
            qs = np.full(len(sel), 0xFF, dtype=np.uint8)
            host.fighost_quality_gaps_on(len(sel), api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p) if given else None, api._p(qs, api.c_u8_p))
            assert (st <= qs).all()                            # never on where the quality is off
    one = lambda unm, n, lu, lp, o: int((lambda st: (host.fighost_placement_gaps_on(unm, 1, api._p(np.array([n], np.int32), api.c_i32_p), api._p(np.array([lu, lp], np.int32), api.c_i32_p),
                                                                                       api._p(np.array([o], np.int32), api.c_i32_p), api._p(st, api.c_u8_p)), st[0])[1])(np.zeros(1, np.uint8)))
    assert one(1, 57, 57, -1, F_) == one(1, 57, 57, -1, F_ | T_) == 1
    assert one(1, 57, -1, 57, F_) == one(1, 57, 57, -1, F_ | O_) == one(1, 57, 58, -1, F_) == one(0, 57, 57, -1, F_) == one(1, 57, 57, -1, 0) == 0


def test_placement_writer_format(tmp_path):
    """fighost_run_write_placement on hand-made arrays: `g contig start G0 n state R Q`, Q = R characters of Phred+33 or `~`."""
    root = util.extract_golden("unmapped_small", str(tmp_path))
    exp = _gapout(root)
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        ids = np.arange(max(n, 1), dtype=np.int64)
        cb = api.FigGapBatch(); su = C.c_int64(); sp = C.c_int64()
        assert host.fighost_run_shard(h, api._p(ids, api.c_i64_p), n, C.byref(cb), C.byref(su), C.byref(sp)) == 0
        u_off = np.ctypeslib.as_array(cb.u_read_off, shape=(n + 1,)).copy()
        nu = int(su.value)
        assert n == len(exp) and nu > 3
        fl = np.arange(3, 3 + n, dtype=np.int32)
        pq = (np.arange(nu) % 61).astype(np.uint8); pq[::3] = 255
        st = (np.arange(n) % 2).astype(np.uint8)
        err = C.create_string_buffer(512)
        cwd = os.getcwd(); os.chdir(root)
        try:
            rc = host.fighost_run_write_placement(h, api._p(fl, api.c_i32_p), api._p(pq, api.c_u8_p), api._p(st, api.c_u8_p), err, 512)
        finally:
            os.chdir(cwd)
    finally:
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    want = "".join("\t".join(exp[g][:4]) + f"\t{fl[g]}\t{st[g]}\t{u_off[g + 1] - u_off[g]}\t" + "".join("~" if q == 255 else chr(33 + q) for q in pq[u_off[g]:u_off[g + 1]]) + "\n"
                   for g in range(n))
    got = util.read(os.path.join(root, "tmp", "gapplacement.txt"))
    assert got == want and "~" in got and "!" in got and chr(33 + 60) in got
    assert not os.path.exists(os.path.join(root, "tmp", "gapquality.txt"))


def test_kernel_arithmetic_on_the_cpu(hand, tmp_path):
    """The functions fig_placement_kernel calls per (read, placement) pair, compiled as plain C++ into a program of its own with
    AddressSanitizer and UBSan (tests/placement_read_main.cpp; run directly), over the scored reads of the hand-made case:
    ll_drawn, ll_other, off_other and n_valid equal the numpy restatement bit for bit."""
    H, W = hand
    exe = str(tmp_path / "placement_read")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "placement_read_main.cpp")])
    m = H.model
    on = [g for g in range(len(GAPS)) if H.state[g]]
    lines = ["200", " ".join(float(v).hex() for v in m.e), " ".join(float(v).hex() for v in m.T), f"{len(m.insd)} {m.Tmin} {m.Tmax}",
             " ".join(float(v).hex() for v in m.insd), str(len(on))]
    for g in on:
        n, st = int(H.filled_len[g]), int(H.starts[g])
        left = [CODE[H.contig[st - k]] if st - k >= 0 else 4 for k in range(1, FLANK + 1)]
        right = [CODE[H.contig[st + G0 + k]] if st + G0 + k < len(H.contig) else 4 for k in range(FLANK)]
        ks = range(int(H.u_off[g]), int(H.u_off[g + 1]))
        lines += [f"{n} {st} {G0} {len(ks)}", "".join(str(int(c)) for c in left + right), H.raw[int(H.str_off[g]):int(H.str_off[g + 1])].tobytes().decode() or "-"]
        lines += [f"{int(H.draw_pos[k])} {len(H.seqs[k])} {int(H.rev[k])} {H.pos[k]} {H.seqs[k].tobytes().decode()}" for k in ks]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    sc = np.flatnonzero(H.scored())
    assert len(rows) == len(sc) > 200
    got_d = np.array([int(t[0], 16) for t in rows], dtype=np.uint64).view(np.float64)
    got_o = np.array([int(t[1], 16) for t in rows], dtype=np.uint64).view(np.float64)
    assert same_bits(got_d, W["ll_drawn"][sc]) and same_bits(got_o, W["ll_other"][sc])
    assert [int(t[2]) for t in rows] == list(W["off_other"][sc]) and [int(t[3]) for t in rows] == list(W["n_valid"][sc])


def test_edge_lengths_on_the_cpu(hand_edge, tmp_path):
    """The edge-length case through the same stand-alone program (tests/placement_read_main.cpp, AddressSanitizer and UBSan):
    ll_drawn, ll_other, off_other and n_valid equal the numpy restatement bit for bit."""
    H, W = hand_edge
    exe = str(tmp_path / "placement_read")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "placement_read_main.cpp")])
    m = H.model
    st = int(H.starts[0])
    left = [CODE[H.contig[st - k]] if st - k >= 0 else 4 for k in range(1, FLANK + 1)]
    right = [CODE[H.contig[st + G0 + k]] if st + G0 + k < len(H.contig) else 4 for k in range(FLANK)]
    lines = ["200", " ".join(float(v).hex() for v in m.e), " ".join(float(v).hex() for v in m.T), f"{len(m.insd)} {m.Tmin} {m.Tmax}",
             " ".join(float(v).hex() for v in m.insd), "1", f"40 {st} {G0} {H.NU}", "".join(str(int(c)) for c in left + right), H.raw.tobytes().decode()]
    lines += [f"{int(H.draw_pos[k])} {len(H.seqs[k])} {int(H.rev[k])} {H.pos[k]} {H.seqs[k].tobytes().decode()}" for k in range(H.NU)]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    sc = np.flatnonzero(H.scored())
    assert len(rows) == len(sc) > 40
    assert same_bits(np.array([int(t[0], 16) for t in rows], dtype=np.uint64).view(np.float64), W["ll_drawn"][sc])
    assert same_bits(np.array([int(t[1], 16) for t in rows], dtype=np.uint64).view(np.float64), W["ll_other"][sc])
    assert [int(t[2]) for t in rows] == list(W["off_other"][sc]) and [int(t[3]) for t in rows] == list(W["n_valid"][sc])


# ------------------------------------------------------------------------------------- GPU
def _placement_raw(eng, H, origin, nu=None):
    """fig_batch_placement through ctypes with the caller's buffers filled with 0xFF bytes before the call"""
    r = api.FigGapResults()
    r.filled_len = api._p(H.filled_len, api.c_i32_p); r.str_off = api._p(H.str_off, api.c_i64_p)
    r.str = C.cast(H.raw.ctypes.data, C.c_char_p); r.str_capacity = len(H.raw)
    r.draw_pos = api._p(H.draw_pos, api.c_i32_p); r.draw_isz = api._p(H.draw_isz, api.c_i32_p); r.draw_len = api._p(H.draw_len, api.c_i32_p)
    nu = H.NU if nu is None else nu
    m = max(nu, 1)
    d = [np.zeros(m) for _ in range(3)]
    for a in d:
        a.view(np.uint8)[...] = 0xFF
    off = np.full(m, -1, dtype=np.int32); nv = np.full(m, -1, dtype=np.int32); pq = np.full(m, 0xFF, dtype=np.uint8); pq[::2] = 0xFE
    st = np.full(len(H.gaps), 0xFF, dtype=np.uint8)
    rp = api.FigReadPlacement()
    rp.ll_drawn = api._p(d[0], api.c_double_p); rp.ll_other = api._p(d[1], api.c_double_p); rp.sum_other = api._p(d[2], api.c_double_p)
    rp.off_other = api._p(off, api.c_i32_p); rp.n_valid = api._p(nv, api.c_i32_p); rp.pq = api._p(pq, api.c_u8_p); rp.state = api._p(st, api.c_u8_p)
    rc = eng.lib.fig_batch_placement(eng.ctx, C.byref(r), api._p(origin, api.c_i32_p) if origin is not None else None, C.byref(rp))
    return rc, api.Placement(d[0][:nu], d[1][:nu], d[2][:nu], off[:nu], nv[:nu], pq[:nu], st)


@pytest.mark.gpu
def test_hand_made_batch(hand):
    """fig_batch_placement on the resident hand-made batch, no fill: read lengths 31 / 77 / 150 / 200, n = 1 / 65 / 257 / 600, 3 / 70
    / 130 reads, both anchor sides and orientations, -inf from e[17] = 0, T[C][G] = 0 and insd[500] = 0, thresholds cutting the
    window, reads without a valid placement, invalid drawn offsets, gaps at the contig ends, N everywhere, undrawn reads, one gap
    off by each rule, the tandem gap.  Exact outputs bit for bit, sum_other inside its bound, pq as defined; buffers came in as
    0xFF bytes; the Python face gives the same arrays; without origins the ORIGINAL gap is on too; freed batch: FIG_EINVAL."""
    H, W = hand
    sc = H.scored()
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        rc, P = _placement_raw(eng, H, H.origin)
        assert rc == 0 and list(P.state) == STATE
        far = compare(P, W, sc)
        assert far.sum() == sc.sum()
        g = [i for i in range(len(GAPS)) if GAPS[i][6] == "tandem"][0]
        ks = slice(int(H.u_off[g]), int(H.u_off[g + 1]))
        assert same_bits(P.ll_other[ks], P.ll_drawn[ks]) and np.array_equal(P.pq[ks], W["pq"][ks]) and np.array_equal(P.off_other[ks], W["off_other"][ks])
        P2 = eng.placement(H.result(), H.origin)
        for f in ("ll_drawn", "ll_other", "sum_other"):
            assert same_bits(getattr(P2, f), getattr(P, f)), f
        for f in ("off_other", "n_valid", "pq", "state"):
            assert np.array_equal(getattr(P2, f), getattr(P, f)), f
        rc, P3 = _placement_raw(eng, H, None)
        assert rc == 0 and list(P3.state) == [1, 1, 1, 1, 1, 0, 0, 1, 1]
        keep = np.ones(H.NU, dtype=bool); keep[int(H.u_off[4]):int(H.u_off[5])] = False
        assert same_bits(P3.ll_drawn[keep], P.ll_drawn[keep]) and np.array_equal(P3.pq[keep], P.pq[keep]) and (P3.pq[~keep] != 255).any()
        # |o*| = 2^20 is refused in a gap that is on and not looked at in a gap that is off
        for k, v, want_rc in ((int(H.u_off[2]) + 1, 1 << 20, -1), (int(H.u_off[2]) + 1, -(1 << 20), -1), (int(H.u_off[2]) + 1, (1 << 20) - 1, 0), (int(H.u_off[6]) + 1, 1 << 20, 0)):
            B = HandPlace()
            B.draw_pos[k] = v
            assert _placement_raw(eng, B, B.origin)[0] == want_rc, (k, v)
        eng.free_batch()
        assert _placement_raw(eng, H, H.origin)[0] == -1                # no resident batch
    finally:
        eng.close()
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_edge_lengths_on_the_device(hand_edge):
    """fig_batch_placement on the resident edge-length case (read lengths 1, 16, 17, 32, 33, 199; 65 reads; 40 columns): the exact
    outputs bit for bit the restatement's, sum_other inside its bound, pq as defined; buffers came in as 0xFF bytes."""
    H, W = hand_edge
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        rc, P = _placement_raw(eng, H, H.origin)
    finally:
        eng.close()
    assert rc == 0 and list(P.state) == [1]
    compare(P, W, H.scored())


@pytest.mark.gpu
def test_partial_mode_model_scores_nothing():
    """The same batch under a partial-mode model: every gap is off and every read comes back as unscored."""
    H = HandPlace(mode="partial")
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        rc, P = _placement_raw(eng, H, H.origin, nu=0)
        assert rc == 0 and not P.state.any()
        P2 = eng.placement(H.result(), H.origin)
        assert len(P2.pq) == 0 and not P2.state.any()
    finally:
        eng.close()


@pytest.mark.gpu
def test_quality_with_min_pq(hand):
    """Engine.quality(placement=P, min_pq=k) on the hand-made case: the plane equals test_base_quality.restate over the drawn reads
    whose pq is at least k, bit for bit, and differs from the unfiltered plane."""
    H, _ = hand
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        P = eng.placement(H.result(), H.origin)
        k = 3
        ll, ph, st = eng.quality(H.result(), H.origin, placement=P, min_pq=k)
        ll0, _, st0 = eng.quality(H.result(), H.origin)
    finally:
        eng.close()
    tabs = tbq.tables(H.model.cstruct())
    assert np.array_equal(st, st0) and list(st) == [1, 1, 1, 1, 0, 1, 0, 1, 1]          # (the quality scores the partial-evidence gap as well)
    dropped = 0
    for g in range(len(GAPS)):
        a, b = int(H.str_off[g]), int(H.str_off[g + 1])
        if GAPS[g][3] != "u" or not st[g]:
            assert same_bits(ll[a:b], ll0[a:b])
            continue
        ks = [x for x in range(int(H.u_off[g]), int(H.u_off[g + 1])) if H.draw_pos[x] != INT_MIN]
        kept = [x for x in ks if P.pq[x] == 255 or P.pq[x] >= k]
        dropped += len(ks) - len(kept)
        assert same_bits(ll[a:b], tbq.restate(int(H.filled_len[g]), [(int(H.draw_pos[x]), H.seqs[x], bool(H.rev[x])) for x in kept], tabs)), f"gap {g}"
    assert dropped > 10 and not same_bits(ll, ll0)
    assert np.array_equal(ph[np.repeat(st.astype(bool), H.filled_len)], tbq.phred_of(ll, H.raw)[np.repeat(st.astype(bool), H.filled_len)])


def run_golden_placement(root):
    """A golden filled as figfill fills it (draw and support planes), then Engine.placement with the returned origins while the
    batch is resident, then a second plain fill.  -> Fill with .P, .second and what the restatement needs"""
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
        F.contig = np.frombuffer(cb.contig_seq or b"", dtype=np.uint8)               # (ASCII bases: no NUL inside)
        F.u_off = np.ctypeslib.as_array(cb.u_read_off, shape=(n + 1,)).copy()
        F.u_seq_off = np.ctypeslib.as_array(cb.u_seq_off, shape=(nu + 1,)).copy()
        F.u_seq = np.frombuffer(cb.u_seq or b"", dtype=np.uint8)
        assert len(F.contig) == int(F.contig_off[nc]) and len(F.u_seq) == int(F.u_seq_off[nu])
        F.u_rev = np.ctypeslib.as_array(cb.u_is_reverse, shape=(nu,)).copy(); F.u_pos = np.ctypeslib.as_array(cb.u_anchor_pos, shape=(nu,)).copy()
        F.tabs = place_tables(cm); F.unmapped = bool(cm.unmapped_flag); F.nu = nu
        eng = api.Engine(0)
        try:
            eng.set_model_struct(cm)
            eng.upload_struct(cb)
            reach = np.zeros(max(n, 1), dtype=np.uint8); reach[:n] = eng.probe_reach()
            preset = np.zeros(max(n, 1), dtype=np.uint8)
            host.fighost_run_ot_presets(h, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
            eng.set_ot_preset(preset[:n])
            res = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, placement=True, keep_resident=True)
            F.second = _take(Fill(), eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.P = res.placement
        return F
    finally:
        host.fighost_run_close(h)


@pytest.fixture(scope="module")
def pfills(tmp_path_factory):
    """name -> golden filled with the draw and support planes and the placement; computed once per module, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden_placement(util.extract_golden(name, str(tmp_path_factory.mktemp(name))))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "bench_b160"])
def test_goldens_end_to_end(name, pfills):
    """A golden filled as figfill fills it, then the placement: states by the rule, every scored read against the restatement
    (exact outputs bit for bit, sum_other inside its bound, pq as defined), and the fill's own draw_isz equals isz(draw_pos) for
    every scored read."""
    F = pfills(name)
    assert F.unmapped and (np.diff(F.u_off) <= 3000).all()
    want = unscored(F.nu)
    sc = np.zeros(F.nu, dtype=bool)
    for g in range(F.n):
        n = int(F.filled_len[g]); org = int(F.origin[g])
        on = n > 0 and int(F.draw_len[2 * g]) == n and int(F.draw_len[2 * g + 1]) < 0 and bool(org & F_) and not org & O_
        assert int(F.P.state[g]) == int(on), f"gap {g}"
        if not on:
            continue
        c = int(F.gap_contig[g])
        S = columns(F.contig[int(F.contig_off[c]):int(F.contig_off[c + 1])], int(F.start[g]), int(F.G0[g]), F.raw[int(F.str_off[g]):int(F.str_off[g + 1])])
        for k in range(int(F.u_off[g]), int(F.u_off[g + 1])):
            if F.draw_pos[k] == INT_MIN:
                continue
            sc[k] = True
            seq = F.u_seq[int(F.u_seq_off[k]):int(F.u_seq_off[k + 1])]
            r = restate_read(S, n, seq, int(F.u_rev[k]), int(F.u_pos[k]), int(F.draw_pos[k]), int(F.start[g]), int(F.G0[g]), F.tabs)
            for f, v in r.items():
                want[f][k] = v
            assert int(F.draw_isz[k]) == int(isz_of(int(F.u_pos[k]), int(F.start[g]), int(F.G0[g]), n, len(seq), int(F.draw_pos[k]))), (g, k)
    compare(F.P, want, sc)
    assert sc.any() and (F.P.pq[sc] > 0).any()
    if name == "bench_b160":            # what tests/test_base_quality.py pins of this gap
        assert F.P.state[0] == 1 and int(sc[int(F.u_off[0]):int(F.u_off[1])].sum()) == 657


@pytest.mark.gpu
def test_off_means_off(pfills, tmp_path):
    """unmapped_small: lengths, strings, gaptofill, the draw planes and the support plane of a fill are identical with and without a
    following fig_batch_placement, and a second fill of the still resident batch after the call returns the same bytes."""
    from test_base_support import run_golden
    on = pfills("unmapped_small")
    off = run_golden(util.extract_golden("unmapped_small", str(tmp_path)), support=True)
    for other in (off, on.second):
        for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
            assert np.array_equal(getattr(on, f), getattr(other, f)), f


@pytest.mark.gpu
def test_gapplacement_file_is_the_same_from_every_host_path(pfills, tmp_path, monkeypatch):
    """unmapped_small with FIGFILL_PLACEMENT=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 and two-rank figfill_mp leave the
    same gapplacement.txt, which is the file of Engine.placement's pq; the reference's files stay byte-identical in every run;
    with neither variable set no new file appears.  FIGFILL_QUALITY_MINPQ with FIGFILL_QUALITY=1 changes gapquality.txt and writes
    no gapplacement.txt; without FIGFILL_QUALITY it does nothing."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    name = "unmapped_small"
    for v in ("FIGFILL_SUPPORT", "FIGFILL_QUALITY", "FIGFILL_PLACEMENT", "FIGFILL_QUALITY_MINPQ"):
        monkeypatch.delenv(v, raising=False)
    roots = [util.extract_golden(name, str(tmp_path / f"r{k}")) for k in range(7)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    new = ("gapplacement.txt", "gapquality.txt", "gapsupport.txt")
    r = util.run([util.FIGFILL] + argv, roots[3])
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[4], {"FIGFILL_QUALITY_MINPQ": "3"})
    assert r.returncode == 0, r.stderr
    for root in roots[3:5]:
        assert not any(os.path.exists(os.path.join(root, "tmp", fn)) for fn in new)
    r = util.run([util.FIGFILL] + argv, roots[0], {"FIGFILL_PLACEMENT": "1"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[1], {"FIGFILL_PLACEMENT": "1", "FIGFILL_DEVICES": "0,0"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[5], {"FIGFILL_QUALITY": "1"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[6], {"FIGFILL_QUALITY": "1", "FIGFILL_QUALITY_MINPQ": "61"})
    assert r.returncode == 0, r.stderr
    monkeypatch.setenv("FIGFILL_PLACEMENT", "1")                            # the spawned ranks inherit it
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
    files = [util.read(os.path.join(root, "tmp", "gapplacement.txt")) for root in roots[:3]]
    assert files[0] == files[1] == files[2]
    F = pfills(name)
    exp = _gapout(roots[0])
    lines = files[0].splitlines()
    assert len(lines) == len(exp) == F.n
    for g, (ln, e) in enumerate(zip(lines, exp)):
        f = ln.split("\t")
        assert len(f) == 8 and f[:5] == e[:5] and f[5] == str(int(F.P.state[g])) and int(f[6]) == F.u_off[g + 1] - F.u_off[g]
        assert f[7] == "".join("~" if v == 255 else chr(33 + v) for v in F.P.pq[int(F.u_off[g]):int(F.u_off[g + 1])])
    assert any(ln.split("\t")[5] == "1" for ln in lines)
    # every read is below pq 61: the filtered quality has no evidence left in the unmapped gaps that are on, which leaves the
    # uniform prior -- perr = 3/4, Phred 1 (`"`) under a called base, 0 (`!`) under an N
    q0, q1 = (util.read(os.path.join(root, "tmp", "gapquality.txt")) for root in roots[5:7])
    assert q0 != q1 and len(q0.splitlines()) == len(q1.splitlines()) == F.n
    for g, (a, b) in enumerate(zip(q0.splitlines(), q1.splitlines())):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:6] == fb[:6]
        if F.P.state[g]:
            assert set(fb[6]) <= {"!", '"'} and all((c == "!") == (s == "N") for c, s in zip(fb[6], exp[g][5] if len(exp[g]) > 5 else ""))
        else:
            assert fa[6] == fb[6]
    for k, root in enumerate(roots):
        assert os.path.exists(os.path.join(root, "tmp", "gapplacement.txt")) == (k < 3)
        assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
