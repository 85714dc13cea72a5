"""Indel evidence per filled base (fig_batch_indel, include/figbird_hip.h: fig_gap_indel).

The restatement below is numpy over the reads of a gap at once: per row of the band one elementwise addition per term in the defined
order (never a sum routine), the deletion sweep sequentially in ascending d, the traceback as a list of steps that is normalised
afterwards.  Every output of the device is compared with it with no tolerance, doubles on their int64 view: the device only adds
table entries and compares.
"""
import ctypes as C
import math
import os
import socket
import subprocess

import numpy as np
import pytest

import util
from figbird_amd import api
import test_base_quality as tbq
import test_read_placement as trp
from test_base_support import CODE, INT_MIN, Fill, _gapout, _open_run, _take

NINF = -math.inf
LQ = float.fromhex("-0x1.34413509f79ffp-1")
W = 7
ND = 15
FLANK = 208
F_, O_, T_ = api.SUP_FINAL, api.SUP_ORIGINAL, api.SUP_TIEBREAK
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
END_ORDER = [0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5, -6, 6, -7, 7]
PAD = 210                                                      # columns kept either side of a string: element PAD + x is column x


# ------------------------------------------------------------------------------------- the restatement
def indel_tables(cm):
    """fig_model struct -> (lm, le, lt [4, 4], lI, lD)"""
    host = api.load_host_library()
    lm, le, lt = tbq.tables(cm)
    L = int(cm.max_read_length)
    lI = np.zeros(L); lD = np.zeros(L)
    assert host.fighost_indel_tables(C.byref(cm), api._p(lI, api.c_double_p), api._p(lD, api.c_double_p)) == 0
    return lm, le, lt, lI, lD


def columns(contig, gap_start, G0, string):
    """codes of the columns -PAD .. n + PAD - 1 of a gap: N outside the contig and beyond the 208 flank columns either side"""
    n = len(string)
    x = np.arange(-PAD, n + PAD, dtype=np.int64)
    p = np.where(x < 0, gap_start + x, gap_start + G0 + (x - n))
    inside = (p >= 0) & (p < len(contig)) & (x >= -FLANK) & (x - n < FLANK)
    S = np.where(inside, CODE[contig[np.clip(p, 0, len(contig) - 1)]], 4)
    S[PAD:PAD + n] = CODE[string]
    return S


def band(S, reads, tabs):
    """The band of every read of one gap.  reads: [(seq uint8, rev, ostar)], all aligned.  -> H [R, 15] of the last row, the
    back-pointers BP [R, maxlen + 1, 15] (0 DIAG, 1 INS, 2 DEL) and ll_flat [R]"""
    lm, le, lt, lI, lD = tabs
    R = len(reads)
    lens = np.array([len(r[0]) for r in reads], dtype=np.int64)
    ml = int(lens.max())
    s = np.full((R, ml), 4, dtype=np.int64)
    for a, r in enumerate(reads):
        s[a, :lens[a]] = CODE[r[0]]
    rev = np.array([r[1] for r in reads], dtype=bool)
    o = np.array([r[2] for r in reads], dtype=np.int64)
    d = np.arange(-W, W + 1, dtype=np.int64)
    H = np.zeros((R, ND)); flat = np.zeros(R)
    BP = np.zeros((R, ml + 1, ND), dtype=np.int8)
    with np.errstate(invalid="raise"):
        for i in range(1, ml + 1):
            j = i - 1
            act = lens >= i
            k = np.clip(np.where(rev, lens - 1 - j, j), 0, len(lm) - 1)
            sj = s[:, j]
            ok = sj < 4
            c = S[PAD + o[:, None] + j + d[None, :]]
            sc = np.where(ok, sj, 0)
            t = np.where(c > 3, LQ, np.where(c == sc[:, None], lm[k][:, None], le[k][:, None] + lt[c & 3, sc[:, None]]))
            diag = np.where(ok[:, None], H + t, H)
            ins = np.full((R, ND), NINF)
            ins[:, :ND - 1] = H[:, 1:] + lI[k][:, None]
            Hn = np.where(diag >= ins, diag, ins)
            bp = np.where(diag >= ins, 0, 1).astype(np.int8)
            # the sweep changes nothing unless some single step from the values as they stand would: only those reads are swept
            first = Hn[:, :-1] + lD[k][:, None] > Hn[:, 1:]
            for a in np.flatnonzero(act & (lens > i) & first.any(axis=1)):
                for q in range(1, ND):
                    v = Hn[a, q - 1] + lD[k[a]]
                    if v > Hn[a, q]:
                        Hn[a, q] = v; bp[a, q] = 2
            flat = np.where(act & ok, flat + t[:, W], flat)
            H = np.where(act[:, None], Hn, H)
            BP[:, i, :] = bp
    assert not np.isnan(H).any()
    return H, BP, flat


def path_of(BP, S, code, ln, ostar, d_end):
    """traceback and left-normalised events of one read -> (d_start, n_ins, n_del, ins columns (set), del columns (set), events in
    path order from the end as the stand-alone program prints them)"""
    steps = []                                                  # (kind, i, d) of the cell a step ends in, last step first
    i, d = ln, d_end
    while i > 0:
        p = int(BP[i, d + W])
        steps.append((p, i, d))
        if p == 0:
            i -= 1
        elif p == 1:
            i -= 1; d += 1
        else:
            d -= 1
        assert -W <= d <= W
    d_start = d
    n_ins = n_del = 0
    ins_cols, del_cols, text = set(), set(), []
    a = 0
    while a < len(steps):
        kind = steps[a][0]
        if kind == 0:
            a += 1
            continue
        b = a
        while b < len(steps) and steps[b][0] == kind:
            b += 1
        m = b - a
        p = b
        if kind == 1:
            n_ins += m
            i0 = steps[b - 1][1] - 1
            x = ostar + steps[a][1] + steps[a][2]
            while p < len(steps) and steps[p][0] == 0 and code[i0 - 1] == code[i0 + m - 1]:
                i0 -= 1; x -= 1; p += 1
            if x not in ins_cols:
                text.append(f"I{x}")
            ins_cols.add(x)
        else:
            n_del += m
            x = ostar + steps[b - 1][1] + steps[b - 1][2] - 1
            while p < len(steps) and steps[p][0] == 0 and S[PAD + x - 1] == S[PAD + x + m - 1]:
                x -= 1; p += 1
            assert not del_cols & set(range(x, x + m))
            del_cols |= set(range(x, x + m))
            text.append(f"D{x}+{m}")
        a = b
    return d_start, n_ins, n_del, ins_cols, del_cols, ",".join(text) or "-"


def restate_gap(S, n, reads, tabs):
    """reads: [(seq, rev, ostar)] of the aligned reads of a gap -> per-read dicts and the planes del_reads, ins_reads, cover [n], ins_end"""
    dl = np.zeros(n, dtype=np.int32); il = np.zeros(n, dtype=np.int32); cv = np.zeros(n, dtype=np.int32)
    ie = 0
    out = []
    if not reads:
        return out, dl, il, cv, ie
    H, BP, flat = band(S, reads, tabs)
    for a, (seq, rev, ostar) in enumerate(reads):
        ln = len(seq)
        best, d_end = NINF, 0
        for dd in END_ORDER:
            if H[a, dd + W] > best:
                best, d_end = float(H[a, dd + W]), dd
        r = dict(ll_flat=float(flat[a]), ll_gapped=best, n_ins=0, n_del=0, d_end=0, d_start=0, events="-")
        if best > NINF:
            code = CODE[seq]
            d_start, n_ins, n_del, ic, dc, text = path_of(BP[a], S, code, ln, ostar, d_end)
            r.update(n_ins=n_ins, n_del=n_del, d_end=d_end, d_start=d_start, events=text)
            for x in dc:
                if 0 <= x < n:
                    dl[x] += 1
            for x in ic:
                if 0 <= x < n:
                    il[x] += 1
                elif x == n:
                    ie += 1
            lo, hi = max(ostar + d_start, 0), min(ostar + ln - 1 + d_end, n - 1)
            if lo <= hi:
                cv[lo:hi + 1] += 1
        assert r["ll_gapped"] >= r["ll_flat"]
        out.append(r)
    return out, dl, il, cv, ie


def call_of(dl, il, cv):
    return "".join("D" if (a >= 2 and 2 * a > c) else "I" if (b >= 2 and 2 * b > c) else "." for a, b, c in zip(dl, il, cv))


def is_aligned(o, ln, n):
    return o != INT_MIN and -(ln - 1) <= o <= n - 1


def expected(H, tabs=None, state=None):
    """The restatement of a whole hand-made case (a trp.HandPlace or a Case below) -> dict of the arrays of fig_gap_indel, plus
    `aligned` [NU] and `events` (per read, the text of the stand-alone program)"""
    tabs = tabs or indel_tables(H.model.cstruct())
    state = H.state if state is None else state
    NU, total, ng = H.NU, int(H.str_off[-1]), len(H.filled_len)
    w = dict(ll_flat=np.zeros(NU), ll_gapped=np.zeros(NU), n_ins=np.zeros(NU, np.int32), n_del=np.zeros(NU, np.int32), d_end=np.zeros(NU, np.int32),
             d_start=np.full(NU, INT_MIN, np.int32), del_reads=np.zeros(total, np.int32), ins_reads=np.zeros(total, np.int32), cover=np.zeros(total, np.int32),
             ins_end=np.zeros(ng, np.int32), call=np.full(total, ord("."), np.uint8), call_end=np.full(ng, ord("."), np.uint8),
             state=np.asarray(state, dtype=np.uint8), aligned=np.zeros(NU, bool), events=["-"] * NU)
    for g in range(ng):
        if not state[g]:
            continue
        n = int(H.filled_len[g])
        ks = [k for k in range(int(H.u_off[g]), int(H.u_off[g + 1])) if is_aligned(int(H.draw_pos[k]), len(H.seqs[k]), n)]
        a, b = int(H.str_off[g]), int(H.str_off[g]) + n
        S = columns(H.contig, int(H.starts[g]), trp.G0, H.raw[a:b])
        rs, dl, il, cv, ie = restate_gap(S, n, [(H.seqs[k], int(H.rev[k]), int(H.draw_pos[k])) for k in ks], tabs)
        for k, r in zip(ks, rs):
            w["aligned"][k] = True
            for f in ("ll_flat", "ll_gapped", "n_ins", "n_del", "d_end", "d_start"):
                w[f][k] = r[f]
            w["events"][k] = r["events"]
        w["del_reads"][a:b] = dl; w["ins_reads"][a:b] = il; w["cover"][a:b] = cv; w["ins_end"][g] = ie
        w["call"][a:b] = np.frombuffer(call_of(dl, il, cv).encode(), dtype=np.uint8)
        w["call_end"][g] = ord("I") if (ie >= 2 and 2 * ie > cv[n - 1]) else ord(".")
    return w


FIELDS_D = ("ll_flat", "ll_gapped")
FIELDS_I = ("n_ins", "n_del", "d_end", "d_start", "del_reads", "ins_reads", "cover", "ins_end", "call", "call_end", "state")


def compare(I, want):
    """every array of the device against the restatement's: doubles on their int64 view, everything else equal"""
    for f in FIELDS_D:
        bad = np.flatnonzero(np.asarray(getattr(I, f)).view(np.int64) != np.asarray(want[f]).view(np.int64))
        assert not len(bad), f"{f}: reads {bad[:8]}: got {getattr(I, f)[bad[:4]]}, want {want[f][bad[:4]]}"
    for f in FIELDS_I:
        got = np.asarray(getattr(I, f))
        assert got.shape == want[f].shape, f
        bad = np.flatnonzero(got != want[f])
        assert not len(bad), f"{f}: elements {bad[:8]}: got {got[bad[:4]]}, want {want[f][bad[:4]]}"


# ------------------------------------------------------------------------------------- hand-made cases
def clean_model(ins=1e-4, dele=1e-4):
    """0.5 % substitutions spread evenly, the given indel rates, no zero anywhere; the insert-size table of trp.place_model"""
    m = trp.place_model("unmapped")
    L = len(m.e)
    m.e = np.full(L, 0.005) + 1e-6 * np.arange(L)
    T = np.zeros(25)
    for b in range(5):
        for s in range(5):
            T[b * 5 + s] = 0.0 if b == s else 1.0 / 3
    m.T = T
    m.ins = np.full(L, ins); m.dele = np.full(L, dele)
    return m


class Case:
    """A resident batch and a `filled` made by hand, no fill, with the attribute names of trp.HandPlace.  gaps: per gap a dict with
    `string` (uint8) and `reads` [(seq uint8, rev, draw)]; optional `left` / `right`: the flank bases put into the contig beside the
    gap; `origin`, `hdr` (the unmapped draw header; default n).  Gap 0 lies 120 bases from the contig start and the last gap ends 100
    bases before the contig end."""

    def __init__(self, gaps, model, seed=1):
        rng = np.random.default_rng(seed)
        self.model = model
        ng = len(gaps)
        self.G0 = np.full(ng, trp.G0, dtype=np.int32)
        starts, p = [], 120
        for g in range(ng):
            starts.append(p); p += trp.G0 + 440
        clen = starts[-1] + trp.G0 + 100
        contig = rng.choice(ACGT, size=clen).copy()
        for g, gp in enumerate(gaps):
            st = starts[g]
            if "left" in gp:
                lf = gp["left"][-min(len(gp["left"]), st):]
                contig[st - len(lf):st] = lf
            if "right" in gp:
                rt = gp["right"][:clen - st - trp.G0]
                contig[st + trp.G0:st + trp.G0 + len(rt)] = rt
            contig[st:st + trp.G0] = ord("N")
        self.contig, self.starts = contig, np.array(starts, dtype=np.int64)
        self.filled_len = np.array([len(gp["string"]) for gp in gaps], dtype=np.int32)
        self.str_off = np.concatenate([[0], np.cumsum(self.filled_len)]).astype(np.int64)
        self.raw = np.concatenate([gp["string"] for gp in gaps] + [np.zeros(0, np.uint8)]).astype(np.uint8)
        if not len(self.raw):
            self.raw = np.zeros(1, np.uint8)
        self.seqs = [np.asarray(r[0], dtype=np.uint8) for gp in gaps for r in gp["reads"]]
        self.rev = np.array([r[1] for gp in gaps for r in gp["reads"]] or [0], dtype=np.uint8)[:len(self.seqs)] if self.seqs else np.zeros(0, np.uint8)
        draw = [r[2] for gp in gaps for r in gp["reads"]]
        self.u_off = np.concatenate([[0], np.cumsum([len(gp["reads"]) for gp in gaps])]).astype(np.int64)
        self.NU = int(self.u_off[-1])
        i32 = lambda v: np.asarray(v if len(v) else [0], dtype=np.int32)
        soff = np.concatenate([[0], np.cumsum([len(s) for s in self.seqs])]).astype(np.int64)
        pos = [int(self.starts[g]) - 300 for g, gp in enumerate(gaps) for _ in gp["reads"]]
        self.batch = api.GapBatch(
            contig_off=np.array([0, clen], dtype=np.int64), contig_seq=contig,
            gap_contig=np.zeros(ng, dtype=np.int32), gap_start=self.starts, gap_len=self.G0.copy(),
            gap_stat2=np.zeros(3 * ng, dtype=np.int32), gap_fillflag=np.ones(ng, dtype=np.int32),
            u_read_off=self.u_off, u_anchor_pos=i32(pos), u_is_reverse=self.rev if self.NU else np.zeros(1, np.uint8), u_seq_off=soff,
            u_seq=np.concatenate(self.seqs) if self.seqs else np.zeros(1, np.uint8),
            p_read_off=np.zeros(ng + 1, dtype=np.int64), p_clipped_index=i32([]), p_match=i32([]), p_pos=i32([]), p_ref_pos=i32([]),
            p_seq_off=np.zeros(1, dtype=np.int64), p_seq=np.zeros(1, np.uint8), p_qual=np.zeros(1, np.uint8))
        self.draw_pos = i32(draw)
        self.draw_isz = np.zeros(len(self.draw_pos), dtype=np.int32)
        self.draw_len = np.full(2 * ng, -1, dtype=np.int32)
        for g, gp in enumerate(gaps):
            self.draw_len[2 * g] = gp.get("hdr", len(gp["string"]))
        self.origin = np.array([gp.get("origin", F_) for gp in gaps], dtype=np.int32)
        self.state = np.array([1 if (len(gp["string"]) > 0 and gp.get("hdr", len(gp["string"])) == len(gp["string"]) and gp.get("origin", F_) & F_ and not gp.get("origin", F_) & O_) else 0
                               for gp in gaps], dtype=np.uint8)

    def result(self):
        return api.FillResult(self.filled_len, np.zeros_like(self.filled_len), None, str_off=self.str_off, raw=self.raw,
                              draw=(self.draw_pos, self.draw_isz, self.draw_len))


def mutate(rng, s, rate):
    s = s.copy()
    for j in np.flatnonzero(rng.random(len(s)) < rate):
        s[j] = ACGT[(int(CODE[s[j]]) + 1 + int(rng.integers(0, 3))) % 4]
    return s


def best_flat_offset(seq, full, t0, lo):
    """the offset among t0 - 2 .. t0 + 2 with the fewest mismatches of seq against `full` (whose element x - lo is column x); first minimum"""
    best = None
    for o in range(t0 - 2, t0 + 3):
        a = o - lo
        if a < 0 or a + len(seq) > len(full):
            continue
        mm = int((full[a:a + len(seq)] != seq).sum())
        if best is None or mm < best[0]:
            best = (mm, o)
    return best[1]


HOMO_AT, UNIQUE_AT = 45, 52


def planted_case():
    """One truth sequence of 101 columns with a 5-base homopolymer at 45 .. 49, between random flanks; 40 reads of 60 .. 77 bases copied
    from it with 0.5 % substitutions.  Three gaps with the same reads' material: the unedited string; the string with one base of the
    homopolymer removed (the reads show an insertion); the string with one base inserted before truth column 52 (the reads show a
    deletion).  Each read is drawn at its best ungapped offset against the gap's own emitted sequence."""
    rng = np.random.default_rng(20261021)
    left = rng.choice(ACGT, size=300); right = rng.choice(ACGT, size=300)
    truth = rng.choice(ACGT, size=101)
    truth[HOMO_AT - 1] = ord("C"); truth[HOMO_AT:HOMO_AT + 5] = ord("A"); truth[HOMO_AT + 5] = ord("G")
    truth[UNIQUE_AT - 1:UNIQUE_AT + 1] = np.frombuffer(b"CT", dtype=np.uint8)
    full_t = np.concatenate([left, truth, right])
    strings = [truth.copy(), np.delete(truth, HOMO_AT), np.insert(truth, UNIQUE_AT, ord("G"))]
    picks = [(int(rng.integers(60, 78)), int(rng.integers(-30, 75)), int(rng.integers(0, 2))) for _ in range(40)]
    seqs = [mutate(rng, full_t[300 + t:300 + t + ln], 0.005) for ln, t, _ in picks]
    gaps = []
    for s in strings:
        full = np.concatenate([left, s, right])
        reads = []
        for (ln, t, rev), q in zip(picks, seqs):
            reads.append((q, rev, best_flat_offset(q, full, t, -300)))
        gaps.append(dict(string=s, reads=reads, left=left, right=right))
    return Case(gaps, clean_model())


@pytest.fixture(scope="module")
def planted():
    H = planted_case()
    return H, expected(H)


EDGE_COUNTS = (1, 15, 16, 17, 63, 64, 65)
EDGE_LENS = tuple(tbq.EDGE_LENS) + (31, 200)


def edge_reads(rng, S, n, count):
    """reads copied from the gap's own columns at a random true offset, a few substitutions, one in three with a base removed or added;
    drawn at the true offset, at either end of the placement range, outside it, or not at all; N bases, the first and the last included"""
    out = []
    for r in range(count):
        ln = EDGE_LENS[r % len(EDGE_LENS)]
        t = int(rng.integers(-(ln - 1), n))
        src = np.frombuffer(b"ACGTN", dtype=np.uint8)[S[PAD + t + np.arange(ln + 3)]].copy()
        src[src == ord("N")] = rng.choice(ACGT, size=int((src == ord("N")).sum()))
        if ln > 8 and r % 3 == 1:
            cut = int(rng.integers(3, ln - 3)); src = np.delete(src, cut)
        elif ln > 8 and r % 3 == 2:
            cut = int(rng.integers(3, ln - 3)); src = np.insert(src, cut, rng.choice(ACGT))
        s = mutate(rng, src[:ln], 0.02)
        if r % 4 == 3:
            s[0] = ord("N")
        if r % 6 == 5:
            s[-1] = ord("N")
        if r % 10 == 9 and ln > 20:
            s[rng.choice(ln, size=2, replace=False)] = ord("N")
        o = t
        if r % 7 == 6:
            o = INT_MIN
        elif r % 11 == 10:
            o = n + 2
        elif r % 13 == 12:
            o = -ln
        elif r % 5 == 0:
            o = -(ln - 1)
        elif r % 5 == 1:
            o = n - 1
        out.append((s, r % 2, o))
    return out


def edge_case(model=None, seed=20261022):
    """Gaps with 1, 15, 16, 17, 63, 64 and 65 reads (the row-group and chunk edges) of the lengths 1, 16, 17, 32, 33, 199, 31 and 200
    mixed within a chunk, both orientations; strings with N columns; n = 1 and n = 300; a gap that is on with no drawn read; the gaps at
    either contig end (reads hang over the string into the flanks and past the contig end; the band of an aligned read reaches 206
    columns beyond the string at most, which is inside the 208 flank codes); and the read that only an insertion
    saves: 40 A's with a C at base 17 (e[17] = 0: every diagonal is -inf) on a string of A's."""
    rng = np.random.default_rng(seed)
    ns = [40, 57, 1, 300, 33, 64, 90]
    pre = []
    for n, count in zip(ns, EDGE_COUNTS):
        string = rng.choice(np.frombuffer(b"ACGTACGTACGTACGTACGTN", dtype=np.uint8), size=n).copy()
        pre.append(dict(string=string, reads=[], count=count))
    pre.append(dict(string=rng.choice(ACGT, size=20).copy(), reads=[], count=5, undrawn=True))
    allA = np.full(60, ord("A"), dtype=np.uint8)
    rd = np.full(40, ord("A"), dtype=np.uint8); rd[17] = ord("C")
    pre.append(dict(string=allA, reads=[(rd, 0, 5), (rd.copy(), 0, 6)], count=0, left=np.full(300, ord("A"), np.uint8), right=np.full(300, ord("A"), np.uint8)))
    pre.append(dict(string=rng.choice(ACGT, size=70).copy(), reads=[], count=20))
    shell = Case(pre, model or trp.place_model("unmapped"), seed=seed)          # the contig the reads are copied from
    for g, gp in enumerate(pre):
        if gp["count"]:
            n = len(gp["string"])
            S = columns(shell.contig, int(shell.starts[g]), trp.G0, gp["string"])
            gp["reads"] = edge_reads(rng, S, n, gp["count"])
            if gp.get("undrawn"):
                gp["reads"] = [(s, rv, INT_MIN) for s, rv, _ in gp["reads"]]
    return Case(pre, model or trp.place_model("unmapped"), seed=seed)


@pytest.fixture(scope="module")
def edges():
    H = edge_case()
    return H, expected(H)


def band_model():
    """The first 40 read bases are nearly always right (they pin the path's start to the drawn diagonal: the start is free) and half
    of all later ones are wrong (a chance match is worth little); deletions only after read base 39 and insertions only of the read
    bases 40 .. 47: what the band cannot reach is then not made up elsewhere from chance matches of random sequence"""
    m = clean_model()
    L = len(m.e)
    m.e = np.full(L, 0.5); m.e[:40] = 0.001
    m.ins = np.zeros(L); m.ins[40:48] = 1e-4
    m.dele = np.zeros(L); m.dele[39] = 1e-4
    return m


def band_case():
    """One gap of 230 unique columns and four forward reads drawn at 20 whose first 40 bases lie on the drawn diagonal and whose last
    150 follow an edit: 7 columns missing from the read, 8 missing, 7 bases too many in the read, 8 too many"""
    rng = np.random.default_rng(20261023)
    s = rng.choice(ACGT, size=230).copy()
    extra = rng.choice(ACGT, size=8)
    reads = [(np.concatenate([s[20:60], s[67:217]]), 0, 20), (np.concatenate([s[20:60], s[68:218]]), 0, 20),
             (np.concatenate([s[20:60], extra[:7], s[60:210]]), 0, 20), (np.concatenate([s[20:60], extra, s[60:210]]), 0, 20)]
    return Case([dict(string=s, reads=reads)], band_model())


# ------------------------------------------------------------------------------------- CPU
def test_tables_by_hand():
    """lI[k] = log10(ins[k]) + log10(1/4) in one addition, lD[k] = log10(del[k]); a zero rate gives -inf"""
    m = tbq.hand_model("unmapped")
    m.ins = 1e-4 * (1 + np.arange(200)); m.dele = 1e-5 * (3 + np.arange(200))
    m.ins[5] = 0.0; m.dele[9] = 0.0
    lm, le, lt, lI, lD = indel_tables(m.cstruct())
    assert lI[5] == NINF and lD[9] == NINF and np.isfinite(np.delete(lI, 5)).all() and np.isfinite(np.delete(lD, 9)).all()
    for k in (0, 1, 7, 199):
        assert lI[k] == math.log10(m.ins[k]) + LQ and lD[k] == math.log10(m.dele[k])
    assert lI[0] == -4.0 + LQ and LQ == math.log10(0.25)
    host = api.load_host_library()
    assert host.fighost_indel_tables(None, None, None) != 0


def test_rules_by_hand():
    """on = the placement's rule; aligned iff -(len-1) <= o <= n-1 and drawn; the end's tie order; the call: at least two reads and
    more than half of the cover, D before I"""
    host = api.load_host_library()
    rows = [(n, hdr, org) for n in (0, -3, 1, 57) for hdr in [(-1, -1), (n, -1), (-1, n), (n + 1, -1), (n, n)] for org in [None] + list(range(8))]
    for given in (False, True):
        sel = [r for r in rows if (r[2] is not None) == given]
        fl = np.array([r[0] for r in sel], dtype=np.int32); dl = np.array([h for r in sel for h in r[1]], dtype=np.int32)
        org = np.array([r[2] or 0 for r in sel], dtype=np.int32)
        for unm in (1, 0):
            st = np.full(len(sel), 0xFF, dtype=np.uint8); ps = np.full(len(sel), 0xFF, dtype=np.uint8)
            args = (unm, len(sel), api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p) if given else None)
            host.fighost_indel_gaps_on(*args, api._p(st, api.c_u8_p)); host.fighost_placement_gaps_on(*args, api._p(ps, api.c_u8_p))
            want = [1 if (unm and n > 0 and lu == n and lp < 0 and (o is None or (o & 1 and not o & 2))) else 0 for n, (lu, lp), o in sel]
            assert list(st) == want == list(ps)
    al = lambda o, ln, n: host.fighost_indel_aligned(o, ln, n)
    assert al(0, 1, 1) == 1 and al(-59, 60, 100) == 1 and al(-60, 60, 100) == 0 and al(99, 60, 100) == 1 and al(100, 60, 100) == 0
    assert al(INT_MIN, 60, 100) == 0 and al(1, 1, 1) == 0 and al(-1, 1, 1) == 0 and al(-199, 200, 1) == 1
    assert [host.fighost_indel_end_order(t) for t in range(15)] == END_ORDER
    cases = [(0, 0, 0, "."), (1, 0, 1, "."), (2, 0, 3, "D"), (2, 0, 4, "."), (2, 2, 3, "D"), (1, 2, 3, "I"), (0, 9, 18, "."), (0, 10, 19, "I"), (3, 0, 0, "D"), (0, 2, 2, "I")]
    a, b, c = (np.array([r[i] for r in cases], dtype=np.int32) for i in range(3))
    out = np.full(len(cases), 0xFF, dtype=np.uint8)
    host.fighost_indel_call(len(cases), api._p(a, api.c_i32_p), api._p(b, api.c_i32_p), api._p(c, api.c_i32_p), api._p(out, api.c_u8_p))
    assert out.tobytes().decode() == "".join(r[3] for r in cases) == call_of(a, b, c)
    assert [chr(host.fighost_indel_call_end(e, c)) for e, c in ((0, 0), (1, 1), (2, 3), (2, 4), (5, 2))] == [".", ".", "I", ".", "I"]


def test_indel_writer_format(tmp_path):
    """fighost_run_write_indel on hand-made arrays: `g contig start G0 n state C E`, C = the n characters of call, E = call_end"""
    root = util.extract_golden("unmapped_small", str(tmp_path))
    exp = _gapout(root)
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        fl = np.arange(3, 3 + n, dtype=np.int32); fl[0] = 0
        so = np.concatenate([[0], np.cumsum(fl)]).astype(np.int64)
        call = np.frombuffer(b".DI", dtype=np.uint8)[np.arange(int(so[-1])) % 3].copy()
        ce = np.frombuffer(b".I", dtype=np.uint8)[np.arange(n) % 2].copy()
        st = (np.arange(n) % 2).astype(np.uint8)
        err = C.create_string_buffer(512)
        cwd = os.getcwd(); os.chdir(root)
        try:
            rc = host.fighost_run_write_indel(h, api._p(fl, api.c_i32_p), api._p(so, api.c_i64_p), C.cast(call.ctypes.data, C.c_char_p), C.cast(ce.ctypes.data, C.c_char_p),
                                              api._p(st, api.c_u8_p), err, 512)
        finally:
            os.chdir(cwd)
    finally:
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    want = "".join("\t".join(exp[g][:4]) + f"\t{fl[g]}\t{st[g]}\t" + call[int(so[g]):int(so[g + 1])].tobytes().decode() + f"\t{chr(ce[g])}\n" for g in range(n))
    got = util.read(os.path.join(root, "tmp", "gapindel.txt"))
    assert n >= 2 and got == want and "D" in got and "I\n" in got
    assert not os.path.exists(os.path.join(root, "tmp", "gapplacement.txt"))


def test_planted_case_is_not_vacuous(planted):
    """The restatement alone, on the planted case: the unedited string has no call and no read with an event; the string with one base
    of the homopolymer removed has exactly one call, 'I' on the run's first column; the string with a base inserted has exactly one
    call, 'D' on that column; reads span the edits and most of them show it."""
    H, Wt = planted
    calls = [Wt["call"][int(H.str_off[g]):int(H.str_off[g + 1])].tobytes().decode() for g in range(3)]
    ev = [[Wt["n_ins"][k] + Wt["n_del"][k] for k in range(int(H.u_off[g]), int(H.u_off[g + 1]))] for g in range(3)]
    print([sum(1 for v in e if v) for e in ev], [Wt["cover"][int(H.str_off[g]) + HOMO_AT] for g in range(3)])
    assert Wt["aligned"].all() and list(Wt["state"]) == [1, 1, 1] and Wt["call_end"].tobytes() == b"..."
    assert calls[0] == "." * 101 and not any(ev[0])
    assert calls[1] == "." * HOMO_AT + "I" + "." * (100 - HOMO_AT - 1)
    assert calls[2] == "." * UNIQUE_AT + "D" + "." * (102 - UNIQUE_AT - 1)
    a1, a2 = int(H.str_off[1]), int(H.str_off[2])
    assert Wt["ins_reads"][a1 + HOMO_AT] >= 10 and Wt["del_reads"][a2 + UNIQUE_AT] >= 10
    assert sum(1 for v in ev[1] if v) >= 10 and sum(1 for v in ev[2] if v) >= 10


def test_edge_case_is_not_vacuous(edges):
    """The restatement alone, on the edge case: it holds aligned reads of every length and both orientations, reads with events of
    both kinds, unaligned and undrawn reads, a first-base and a last-base N among the aligned reads, reads at either end of the
    placement range, N columns, the on-gap without a drawn read, and the read that only an insertion saves."""
    H, Wt = edges
    al = Wt["aligned"]
    lens = np.array([len(s) for s in H.seqs])
    assert {int(v) for v in lens[al]} >= set(EDGE_LENS) and set(H.rev[al]) == {0, 1}
    assert (Wt["n_ins"][al] > 0).sum() > 5 and (Wt["n_del"][al] > 0).sum() > 5
    assert (~al & (H.draw_pos[:H.NU] == INT_MIN)).any() and (~al & (H.draw_pos[:H.NU] != INT_MIN)).any()
    assert any(al[k] and H.seqs[k][0] == ord("N") for k in range(H.NU)) and any(al[k] and H.seqs[k][-1] == ord("N") for k in range(H.NU))
    n_of = np.repeat(H.filled_len, np.diff(H.u_off))
    assert (al & (H.draw_pos[:H.NU] == -(lens - 1))).any() and (al & (H.draw_pos[:H.NU] == n_of - 1)).any()
    assert (H.raw == ord("N")).any() and list(H.state) == [1] * len(H.filled_len)
    g = 7
    assert not al[int(H.u_off[g]):int(H.u_off[g + 1])].any() and not Wt["cover"][int(H.str_off[g]):int(H.str_off[g + 1])].any()
    k = int(H.u_off[8])
    assert Wt["ll_flat"][k] == NINF and np.isfinite(Wt["ll_gapped"][k]) and Wt["n_ins"][k] == 1 and Wt["n_del"][k] == 0
    assert (Wt["ll_gapped"][al] == NINF).sum() == 0 and (Wt["ll_flat"][al] == NINF).any()
    assert (Wt["d_end"][al] != 0).any() and (Wt["d_start"][al] != 0).any() and Wt["cover"].max() > 3


def case_lines(H, Wt, tabs):
    lm, le, lt, lI, lD = tabs
    hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v).reshape(-1))
    lines = [str(len(lm)), hx(lm), hx(le), hx(lt), hx(lI), hx(lD)]
    ks = np.flatnonzero(Wt["aligned"])
    lines.append(str(len(ks)))
    for k in ks:
        g = int(np.searchsorted(H.u_off, k, side="right") - 1)
        n = int(H.filled_len[g])
        S = columns(H.contig, int(H.starts[g]), trp.G0, H.raw[int(H.str_off[g]):int(H.str_off[g]) + n])
        o, ln = int(H.draw_pos[k]), len(H.seqs[k])
        lines += [f"{o} {ln} {int(H.rev[k])}", "".join(str(int(c)) for c in S[PAD + o - W:PAD + o + ln + W]), H.seqs[k].tobytes().decode()]
    return lines, ks


def test_kernel_pieces_on_the_cpu(planted, edges, tmp_path):
    """The __host__ __device__ pieces of fig_indel.h and fig_band.h (the band in tests/band_form.h's form) compiled as plain C++ into a
    program of its own with AddressSanitizer and UBSan (tests/indel_read_main.cpp; run directly), over the aligned reads of the planted, the edge and the band case: inside the program
    the kernel's form (lanes, repeated relaxation of the deletion sweep, packed pointers) equals a sequential restatement in every
    cell and pointer bit for bit; its output equals the numpy restatement, events included."""
    exe = str(tmp_path / "indel_read")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "indel_read_main.cpp")])
    B = band_case()
    noindel = edge_case(model=zero_rate_model())
    total = 0
    for tag, (H, Wt) in (("planted", planted), ("edges", edges), ("band", (B, expected(B))), ("zero", (noindel, expected(noindel)))):
        lines, ks = case_lines(H, Wt, indel_tables(H.model.cstruct()))
        case = tmp_path / f"{tag}.txt"
        case.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(case)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines()]
        assert len(rows) == len(ks) > 3
        bits = lambda i: np.array([int(t[i], 16) for t in rows], dtype=np.uint64).view(np.float64)
        assert tbq.same_bits(bits(0), Wt["ll_flat"][ks]) and tbq.same_bits(bits(1), Wt["ll_gapped"][ks]), tag
        for i, f in ((2, "n_ins"), (3, "n_del"), (4, "d_end"), (5, "d_start")):
            assert [int(t[i]) for t in rows] == list(Wt[f][ks]), (tag, f)
        assert [t[6] for t in rows] == [Wt["events"][k] for k in ks], tag
        total += len(ks)
    assert total > 300


def zero_rate_model():
    m = trp.place_model("unmapped")
    m.ins = np.zeros(len(m.e)); m.dele = np.zeros(len(m.e))
    return m


def test_band_and_zero_rates_on_the_cpu():
    """The restatement alone: a planted 7-base indel of either kind is found as one event and an 8-base one is not (no event, finite
    score); with ins = del = 0 no read has an event, ll_gapped is the best whole-diagonal sum, and the read whose every diagonal is
    -inf reports -inf and zeros."""
    B = band_case()
    Wt = expected(B)
    assert list(Wt["n_del"]) == [7, 0, 0, 0] and list(Wt["n_ins"]) == [0, 0, 7, 0] and list(Wt["d_end"]) == [7, 0, -7, 0]
    assert np.isfinite(Wt["ll_gapped"]).all() and list(Wt["d_start"]) == [0, 0, 0, 0]
    assert Wt["events"][0] == "D60+7" and Wt["events"][1] == "-" and Wt["events"][3] == "-"
    Z = edge_case(model=zero_rate_model())
    Wz = expected(Z)
    al = Wz["aligned"]
    assert not Wz["n_ins"].any() and not Wz["n_del"].any() and not Wz["del_reads"].any() and not Wz["ins_reads"].any()
    assert (Wz["d_end"][al] == Wz["d_start"][al]).all() and (Wz["d_end"][al] != 0).any()
    k = int(Z.u_off[8])
    assert Wz["ll_gapped"][k] == NINF and Wz["ll_flat"][k] == NINF and Wz["d_end"][k] == 0 and Wz["d_start"][k] == 0
    assert not Wz["cover"][int(Z.str_off[8]):int(Z.str_off[9])].any()


def test_abi_surface():
    """the header declares the call and the struct, the version stays 1, and the Python struct has the header's thirteen pointers"""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert "#define FIG_ABI_VERSION 1" in hdr and "int fig_batch_indel(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, fig_gap_indel *out);" in hdr
    body = hdr[hdr.index("typedef struct fig_gap_indel {"):hdr.index("} fig_gap_indel;")]
    names = [ln.split(";")[0].split("*")[-1].strip() for ln in body.splitlines()[1:] if "*" in ln.split("/*")[0]]
    assert names == [f for f, _ in api.FigGapIndel._fields_] and len(names) == 13
    assert "fig_batch_indel" in api.EXPORTS and api.INDEL_W == W


# ------------------------------------------------------------------------------------- GPU
def _run_case(H, origin="own"):
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        return eng.indel(H.result(), H.origin if origin == "own" else origin)
    finally:
        eng.close()


@pytest.mark.gpu
def test_planted_edits(planted):
    """fig_batch_indel on the planted case: every array the restatement's, bit for bit; so no call on the unedited string, one 'I' on
    the homopolymer's first column, one 'D' on the inserted base."""
    H, Wt = planted
    I = _run_case(H)
    compare(I, Wt)
    calls = [I.call[int(H.str_off[g]):int(H.str_off[g + 1])].tobytes().decode() for g in range(3)]
    assert calls[0].count(".") == 101 and calls[1].replace(".", "") == "I" and calls[1][HOMO_AT] == "I" and calls[2].replace(".", "") == "D" and calls[2][UNIQUE_AT] == "D"
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_edges_on_the_device(edges):
    """fig_batch_indel on the edge case (1 .. 65 reads, lengths 1 .. 200 mixed, N bases and columns, flanks and contig ends, the ends of
    the placement range, unaligned and undrawn reads, n = 1 and n = 300, an on-gap without a drawn read, -inf mismatches that an
    insertion routes around): every array the restatement's, bit for bit; the buffers came in as 0xFF bytes."""
    H, Wt = edges
    compare(_run_case(H), Wt)


@pytest.mark.gpu
def test_band_on_the_device():
    """a planted 7-base indel of either kind is found, an 8-base one is not: no event, finite score"""
    B = band_case()
    I = _run_case(B)
    compare(I, expected(B))
    assert list(I.n_del) == [7, 0, 0, 0] and list(I.n_ins) == [0, 0, 7, 0] and np.isfinite(I.ll_gapped).all()


@pytest.mark.gpu
def test_zero_rates_on_the_device():
    """ins = del = 0: no events, ll_gapped the best whole-diagonal sum, the all -inf read reports -inf and zeros"""
    Z = edge_case(model=zero_rate_model())
    I = _run_case(Z)
    compare(I, expected(Z))
    k = int(Z.u_off[8])
    assert not I.n_ins.any() and not I.n_del.any() and I.ll_gapped[k] == NINF and I.d_start[k] == 0


@pytest.mark.gpu
def test_off_means_off():
    """trp.HandPlace's gap list with its off states: the restatement over the gaps that are on, defaults everywhere else over buffers
    that came in as 0xFF bytes; without origins the ORIGINAL gap is on too; a partial-mode model aligns nothing; a NULL member, a
    drawn offset of 2^20 in a gap that is on and a freed batch are FIG_EINVAL."""
    H = trp.HandPlace()
    Wt = expected(H)
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        I = eng.indel(H.result(), H.origin)
        compare(I, Wt)
        assert list(I.state) == trp.STATE and Wt["aligned"].sum() > 100 and (~Wt["aligned"]).sum() > 30
        for g in np.flatnonzero(I.state == 0):
            a, b = int(H.str_off[g]), int(H.str_off[g + 1])
            assert not I.cover[a:b].any() and I.call[a:b].tobytes() == b"." * (b - a) and I.d_start[int(H.u_off[g]):int(H.u_off[g + 1])].tolist() == [INT_MIN] * int(H.u_off[g + 1] - H.u_off[g])
        I2 = eng.indel(H.result(), None)
        st2 = [1, 1, 1, 1, 1, 0, 0, 1, 1]
        compare(I2, expected(H, state=st2))
        r, keep = eng._filled_struct("indel", H.result())
        gi = api.FigGapIndel()
        assert eng.lib.fig_batch_indel(eng.ctx, C.byref(r), None, C.byref(gi)) == -1
        # |o*| = 2^20 is refused in a gap that is on and not looked at in a gap that is off
        for k, v, ok in ((int(H.u_off[2]) + 1, 1 << 20, False), (int(H.u_off[2]) + 1, -(1 << 20), False), (int(H.u_off[2]) + 1, (1 << 20) - 1, True), (int(H.u_off[6]) + 1, 1 << 20, True)):
            B = trp.HandPlace()
            B.draw_pos[k] = v
            if ok:
                eng.indel(B.result(), B.origin)
            else:
                with pytest.raises(RuntimeError):
                    eng.indel(B.result(), B.origin)
        eng.free_batch()
        with pytest.raises(RuntimeError):
            eng.indel(H.result(), H.origin)
    finally:
        eng.close()
    P = trp.HandPlace(mode="partial")
    eng = api.Engine(0)
    try:
        eng.set_model(P.model)
        eng.upload(P.batch)
        I = eng.indel(P.result(), P.origin)
        assert len(I.ll_gapped) == 0 and not I.state.any() and not I.cover.any() and I.call.tobytes() == b"." * len(I.call) and I.call_end.tobytes() == b"." * len(I.state)
    finally:
        eng.close()


def run_golden_indel(root):
    """A golden filled as figfill fills it (draw and support planes), then Engine.indel with the returned origins while the batch is
    resident, then a second plain fill -> Fill with .I, .second and what the restatement needs"""
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
        F.tabs = indel_tables(cm); F.unmapped = bool(cm.unmapped_flag); F.nu = nu
        eng = api.Engine(0)
        try:
            eng.set_model_struct(cm)
            eng.upload_struct(cb)
            reach = np.zeros(max(n, 1), dtype=np.uint8); reach[:n] = eng.probe_reach()
            preset = np.zeros(max(n, 1), dtype=np.uint8)
            host.fighost_run_ot_presets(h, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
            eng.set_ot_preset(preset[:n])
            res = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, indel=True, keep_resident=True)
            F.second = _take(Fill(), eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.I = res.indel
        return F
    finally:
        host.fighost_run_close(h)


@pytest.fixture(scope="module")
def ifills(tmp_path_factory):
    """name -> golden filled with the draw and support planes and the indel evidence; computed once per module, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden_indel(util.extract_golden(name, str(tmp_path_factory.mktemp(name))))
        return cache[name]
    return get


class _View:
    """a golden's fill under the attribute names expected() reads"""

    def __init__(self, F):
        self.NU, self.filled_len, self.str_off, self.raw, self.u_off, self.draw_pos, self.rev = F.nu, F.filled_len, F.str_off, F.raw, F.u_off, F.draw_pos, F.u_rev
        self.seqs = [F.u_seq[int(F.u_seq_off[k]):int(F.u_seq_off[k + 1])] for k in range(F.nu)]
        self.F = F


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "bench_b160"])
def test_goldens_end_to_end(name, ifills):
    """A golden filled as figfill fills it, then the indel evidence: states by the rule and every array the restatement's, bit for bit;
    a second fill of the still resident batch returns the bytes of the first."""
    F = ifills(name)
    assert F.unmapped
    V = _View(F)
    state = []
    for g in range(F.n):
        n = int(F.filled_len[g]); org = int(F.origin[g])
        state.append(int(n > 0 and int(F.draw_len[2 * g]) == n and int(F.draw_len[2 * g + 1]) < 0 and bool(org & F_) and not org & O_))
    total, NU = int(F.str_off[F.n]), F.nu
    w = dict(ll_flat=np.zeros(NU), ll_gapped=np.zeros(NU), n_ins=np.zeros(NU, np.int32), n_del=np.zeros(NU, np.int32), d_end=np.zeros(NU, np.int32),
             d_start=np.full(NU, INT_MIN, np.int32), del_reads=np.zeros(total, np.int32), ins_reads=np.zeros(total, np.int32), cover=np.zeros(total, np.int32),
             ins_end=np.zeros(F.n, np.int32), call=np.full(total, ord("."), np.uint8), call_end=np.full(F.n, ord("."), np.uint8), state=np.array(state, dtype=np.uint8))
    aligned = 0
    for g in range(F.n):
        if not state[g]:
            continue
        n = int(F.filled_len[g]); c = int(F.gap_contig[g])
        a, b = int(F.str_off[g]), int(F.str_off[g]) + n
        S = columns(F.contig[int(F.contig_off[c]):int(F.contig_off[c + 1])], int(F.start[g]), int(F.G0[g]), F.raw[a:b])
        ks = [k for k in range(int(F.u_off[g]), int(F.u_off[g + 1])) if is_aligned(int(F.draw_pos[k]), len(V.seqs[k]), n)]
        rs, dl, il, cv, ie = restate_gap(S, n, [(V.seqs[k], int(F.u_rev[k]), int(F.draw_pos[k])) for k in ks], F.tabs)
        for k, r in zip(ks, rs):
            for f in ("ll_flat", "ll_gapped", "n_ins", "n_del", "d_end", "d_start"):
                w[f][k] = r[f]
        aligned += len(ks)
        w["del_reads"][a:b] = dl; w["ins_reads"][a:b] = il; w["cover"][a:b] = cv; w["ins_end"][g] = ie
        w["call"][a:b] = np.frombuffer(call_of(dl, il, cv).encode(), dtype=np.uint8)
        w["call_end"][g] = ord("I") if (ie >= 2 and 2 * ie > cv[n - 1]) else ord(".")
    compare(F.I, w)
    print(f"{name}: gaps on {sum(state)}, aligned {aligned}, reads with an event {int(((w['n_ins'] + w['n_del']) > 0).sum())}, columns called {int((w['call'] != ord('.')).sum())}")
    assert aligned > 0 and w["cover"].any()
    for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
        assert np.array_equal(getattr(F, f), getattr(F.second, f)), f


@pytest.mark.gpu
def test_gapindel_file_is_the_same_from_every_host_path(ifills, tmp_path, monkeypatch):
    """unmapped_small with FIGFILL_INDEL=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 and two-rank figfill_mp leave the same
    gapindel.txt, which is the file of Engine.indel's calls; the reference's files stay byte-identical in every run; without the
    variable the file is absent."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    name = "unmapped_small"
    for v in ("FIGFILL_SUPPORT", "FIGFILL_QUALITY", "FIGFILL_PLACEMENT", "FIGFILL_QUALITY_MINPQ", "FIGFILL_SOFTQUALITY", "FIGFILL_INDEL"):
        monkeypatch.delenv(v, raising=False)
    roots = [util.extract_golden(name, str(tmp_path / f"r{k}")) for k in range(4)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    r = util.run([util.FIGFILL] + argv, roots[3])
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[0], {"FIGFILL_INDEL": "1"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[1], {"FIGFILL_INDEL": "1", "FIGFILL_DEVICES": "0,0"})
    assert r.returncode == 0, r.stderr
    monkeypatch.setenv("FIGFILL_INDEL", "1")                                # the spawned ranks inherit it
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
    files = [util.read(os.path.join(root, "tmp", "gapindel.txt")) for root in roots[:3]]
    assert files[0] == files[1] == files[2]
    F = ifills(name)
    exp = _gapout(roots[0])
    lines = files[0].splitlines()
    assert len(lines) == len(exp) == F.n
    for g, (ln, e) in enumerate(zip(lines, exp)):
        f = ln.split("\t")
        assert len(f) == 8 and f[:5] == e[:5] and f[5] == str(int(F.I.state[g]))
        assert f[6] == F.I.call[int(F.str_off[g]):int(F.str_off[g + 1])].tobytes().decode() and f[7] == chr(F.I.call_end[g])
    assert any(ln.split("\t")[5] == "1" for ln in lines)
    for k, root in enumerate(roots):
        assert os.path.exists(os.path.join(root, "tmp", "gapindel.txt")) == (k < 3)
        assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)


def test_figfill_names_a_missing_call(tmp_path):
    """FIGFILL_INDEL=1 on a library without fig_batch_indel (the one-lane emulation) is an error that names the call, before anything
    is filled or written; the host library has the bindings and FillResult the field"""
    host = api.load_host_library()
    for fn in ("fighost_indel_tables", "fighost_indel_gaps_on", "fighost_indel_aligned", "fighost_indel_end_order", "fighost_indel_call", "fighost_indel_call_end",
               "fighost_run_write_indel"):
        assert hasattr(host, fn), fn
    assert "indel" in api.FillResult.__dataclass_fields__
    root = util.extract_golden("unmapped_small", str(tmp_path))
    r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, {"FIGFILL_INDEL": "1"})
    assert r.returncode != 0 and "fig_batch_indel" in r.stderr
    for fn in ("gapindel.txt", "gapout.txt"):
        assert not os.path.exists(os.path.join(root, "tmp", fn)), fn
