"""Polish of the filled strings (fig_batch_polish, include/figbird_hip.h: fig_gap_polish).

The restatement below writes the whole loop out in numpy and plain Python, independently of fig_polish_host.h: a gap's current
string is a list of cells (an original column, or an inserted base that remembers which column's list it belongs to), an edit is a
list operation, every candidate is scored by building the edited string and running test_indel_evidence's band over it, and the
edit words are made from the cell list at the very end.  Every integer output of the device is compared with it for equality and
every double on its int64 view: the device only adds table entries and compares.
"""
import ctypes as C
import os
import socket
import subprocess

import numpy as np
import pytest

import util
from figbird_amd import api
import test_read_placement as trp
import test_indel_evidence as tie
from test_base_support import CODE, INT_MIN, _gapout, _open_run
from test_indel_evidence import ACGT, END_ORDER, NINF, PAD, W, Case, band, clean_model, columns, planted_case, restate_gap

DEL, INS = 0, 1
ON, EDITED, REJECTED, REVERTED, CAPPED = 1, 2, 4, 8, 16
MAX_SITES, MAX_K = 16, 7
F_, O_ = api.SUP_FINAL, api.SUP_ORIGINAL


# ------------------------------------------------------------------------------------- the restatement
def shift(o, kind, x):
    if kind == INS:
        return o + 1 if o >= x else o
    return o - 1 if o > x else o


def touched(o, ln, x):
    return o - (W + 1) <= x <= o + ln + W


def counted(o, ln, n, kind, x):
    return tie.is_aligned(o, ln, n) and touched(o, ln, x) and tie.is_aligned(shift(o, kind, x), ln, n + 1 if kind == INS else n - 1)


def fsum(values):
    """from 0.0, one IEEE addition each, in the order given"""
    t = 0.0
    for v in values:
        t = t + float(v)
    return t


class Cells:
    """the current string of a gap of n0 original columns as a list of cells: ("o", x, byte) or ("i", owner column, byte)"""

    def __init__(self, string):
        self.n0 = len(string)
        self.c = [("o", x, int(b)) for x, b in enumerate(string)]

    def string(self):
        return np.array([b for _, _, b in self.c], dtype=np.uint8)

    def owner_of_insert(self, y):
        return self.n0 if y == len(self.c) else self.c[y][1]

    def can_insert(self, y):
        own = self.owner_of_insert(y)
        return sum(1 for k, o, _ in self.c if k == "i" and o == own) < MAX_K

    def insert(self, y, byte):
        self.c.insert(y, ("i", self.owner_of_insert(y), int(byte)))

    def remove(self, y):
        del self.c[y]

    def words(self):
        """-> (edit [n0], edit_end)"""
        lists = [[] for _ in range(self.n0 + 1)]
        kept = set()
        for k, o, b in self.c:
            if k == "i":
                lists[o].append(int(CODE[b]))
            else:
                kept.add(o)
        w = []
        for x in range(self.n0 + 1):
            v = (0 if (x in kept or x == self.n0) else 1) | (len(lists[x]) << 1)
            for i, code in enumerate(lists[x]):
                v |= code << (4 + 2 * i)
            w.append(v)
        return np.array(w[:-1], dtype=np.int32), w[-1]


def indel_pass(contig, start, G0, string, reads, offs, tabs):
    """test_indel_evidence's restatement of one gap -> (ll_gapped per read index (dict, aligned reads only), call (str), call_end)"""
    n = len(string)
    S = columns(contig, start, G0, string)
    ks = [i for i, (seq, _, _) in enumerate(reads) if tie.is_aligned(offs[i], len(seq), n)]
    rs, dl, il, cv, ie = restate_gap(S, n, [(reads[i][0], reads[i][1], offs[i]) for i in ks], tabs)
    ll = {i: r["ll_gapped"] for i, r in zip(ks, rs)}
    return ll, tie.call_of(dl, il, cv), ("I" if (ie >= 2 and 2 * ie > cv[n - 1]) else ".")


def candidate_scores(contig, start, G0, string, reads, offs, tabs, kind, x, byte):
    """ll_c of the counted reads of one candidate -> {read index: ll_c}: the edited string is built and the band run over it"""
    n = len(string)
    new = np.insert(string, x, byte) if kind == INS else np.delete(string, x)
    ks = [i for i, (seq, _, _) in enumerate(reads) if counted(offs[i], len(seq), n, kind, x)]
    if not ks:
        return {}
    S = columns(contig, start, G0, new)
    H, _, _ = band(S, [(reads[i][0], reads[i][1], shift(offs[i], kind, x)) for i in ks], tabs)
    out = {}
    for a, i in enumerate(ks):
        best = NINF
        for d in END_ORDER:
            if H[a, d + W] > best:
                best = float(H[a, d + W])
        out[i] = best
    return out


def polish_gap(contig, start, G0, string, reads, tabs, max_rounds, log=None):
    """The loop of one gap that is on.  reads: [(seq, rev, o*)], undrawn ones included -> dict of the gap's outputs"""
    cells = Cells(string)
    offs = [int(r[2]) for r in reads]
    orig = list(offs)
    lens = [len(r[0]) for r in reads]
    ll0, call, call_end = indel_pass(contig, start, G0, string, reads, offs, tabs)
    cur_ll = dict(ll0)
    state, rounds, active = ON, 0, True
    for _ in range(max_rounds):
        cur = cells.string()
        n = len(cur)
        sites = [(x, DEL if ch == "D" else INS) for x, ch in enumerate(call) if ch != "."]
        if call_end != ".":
            sites.append((n, INS))
        sites = sites[:MAX_SITES]
        if not sites:
            active = False
            break
        rounds += 1
        accepted, proposed = [], 0
        for x, kind in sites:
            if (kind == DEL and n < 2) or (kind == INS and not cells.can_insert(x)):
                state |= CAPPED
                continue
            proposed += 1
            bytes_ = [0] if kind == DEL else list(ACGT)
            T, T0 = [], None
            for b in bytes_:
                sc = candidate_scores(contig, start, G0, cur, reads, offs, tabs, kind, x, b)
                T.append(fsum(sc[i] for i in sorted(sc)))
                T0 = fsum(cur_ll[i] for i in sorted(sc))
            best = 0
            for i in range(1, len(T)):
                if T[i] > T[best]:
                    best = i
            if log is not None:
                log.append((kind, x, T, T0))
            if T[best] > T0:
                accepted.append((x, kind, bytes_[best]))
            else:
                state |= REJECTED
        if not accepted:
            active = False
            break
        saved = (list(cells.c), list(offs))
        applied = 0
        for x, kind, b in reversed(accepted):
            if kind == DEL:
                if len(cells.c) < 2:
                    state |= CAPPED
                    continue
                cells.remove(x)
            else:
                if not cells.can_insert(x):
                    state |= CAPPED
                    continue
                cells.insert(x, b)
            offs = [o if o == INT_MIN else shift(o, kind, x) for o in offs]
            applied += 1
        if not applied:
            active = False
            break
        new = cells.string()
        ll_new, call_new, ce_new = indel_pass(contig, start, G0, new, reads, offs, tabs)
        both = [i for i in range(len(reads)) if tie.is_aligned(saved[1][i], lens[i], n) and tie.is_aligned(offs[i], lens[i], len(new))]
        if fsum(ll_new[i] for i in both) > fsum(cur_ll[i] for i in both):
            state |= EDITED
            cur_ll, call, call_end = ll_new, call_new, ce_new
        else:
            state |= REVERTED
            cells.c, offs = saved
            active = False
            break
    if active and (call.strip(".") or call_end != "."):
        state |= CAPPED
    final = cells.string()
    edit, edit_end = cells.words()
    both = [i for i in range(len(reads)) if tie.is_aligned(orig[i], lens[i], len(string)) and tie.is_aligned(offs[i], lens[i], len(final))]
    return dict(edit=edit, edit_end=edit_end, polished_len=len(final), draw_pos=offs, n_ins=sum(1 for k, _, _ in cells.c if k == "i"),
                n_del=len(string) - sum(1 for k, _, _ in cells.c if k == "o"), rounds=rounds, ll_before=fsum(ll0[i] for i in both),
                ll_after=fsum(cur_ll[i] for i in both), state=state, string=final)


def expected(H, max_rounds=4, tabs=None, state=None, logs=None):
    """The restatement of a whole hand-made case (a Case or a trp.HandPlace) -> dict of the arrays of fig_gap_polish, plus `strings`"""
    tabs = tabs or tie.indel_tables(H.model.cstruct())
    state = H.state if state is None else state
    NU, total, ng = H.NU, int(H.str_off[-1]), len(H.filled_len)
    w = dict(edit=np.zeros(total, np.int32), edit_end=np.zeros(ng, np.int32), polished_len=np.array(H.filled_len, dtype=np.int32), draw_pos=np.array(H.draw_pos[:NU], dtype=np.int32),
             n_ins=np.zeros(ng, np.int32), n_del=np.zeros(ng, np.int32), rounds=np.zeros(ng, np.int32), ll_before=np.zeros(ng), ll_after=np.zeros(ng),
             state=np.zeros(ng, np.uint8), strings=[])
    for g in range(ng):
        a, n = int(H.str_off[g]), max(int(H.filled_len[g]), 0)
        if not state[g]:
            w["strings"].append(np.array(H.raw[a:a + n], dtype=np.uint8))
            continue
        k0, k1 = int(H.u_off[g]), int(H.u_off[g + 1])
        reads = [(H.seqs[k], int(H.rev[k]), int(H.draw_pos[k])) for k in range(k0, k1)]
        log = [] if logs is not None else None
        contig, start, G0 = H.geometry(g) if hasattr(H, "geometry") else (H.contig, int(H.starts[g]), trp.G0)
        r = polish_gap(contig, start, G0, np.array(H.raw[a:a + n], dtype=np.uint8), reads, tabs, max_rounds, log)
        if logs is not None:
            logs.append(log)
        w["edit"][a:a + n] = r["edit"]
        w["draw_pos"][k0:k1] = r["draw_pos"]
        for f in ("edit_end", "polished_len", "n_ins", "n_del", "rounds", "ll_before", "ll_after", "state"):
            w[f][g] = r[f]
        w["strings"].append(r["string"])
    return w


FIELDS_D = ("ll_before", "ll_after")
FIELDS_I = ("edit", "edit_end", "polished_len", "draw_pos", "n_ins", "n_del", "rounds", "state")


def compare(P, want):
    """every array of the device against the restatement's: doubles on their int64 view, everything else equal; and the strings"""
    for f in FIELDS_D:
        bad = np.flatnonzero(np.asarray(getattr(P, f)).view(np.int64) != np.asarray(want[f]).view(np.int64))
        assert not len(bad), f"{f}: gaps {bad[:8]}: got {getattr(P, f)[bad[:4]]}, want {want[f][bad[:4]]}"
    for f in FIELDS_I:
        got = np.asarray(getattr(P, f))
        assert got.shape == want[f].shape and got.dtype == want[f].dtype, f
        bad = np.flatnonzero(got != want[f])
        assert not len(bad), f"{f}: elements {bad[:8]}: got {got[bad[:4]]}, want {want[f][bad[:4]]}"
    got = P.strings()
    assert len(got) == len(want["strings"])
    for g, (a, b) in enumerate(zip(got, want["strings"])):
        assert a.tobytes() == b.tobytes(), g


# ------------------------------------------------------------------------------------- hand-made cases
def gap_from_truth(rng, truth, string, picks, left, right, tmap=lambda t: t, sub=0.005, lo=300):
    """reads copied from left + truth + right at the picks' true offsets (truth coordinates) with `sub` substitutions, each drawn at its
    best ungapped offset against left + string + right around tmap(t)"""
    full_t = np.concatenate([left, truth, right]); full = np.concatenate([left, string, right])
    reads = []
    for ln, t, rev in picks:
        q = tie.mutate(rng, full_t[lo + t:lo + t + ln], sub)
        reads.append((q, rev, tie.best_flat_offset(q, full, tmap(t), -lo)))
    return dict(string=string, reads=reads, left=left, right=right)


def unique_truth(rng, n):
    """n random columns with no two equal neighbours: an edit of one column has one place to go"""
    t = rng.choice(ACGT, size=n).copy()
    for i in range(1, n):
        while t[i] == t[i - 1]:
            t[i] = rng.choice(ACGT)
    return t


def multi_case():
    """Three gaps over 40 reads of 60 .. 77 bases each: two errors 50 columns apart in one 121-column gap (a base missing and a base
    too many); two adjacent missing bases; two adjacent extra bases."""
    rng = np.random.default_rng(20261101)
    gaps = []
    for which in range(3):
        left = unique_truth(rng, 300); right = unique_truth(rng, 300)
        truth = unique_truth(rng, 121 if which == 0 else 101)
        if which == 0:
            string = np.insert(np.delete(truth, 30), 79, ACGT[(int(CODE[truth[80]]) + 2) % 4])
        elif which == 1:
            string = np.delete(truth, [50, 51])
        else:
            extra = np.array([ACGT[(int(CODE[truth[49]]) + 1) % 4], ACGT[(int(CODE[truth[50]]) + 2) % 4]], dtype=np.uint8)
            if extra[0] == extra[1] or extra[1] == truth[50]:
                extra[1] = ACGT[(int(CODE[extra[1]]) + 1) % 4]
            string = np.insert(truth, 50, extra)
        picks = [(int(rng.integers(60, 78)), int(rng.integers(-30, len(truth) - 30)), int(rng.integers(0, 2))) for _ in range(40)]
        gaps.append((gap_from_truth(rng, truth, string, picks, left, right), truth))
    return Case([g for g, _ in gaps], clean_model()), [t for _, t in gaps]


SPLIT_AT = 50


def split_gaps():
    """One gap of 100 columns and 30 forward reads of 60 bases that all span column 50: 18 carry a base there that the fill lacks
    (they were copied from the 101-column truth) and 12 do not (copied from the fill itself); no substitutions"""
    rng = np.random.default_rng(20261102)
    left = unique_truth(rng, 300); right = unique_truth(rng, 300)
    truth = unique_truth(rng, 101)
    string = np.delete(truth, SPLIT_AT)
    if string[SPLIT_AT - 1] == string[SPLIT_AT]:                 # keep the fill free of equal neighbours as well
        truth[SPLIT_AT + 1] = ACGT[(int(CODE[truth[SPLIT_AT + 1]]) + 1) % 4]
        if truth[SPLIT_AT + 1] in (truth[SPLIT_AT], truth[SPLIT_AT + 2], truth[SPLIT_AT - 1]):
            truth[SPLIT_AT + 1] = [b for b in ACGT if b not in (truth[SPLIT_AT], truth[SPLIT_AT + 2], truth[SPLIT_AT - 1])][0]
        string = np.delete(truth, SPLIT_AT)
    picks = [(60, 5 + r, 0) for r in range(30)]
    a = gap_from_truth(rng, truth, string, picks[:18], left, right, sub=0.0)
    b = gap_from_truth(rng, string, string, picks[18:], left, right, sub=0.0)
    return [dict(string=string, reads=a["reads"] + b["reads"], left=left, right=right)], truth


def split_model():
    return clean_model(ins=0.2, dele=1e-12)


HOMO2_AT = 40


def homo2_case():
    """A homopolymer of six A's at truth columns 40 .. 45, filled two bases short; 40 reads of 60 .. 77 bases"""
    rng = np.random.default_rng(20261103)
    left = unique_truth(rng, 300); right = unique_truth(rng, 300)
    truth = unique_truth(rng, 101)
    truth[HOMO2_AT - 1] = ord("C"); truth[HOMO2_AT:HOMO2_AT + 6] = ord("A"); truth[HOMO2_AT + 6] = ord("G")
    truth[HOMO2_AT - 2] = ord("T"); truth[HOMO2_AT + 7] = ord("T")
    string = np.delete(truth, [HOMO2_AT, HOMO2_AT + 1])
    picks = [(int(rng.integers(60, 78)), int(rng.integers(-30, 75)), int(rng.integers(0, 2))) for _ in range(40)]
    return Case([gap_from_truth(rng, truth, string, picks, left, right)], clean_model()), truth


@pytest.fixture(scope="module")
def planted():
    H = planted_case()
    logs = []
    return H, expected(H, logs=logs), logs


@pytest.fixture(scope="module")
def multi():
    H, truths = multi_case()
    return H, expected(H), truths


@pytest.fixture(scope="module")
def split():
    gaps, truth = split_gaps()
    Hr, Ha = Case(gaps, split_model()), Case(gaps, clean_model())
    logs = []
    return Hr, expected(Hr, logs=logs), Ha, expected(Ha), truth, logs


@pytest.fixture(scope="module")
def homo2():
    H, truth = homo2_case()
    return H, expected(H), expected(H, max_rounds=1), truth


EDGE_LENS = (60, 1, 16, 17, 199, 200, 31, 70, 65)
EDGE_SITE = 50
EDGE_NAMES = ("x0", "xn", "del_to_1", "d_at_1", "many", "r2", "r63", "r64", "r65", "bounds", "off_origin", "off_header", "nocall")


def edge_case():
    """One gap per edge (EDGE_NAMES): a missing first column (a site at x = 0); a missing last column (a site at x = n, through
    call_end); two columns where the truth has one (a DEL that leaves n = 1); one column where the truth has none (a 'D' call at
    n = 1, which is not proposed); 18 unique columns missing from a 400-column truth (more than 16 called columns); a missing base at
    column 50 seen by 2, 63, 64 and 65 reads (a call needs two reads) of the lengths 1, 16, 17, 199, 200, 31 and others mixed in
    a chunk, every fifth with an N beside the site, on a string with N columns three and nine columns from it; the same site with
    reads whose offsets sit at and one beyond the touched bounds (x + 8, x + 9, x - len - 7, x - len - 8) and undrawn reads; the
    site in a gap that is off by its origin and in one that is off by its header; and a correct string."""
    rng = np.random.default_rng(20261104)
    gaps, truths = [], []

    def flanks():
        return unique_truth(rng, 300), unique_truth(rng, 300)

    def spanning(count, n, site, lens=(60, 66, 72)):
        out = []
        for r in range(count):
            ln = lens[r % len(lens)]
            lo_t, hi_t = max(site - ln + 1, -140), min(site, n + 140 - ln)
            out.append((ln, int(rng.integers(lo_t, hi_t + 1)), r % 2))
        return out

    # x0, xn
    for which in (0, 1):
        left, right = flanks(); truth = unique_truth(rng, 61)
        while truth[0] == left[-1] or truth[-1] == right[0]:
            truth = unique_truth(rng, 61)
        string = truth[1:].copy() if which == 0 else truth[:-1].copy()
        site = 0 if which == 0 else 60
        gaps.append(gap_from_truth(rng, truth, string, spanning(30, 61, site), left, right, tmap=(lambda t: t - 1 if t > 0 else t) if which == 0 else (lambda t: t)))
        truths.append(truth)
    # del_to_1, d_at_1
    for which in (0, 1):
        left, right = flanks()
        left[-1] = ord("C"); left[-2] = ord("T"); right[0] = ord("T"); right[1] = ord("C")
        truth = np.frombuffer(b"G" if which == 0 else b"", dtype=np.uint8).copy()
        string = np.frombuffer(b"GA" if which == 0 else b"G", dtype=np.uint8).copy()
        picks = [(60, int(rng.integers(-50, -8)), r % 2) for r in range(30)]
        gaps.append(gap_from_truth(rng, truth, string, picks, left, right))
        truths.append(truth)
    # many
    left, right = flanks(); truth = unique_truth(rng, 400)
    gone = [15 + 20 * i for i in range(18)]
    for c in gone:                                               # a removed column leaves no equal neighbours behind
        while truth[c - 1] == truth[c + 1]:
            truth[c + 1] = rng.choice(ACGT)
            while truth[c + 1] in (truth[c], truth[c + 2]):
                truth[c + 1] = rng.choice(ACGT)
    string = np.delete(truth, gone)
    picks = [(int(rng.integers(60, 78)), int(rng.integers(-40, 380)), int(rng.integers(0, 2))) for _ in range(220)]
    gaps.append(gap_from_truth(rng, truth, string, picks, left, right, tmap=lambda t: t - sum(1 for c in gone if c < t)))
    truths.append(truth)
    # r2 .. r65, bounds, off_origin, off_header
    for name in EDGE_NAMES[5:12]:
        left, right = flanks(); truth = unique_truth(rng, 101)
        string = np.delete(truth, EDGE_SITE)
        count = {"r2": 2, "r63": 63, "r64": 64, "r65": 65}.get(name, 30)
        gp = gap_from_truth(rng, truth, string, spanning(count, 101, EDGE_SITE, EDGE_LENS if name[0] == "r" and name != "r2" else (60, 66, 72)), left, right,
                            tmap=lambda t: t - 1 if t > EDGE_SITE else t)
        if name[0] == "r":
            string[EDGE_SITE + 3] = ord("N"); string[EDGE_SITE - 9] = ord("N")
            for r in range(0, count, 5):
                seq, rev, o = gp["reads"][r]
                j = EDGE_SITE - o + (1 if r % 2 else -2)
                if 0 <= j < len(seq):
                    seq[j] = ord("N")
        if name == "bounds":
            x = EDGE_SITE
            for o in (x + 8, x + 9, x - 60 - 7, x - 60 - 8, x - 8, x - 9):
                t = o + (1 if o > x else 0)
                gp["reads"].append((np.concatenate([left, truth, right])[300 + t:300 + t + 60].copy(), 0, o))
            gp["reads"] += [(gp["reads"][r][0].copy(), 1, INT_MIN) for r in range(3)]
        if name == "off_origin":
            gp["origin"] = F_ | O_
        if name == "off_header":
            gp["hdr"] = 101
        gaps.append(gp); truths.append(truth)
    left, right = flanks(); truth = unique_truth(rng, 80)
    gaps.append(gap_from_truth(rng, truth, truth.copy(), spanning(20, 80, 40), left, right)); truths.append(truth)
    return Case(gaps, clean_model()), truths


@pytest.fixture(scope="module")
def edges():
    H, truths = edge_case()
    return H, expected(H), truths


# ------------------------------------------------------------------------------------- CPU
def test_shift_touched_counted_by_hand():
    """The three rules at o* = x, x +- 8, x - len - 7 and one past each, through the host library's bindings, against values worked
    out by hand and against the restatement's own functions"""
    host = api.load_host_library()
    x, ln, n = 100, 60, 300
    # INS shifts a read that starts at or after x; DEL one that starts after x
    assert [host.fighost_polish_shift(o, INS, x) for o in (99, 100, 101)] == [99, 101, 102]
    assert [host.fighost_polish_shift(o, DEL, x) for o in (99, 100, 101)] == [99, 100, 100]
    # touched iff o - 8 <= x <= o + len + 7
    by_hand = {x: 1, x + 8: 1, x + 9: 0, x - 8: 1, x - 9: 1, x - ln - 7: 1, x - ln - 8: 0, x - ln - 6: 1}
    for o, want in by_hand.items():
        assert host.fighost_polish_touched(o, ln, x) == want == int(touched(o, ln, x)), o
    # counted needs both alignments: a read that starts on the last column stays there when that column goes (o* = x is not moved)
    # and is then off the end of the n - 1 columns; a DEL further left moves it along
    assert host.fighost_polish_counted(-(ln - 1), ln, n, DEL, 0) == 1 and host.fighost_polish_counted(n - 1, ln, n, DEL, n - 1) == 0
    assert host.fighost_polish_counted(n - 1, ln, n, DEL, n - 5) == 1                   # shifted to n - 2 = n_c - 1: still aligned
    assert host.fighost_polish_counted(0, 1, 1, INS, 0) == 1                            # moved to 1 of 2 columns
    assert host.fighost_polish_counted(1, 1, 2, DEL, 0) == 1 and host.fighost_polish_counted(1, 1, 2, DEL, 1) == 0      # o* = 1 stays, n_c = 1: off the end
    assert host.fighost_polish_counted(INT_MIN, ln, n, INS, x) == 0 and host.fighost_polish_counted(n, ln, n, INS, n) == 0
    for kind in (DEL, INS):
        for o in (x, x + 8, x + 9, x - 8, x - 9, x - ln - 7, x - ln - 8, -(ln - 1), -ln, n - 1, n, INT_MIN):
            for nn in (n, x + 1, 2):
                if kind == DEL and not 0 <= x < nn or kind == INS and not 0 <= x <= nn:
                    continue
                assert host.fighost_polish_counted(o, ln, nn, kind, x) == int(counted(o, ln, nn, kind, x)), (kind, o, nn)


def _book(n0, ops):
    """a script of ("I", y, code) / ("D", y) through the host library -> [(return code, edit list, edit_end)]"""
    host = api.load_host_library()
    edit = np.zeros(max(n0, 1), dtype=np.int32); end = np.zeros(1, dtype=np.int32)
    out = []
    for op in ops:
        if op[0] == "I":
            rc = host.fighost_polish_insert(api._p(edit, api.c_i32_p), n0, api._p(end, api.c_i32_p), op[1], op[2])
        else:
            rc = host.fighost_polish_remove(api._p(edit, api.c_i32_p), n0, api._p(end, api.c_i32_p), op[1])
        out.append((rc, [int(v) for v in edit[:n0]], int(end[0])))
    return out


def test_edit_plane_bookkeeping_by_hand():
    """insert before an original column (the end of its list); insert before an inserted base (that position of the same list); remove
    an inserted base; remove an original column; the place after the last cell; k = 7 kept and the eighth refused; the polished string"""
    word = lambda removed, codes: removed | (len(codes) << 1) | sum(c << (4 + 2 * i) for i, c in enumerate(codes))
    r = _book(3, [("I", 1, 2)])                                  # ACG -> A g CG: the list of column 1
    assert r[-1] == (1, [0, word(0, [2]), 0], 0)
    r = _book(3, [("I", 1, 2), ("I", 2, 3)])                     # before cell 2 = column 1 itself: joins the end of its list
    assert r[-1] == (1, [0, word(0, [2, 3]), 0], 0)
    r = _book(3, [("I", 1, 2), ("I", 2, 3), ("I", 1, 1)])        # before cell 1 = the inserted g: takes its position
    assert r[-1] == (1, [0, word(0, [1, 2, 3]), 0], 0)
    r = _book(3, [("I", 1, 2), ("I", 2, 3), ("I", 1, 1), ("D", 2)])      # cell 2 is the g again: out of the list
    assert r[-1] == (1, [0, word(0, [1, 3]), 0], 0)
    r = _book(3, [("I", 1, 2), ("D", 2)])                        # cell 2 is column 1: removed, its list stays
    assert r[-1] == (1, [0, word(1, [2]), 0], 0)
    r = _book(3, [("I", 3, 0), ("I", 4, 3), ("D", 3)])           # after the last cell: edit_end's list, then its first base out again
    assert [x[2] for x in r] == [word(0, [0]), word(0, [0, 3]), word(0, [3])] and all(x[0] == 1 and x[1] == [0, 0, 0] for x in r)
    assert _book(3, [("I", 4, 0)])[-1][0] == -1 and _book(3, [("D", 3)])[-1][0] == -1 and _book(3, [("D", -1)])[-1][0] == -1
    seven = [("I", 0, i & 3) for i in range(7)]
    r = _book(2, seven + [("I", 0, 1), ("I", 7, 1), ("I", 8, 2)])
    assert r[6][0] == 1 and (r[6][1][0] >> 1) & 7 == 7 and r[7][0] == 0 and r[8][0] == 0 and r[7][1] == r[6][1] == r[8][1]
    assert r[9] == (1, [r[6][1][0], word(0, [2])], 0)            # cell 8 is column 1: its own list is empty still
    # the string: Polish.strings()'s function and the host library's fig_polish_apply agree with the cells
    c = Cells(np.frombuffer(b"ACG", dtype=np.uint8))
    c.insert(1, ord("G")); c.insert(2, ord("T")); c.remove(3); c.insert(len(c.c), ord("A"))
    edit, end = c.words()
    assert c.string().tobytes() == b"AGTGA" and api.polish_string(edit, end, b"ACG").tobytes() == b"AGTGA"
    assert list(edit) == [0, word(1, [2, 3]), 0] and end == word(0, [0])


def test_apply_through_both_libraries():
    """fig_polish_apply from libfighost.so and, where it is built, libfighip.so: the polished string of a gap that is on, the own bytes
    of a gap that is off, the length alone with dst NULL, and FIG_EINVAL where polished_len disagrees with the planes"""
    word = lambda removed, codes: removed | (len(codes) << 1) | sum(c << (4 + 2 * i) for i, c in enumerate(codes))
    fl = np.array([3, 2], dtype=np.int32); so = np.array([0, 3, 6], dtype=np.int64); raw = np.frombuffer(b"ACGTTx", dtype=np.uint8).copy()
    edit = np.array([0, word(1, [2, 3]), 0, word(0, [1]), 0, 0], dtype=np.int32); end = np.array([word(0, [0]), 0], dtype=np.int32)
    plen = np.array([5, 2], dtype=np.int32); st = np.array([ON | EDITED, 0], dtype=np.uint8)
    r = api.FigGapResults(); r.filled_len = api._p(fl, api.c_i32_p); r.str_off = api._p(so, api.c_i64_p); r.str = C.cast(raw.ctypes.data, C.c_char_p)
    p = api.FigGapPolish(); p.edit = api._p(edit, api.c_i32_p); p.edit_end = api._p(end, api.c_i32_p); p.polished_len = api._p(plen, api.c_i32_p); p.state = api._p(st, api.c_u8_p)
    libs = [api.load_host_library()] + ([api.load_library()] if os.path.exists(util.pbuild.LIB) else [])
    for lib in libs:
        dst = np.full(8, ord("#"), dtype=np.uint8)
        assert lib.fig_polish_apply(C.byref(r), C.byref(p), 0, api._p(dst, api.c_u8_p)) == 5 and dst.tobytes() == b"AGTGA###"
        assert lib.fig_polish_apply(C.byref(r), C.byref(p), 0, None) == 5
        dst[:] = ord("#")
        assert lib.fig_polish_apply(C.byref(r), C.byref(p), 1, api._p(dst, api.c_u8_p)) == 2 and dst.tobytes() == b"TT######"
        plen[0] = 4
        assert lib.fig_polish_apply(C.byref(r), C.byref(p), 0, api._p(dst, api.c_u8_p)) == -1
        plen[0] = 5
        assert lib.fig_polish_apply(None, C.byref(p), 0, None) == -1 and lib.fig_polish_apply(C.byref(r), C.byref(p), -1, None) == -1


def test_sites_best_accept_and_verify_by_hand():
    """sites: ascending columns, then the junction, sixteen at most; best: the greatest, ties to the first; accept and keep: strictly
    greater, -inf included"""
    host = api.load_host_library()
    xs = np.zeros(16, dtype=np.int32); ks = np.zeros(16, dtype=np.int32)
    sites = lambda call, ce: (host.fighost_polish_sites(call, len(call), ce, api._p(xs, api.c_i32_p), api._p(ks, api.c_i32_p)), list(xs), list(ks))
    m, x, k = sites(b"..D.I.", b"I")
    assert m == 3 and x[:3] == [2, 4, 6] and k[:3] == [DEL, INS, INS]
    assert sites(b"......", b".")[0] == 0 and sites(b"", b"I")[0] == 1 and xs[0] == 0
    m, x, k = sites(b"D" * 20, b"I")
    assert m == 16 and x == list(range(16)) and k == [DEL] * 16
    m, x, k = sites(b"I" * 15, b"I")
    assert m == 16 and x[15] == 15 and k == [INS] * 16
    best = lambda v: host.fighost_polish_best(api._p(np.array(v, dtype=np.float64), api.c_double_p), len(v))
    assert best([-5.0, -3.0, -3.0, -4.0]) == 1 and best([NINF, NINF, NINF, NINF]) == 0 and best([-2.0]) == 0 and best([NINF, -900.0, NINF, -900.0]) == 1
    for fn in (host.fighost_polish_accept, host.fighost_polish_keep):
        assert fn(-10.0, -11.0) == 1 and fn(-10.0, -10.0) == 0 and fn(-11.0, -10.0) == 0
        assert fn(NINF, NINF) == 0 and fn(-1e300, NINF) == 1 and fn(NINF, -1e300) == 0


def test_polished_writer_format(tmp_path):
    """fighost_run_write_polished on hand-made planes: `g contig start G0 n polished_len state n_ins n_del P`, P rebuilt from the planes"""
    root = util.extract_golden("unmapped_small", str(tmp_path))
    exp = _gapout(root)
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        fl = np.arange(3, 3 + n, dtype=np.int32); fl[0] = 0
        so = np.concatenate([[0], np.cumsum(fl)]).astype(np.int64)
        raw = np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(int(so[-1])) % 4].copy()
        edit = np.zeros(int(so[-1]), dtype=np.int32); end = np.zeros(n, dtype=np.int32)
        st = np.where(np.arange(n) % 2 == 1, ON | EDITED, 0).astype(np.uint8)
        nins = np.zeros(n, dtype=np.int32); ndel = np.zeros(n, dtype=np.int32); plen = fl.copy()
        want_str = []
        for g in range(n):
            a = int(so[g])
            if st[g]:
                edit[a] = 1; edit[a + 1] = (2 << 1) | (3 << 4) | (1 << 6); end[g] = (1 << 1) | (2 << 4)     # column 0 out, "TC" before column 1, "G" at the end
                nins[g], ndel[g], plen[g] = 3, 1, fl[g] + 2
                want_str.append(b"TC" + raw[a + 1:a + int(fl[g])].tobytes() + b"G")
            else:
                want_str.append(raw[a:a + int(fl[g])].tobytes())
        err = C.create_string_buffer(512)
        cwd = os.getcwd(); os.chdir(root)
        try:
            args = lambda: (h, api._p(fl, api.c_i32_p), api._p(so, api.c_i64_p), C.cast(raw.ctypes.data, C.c_char_p), api._p(edit, api.c_i32_p), api._p(end, api.c_i32_p),
                            api._p(plen, api.c_i32_p), api._p(st, api.c_u8_p), api._p(nins, api.c_i32_p), api._p(ndel, api.c_i32_p), err, 512)
            rc = host.fighost_run_write_polished(*args())
            got = util.read(os.path.join(root, "tmp", "gappolished.txt"))
            plen[1] += 1
            rc_bad = host.fighost_run_write_polished(*args())
        finally:
            os.chdir(cwd)
    finally:
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    want = "".join("\t".join(exp[g][:4]) + f"\t{fl[g]}\t{plen[g] - (1 if g == 1 else 0)}\t{st[g]}\t{nins[g]}\t{ndel[g]}\t" + want_str[g].decode() + "\n" for g in range(n))
    assert n >= 2 and got == want and "\t3\t3\t1\tTC" in got
    assert rc_bad != 0 and "gap 1" in err.value.decode()


def test_abi_surface(tmp_path):
    """the header declares the two calls and the struct, the version stays 1, the Python struct has the header's ten pointers in its
    order and its size, the constants agree, and both calls are in EXPORTS"""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert "#define FIG_ABI_VERSION 1" in hdr
    assert "int fig_batch_polish(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, int max_rounds, fig_gap_polish *out);" in hdr
    assert "int fig_polish_apply(const fig_gap_results *filled, const fig_gap_polish *p, int64_t g, char *dst);" in hdr
    body = hdr[hdr.index("typedef struct fig_gap_polish {"):hdr.index("} fig_gap_polish;")]
    names = [ln.split(";")[0].split("*")[-1].strip() for ln in body.splitlines()[1:] if "*" in ln.split("/*")[0]]
    assert names == [f for f, _ in api.FigGapPolish._fields_] and len(names) == 10
    assert "fig_batch_polish" in api.EXPORTS and "fig_polish_apply" in api.EXPORTS and "polish" in api.FillResult.__dataclass_fields__
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu %d %d %d %d %d %d %d %d", sizeof(fig_gap_polish), sizeof(fig_gap_results), '
           'FIG_POLISH_ON, FIG_POLISH_EDITED, FIG_POLISH_REJECTED, FIG_POLISH_REVERTED, FIG_POLISH_CAPPED, FIG_POLISH_MAX_SITES, FIG_POLISH_MAX_ROUNDS, FIG_POLISH_DEFAULT_ROUNDS);'
           + "".join(f'printf(" %zu", offsetof(fig_gap_polish, {f}));' for f in names) + 'printf("\\n");return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = subprocess.check_output([str(tmp_path / "t")], text=True).split()
    assert [int(v) for v in out] == [C.sizeof(api.FigGapPolish), C.sizeof(api.FigGapResults), api.POLISH_ON, api.POLISH_EDITED, api.POLISH_REJECTED, api.POLISH_REVERTED,
                                     api.POLISH_CAPPED, api.POLISH_MAX_SITES, api.POLISH_MAX_ROUNDS, api.POLISH_DEFAULT_ROUNDS] + [getattr(api.FigGapPolish, f).offset for f in names]
    assert (ON, EDITED, REJECTED, REVERTED, CAPPED, MAX_SITES) == (api.POLISH_ON, api.POLISH_EDITED, api.POLISH_REJECTED, api.POLISH_REVERTED, api.POLISH_CAPPED, api.POLISH_MAX_SITES)


def _gap(H, Wt, g, f):
    return Wt[f][int(H.str_off[g]):int(H.str_off[g + 1])]


def test_planted_case_is_not_vacuous(planted, multi):
    """The restatement alone.  planted_case(): the unedited gap has no site and equal sums bit for bit; the homopolymer one base short
    gets exactly one INS at column 45, A is the one best of the four candidates (the other three tie below it), and the string ends equal to the truth;
    the gap with a base too many gets exactly one DEL at column 52 and ends equal to the truth.  The multi-error gaps end equal to
    their truths: two errors in one gap in one round, two adjacent extra bases in one round, two adjacent missing bases (one INS run
    in the reads, so one site) in two."""
    H, Wt, logs = planted
    truth = Wt["strings"][0]
    assert truth.tobytes() == H.raw[:101].tobytes() and all(s.tobytes() == truth.tobytes() for s in Wt["strings"])
    assert list(Wt["state"]) == [ON, ON | EDITED, ON | EDITED] and list(Wt["rounds"]) == [0, 1, 1]
    assert list(Wt["n_ins"]) == [0, 1, 0] and list(Wt["n_del"]) == [0, 0, 1] and list(Wt["polished_len"]) == [101, 101, 101] and not Wt["edit_end"].any()
    assert np.flatnonzero(_gap(H, Wt, 1, "edit")).tolist() == [tie.HOMO_AT] and _gap(H, Wt, 1, "edit")[tie.HOMO_AT] == 1 << 1                # k = 1, base A
    assert np.flatnonzero(_gap(H, Wt, 2, "edit")).tolist() == [tie.UNIQUE_AT] and _gap(H, Wt, 2, "edit")[tie.UNIQUE_AT] == 1
    assert logs[0] == [] and len(logs[1]) == 1 and len(logs[2]) == 1
    kind, x, T, T0 = logs[1][0]
    assert (kind, x) == (INS, tie.HOMO_AT) and T[0] > T0 and all(t < T[0] for t in T[1:]) and T[1] == T[2] == T[3]
    kind, x, T, T0 = logs[2][0]
    assert (kind, x) == (DEL, tie.UNIQUE_AT) and T[0] > T0
    assert Wt["ll_before"].view(np.int64)[0] == Wt["ll_after"].view(np.int64)[0] and (Wt["ll_after"][1:] > Wt["ll_before"][1:]).all()
    assert abs(Wt["ll_before"][1] + 155.357) < 1e-3 and abs(Wt["ll_after"][1] + 53.2187) < 1e-4            # the sums over all forty reads
    # the offsets moved by the rule: a read at or right of the inserted column by one
    k0 = int(H.u_off[1])
    for k in range(k0, int(H.u_off[2])):
        assert Wt["draw_pos"][k] == H.draw_pos[k] + (1 if H.draw_pos[k] >= tie.HOMO_AT else 0)
    M, Wm, truths = multi
    assert all(s.tobytes() == t.tobytes() for s, t in zip(Wm["strings"], truths)) and all(s.tobytes() != M.raw[int(M.str_off[g]):int(M.str_off[g + 1])].tobytes() for g, s in enumerate(Wm["strings"]))
    assert list(Wm["state"]) == [ON | EDITED] * 3 and list(Wm["rounds"]) == [1, 2, 1] and list(Wm["n_ins"]) == [1, 2, 0] and list(Wm["n_del"]) == [1, 0, 2]


def test_rejection_case_is_not_vacuous(split):
    """The restatement alone, on the 60/40 reads: under ins = 0.2, del = 1e-12 there is one 'I' call, every candidate loses, nothing is
    edited and REJECTED is set; under clean_model() the same call is accepted and the truth restored"""
    Hr, Wr, Ha, Wa, truth, logs = split
    assert len(logs[0]) == 1 and logs[0][0][:2] == (INS, SPLIT_AT) and all(t < logs[0][0][3] for t in logs[0][0][2])
    assert list(Wr["state"]) == [ON | REJECTED] and list(Wr["rounds"]) == [1] and not Wr["edit"].any() and not Wr["n_ins"].any()
    assert Wr["strings"][0].tobytes() == Hr.raw[:100].tobytes() and Wr["ll_before"].view(np.int64)[0] == Wr["ll_after"].view(np.int64)[0]
    assert list(Wr["draw_pos"]) == list(Hr.draw_pos[:Hr.NU])
    assert list(Wa["state"]) == [ON | EDITED] and list(Wa["n_ins"]) == [1] and Wa["strings"][0].tobytes() == truth.tobytes()


def test_rounds_case_is_not_vacuous(homo2):
    """The restatement alone, on the homopolymer two bases short: both missing bases normalise to the run's first column, so one base
    per round: two rounds at the default (k = 2, "AA" before column 40, the truth restored); with max_rounds = 1 one base, EDITED and
    CAPPED"""
    H, W4, W1, truth = homo2
    assert list(W4["state"]) == [ON | EDITED] and list(W4["rounds"]) == [2] and list(W4["n_ins"]) == [2] and W4["strings"][0].tobytes() == truth.tobytes()
    assert np.flatnonzero(W4["edit"]).tolist() == [HOMO2_AT] and W4["edit"][HOMO2_AT] == 2 << 1
    assert list(W1["state"]) == [ON | EDITED | CAPPED] and list(W1["rounds"]) == [1] and list(W1["n_ins"]) == [1] and W1["edit"][HOMO2_AT] == 1 << 1
    assert W1["ll_after"][0] > W1["ll_before"][0] and W4["ll_after"][0] > W1["ll_after"][0]


def test_edge_case_is_not_vacuous(edges):
    """The restatement alone, on the edge case: what each gap was built for happens"""
    H, Wt, truths = edges
    g = {name: i for i, name in enumerate(EDGE_NAMES)}
    same = lambda name: Wt["strings"][g[name]].tobytes() == truths[g[name]].tobytes()
    a = lambda name: int(H.str_off[g[name]])
    assert Wt["state"][g["x0"]] == ON | EDITED and (Wt["edit"][a("x0")] >> 1) & 7 == 1 and same("x0")
    assert Wt["state"][g["xn"]] == ON | EDITED and (Wt["edit_end"][g["xn"]] >> 1) & 7 == 1 and not _gap(H, Wt, g["xn"], "edit").any() and same("xn")
    assert Wt["state"][g["del_to_1"]] == ON | EDITED and Wt["polished_len"][g["del_to_1"]] == 1 and Wt["n_del"][g["del_to_1"]] == 1 and same("del_to_1")
    assert Wt["state"][g["d_at_1"]] == ON | CAPPED and Wt["rounds"][g["d_at_1"]] == 1 and Wt["polished_len"][g["d_at_1"]] == 1 and not Wt["n_del"][g["d_at_1"]]
    assert Wt["state"][g["many"]] == ON | EDITED and Wt["rounds"][g["many"]] == 2 and Wt["n_ins"][g["many"]] == 18 and same("many")
    for name in ("r2", "r63", "r64", "r65", "bounds"):
        assert Wt["state"][g[name]] == ON | EDITED and Wt["n_ins"][g[name]] == 1 and (_gap(H, Wt, g[name], "edit")[EDGE_SITE] >> 1) & 7 == 1, name
        assert Wt["edit"][a(name) + EDGE_SITE] >> 4 == CODE[truths[g[name]][EDGE_SITE]], name
    assert same("bounds") and (H.raw[a("r64"):a("r64") + 100] == ord("N")).sum() == 2
    lens = {len(H.seqs[k]) for k in range(int(H.u_off[g["r63"]]), int(H.u_off[g["r65"] + 1]))}
    assert lens >= set(EDGE_LENS) and any((H.seqs[k] == ord("N")).any() for k in range(int(H.u_off[g["r63"]]), int(H.u_off[g["r63"] + 1])))
    assert [int(H.u_off[g[nm] + 1] - H.u_off[g[nm]]) for nm in ("r2", "r63", "r64", "r65")] == [2, 63, 64, 65]
    kb = range(int(H.u_off[g["bounds"]]), int(H.u_off[g["bounds"] + 1]))
    offs = [int(H.draw_pos[k]) for k in kb]
    for o in (EDGE_SITE + 8, EDGE_SITE + 9, EDGE_SITE - 67, EDGE_SITE - 68):
        assert o in offs
    assert offs.count(INT_MIN) == 3 and all(Wt["draw_pos"][k] == INT_MIN for k in kb if H.draw_pos[k] == INT_MIN)
    for name in ("off_origin", "off_header"):
        assert Wt["state"][g[name]] == 0 and not _gap(H, Wt, g[name], "edit").any() and Wt["polished_len"][g[name]] == 100
    assert Wt["state"][g["nocall"]] == ON and Wt["rounds"][g["nocall"]] == 0 and Wt["ll_before"].view(np.int64)[g["nocall"]] == Wt["ll_after"].view(np.int64)[g["nocall"]]


def _program_case(H, Wt_logs, tabs, rng, extra_candidates=()):
    """the case file of tests/polish_main.cpp for the first round of every gap of H that is on: the candidates the restatement logged
    (all four bases of an INS site) plus `extra_candidates` per gap -> (lines, [(gap, kind, x, code, [read indices])])"""
    lm, le, lt, lI, lD = tabs
    hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v).reshape(-1))
    lines = [str(len(lm)), hx(lm), hx(le), hx(lt), hx(lI), hx(lD)]
    on = [g for g in range(len(H.filled_len)) if H.state[g]]
    lines.append(str(len(on)))
    index = []
    for li, g in enumerate(on):
        n = int(H.filled_len[g]); a = int(H.str_off[g])
        S = columns(H.contig, int(H.starts[g]), trp.G0, H.raw[a:a + n])
        fl = [int(S[PAD - 1 - i]) for i in range(208)] + [int(S[PAD + n + i]) for i in range(208)]
        cands = [(kind, x, b) for kind, x, _, _ in Wt_logs[li] for b in (range(4) if kind == INS else [0])] + list(extra_candidates)
        cands = [c for c in cands if (c[0] == INS and 0 <= c[1] <= n) or (c[0] == DEL and 0 <= c[1] < n and n >= 2)]
        lines += [str(n), "".join(str(v) for v in fl), H.raw[a:a + n].tobytes().decode(), str(len(cands))]
        ks = list(range(int(H.u_off[g]), int(H.u_off[g + 1])))
        ks = [k for k in ks if H.draw_pos[k] != INT_MIN]
        for kind, x, b in cands:
            lines.append(f"{kind} {x} {b} {len(ks)}")
            for k in ks:
                lines += [f"{int(H.draw_pos[k])} {len(H.seqs[k])} {int(H.rev[k])}", H.seqs[k].tobytes().decode()]
            index.append((g, kind, x, b, ks))
    return lines, index


def test_kernel_pieces_on_the_cpu(planted, edges, split, tmp_path):
    """The __host__ __device__ pieces of fig_polish.h and fig_polish_host.h compiled as plain C++ into a program of its own with
    AddressSanitizer and UBSan (tests/polish_main.cpp; run directly), over the first-round candidates of the planted, the edge and
    the rejection case and a few candidates nobody called (the string's ends, a DEL beside an N): inside the program the kernel's form
    equals a sequential restatement over the edited string bit for bit; its output equals the numpy restatement, which reads counted
    and which not included; and a script of insertions and removals leaves the words and strings of the cell-list model."""
    exe = str(tmp_path / "polish_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "polish_main.cpp")])
    rng = np.random.default_rng(7)
    Hr, Wr, _, _, _, logs_r = split
    He, We, _ = edges
    logs_e = []
    expected(He, max_rounds=1, logs=logs_e)
    total = 0
    for tag, H, logs, extra in (("planted", planted[0], planted[2], [(DEL, 0, 0), (INS, 0, 3), (INS, 10 ** 6, 1), (DEL, 99, 0)]), ("split", Hr, logs_r, [(DEL, SPLIT_AT, 0)]),
                                ("edges", He, logs_e, [(INS, 1, 2), (DEL, 0, 0), (DEL, EDGE_SITE + 2, 0), (INS, EDGE_SITE - 9, 0)])):
        tabs = tie.indel_tables(H.model.cstruct())
        lines, index = _program_case(H, logs, tabs, rng, extra)
        ops = [("I", 1, 2), ("I", 2, 3), ("I", 1, 1), ("D", 2), ("D", 0), ("I", 0, 0), ("D", 5), ("I", 4, 1), ("I", 9, 0)] + [("I", 3, i & 3) for i in range(8)] + [("D", 3), ("D", 40)]
        lines.append(f"BOOK 5 ACGTA {len(ops)}")
        lines += [" ".join(str(v) for v in op) for op in ops]
        case = tmp_path / f"{tag}.txt"
        case.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(case)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines()]
        crow = [t for t in rows if t[0] == "C"]; brow = [t for t in rows if t[0] == "B"]
        at = 0
        for g, kind, x, b, ks in index:
            n = int(H.filled_len[g]); a = int(H.str_off[g]); k0 = int(H.u_off[g])
            reads = [(H.seqs[k], int(H.rev[k]), int(H.draw_pos[k])) for k in range(k0, int(H.u_off[g + 1]))]
            sc = candidate_scores(H.contig, int(H.starts[g]), trp.G0, np.array(H.raw[a:a + n]), reads, [r_[2] for r_ in reads], tabs, kind, x, ACGT[b])
            for k in ks:
                t = crow[at]; at += 1
                assert int(t[1]) == int((k - k0) in sc), (tag, g, kind, x, k)
                if (k - k0) in sc:
                    assert np.array([int(t[2], 16)], dtype=np.uint64).view(np.float64)[0].hex() == float(sc[k - k0]).hex(), (tag, g, kind, x, b, k)
                    total += 1
        assert at == len(crow)
        # the bookkeeping script against the cell list
        cells = Cells(np.frombuffer(b"ACGTA", dtype=np.uint8))
        assert len(brow) == len(ops)
        for op, t in zip(ops, brow):
            y = op[1]
            if op[0] == "I":
                rc = -1 if not 0 <= y <= len(cells.c) else (1 if cells.can_insert(y) else 0)
                if rc == 1:
                    cells.insert(y, ACGT[op[2]])
            else:
                rc = 1 if 0 <= y < len(cells.c) else -1
                if rc == 1:
                    cells.remove(y)
            edit, end = cells.words()
            assert int(t[1]) == rc and t[2] == (cells.string().tobytes().decode() or "-") and [int(v, 16) for v in t[3:]] == list(edit) + [end], (op, t)
    assert total > 1000


def test_figfill_names_a_missing_call(tmp_path):
    """FIGFILL_POLISH=1 on a library without fig_batch_polish (the one-lane emulation) is an error that names the call, before anything
    is filled or written; Python refuses likewise; the host library has the bindings"""
    host = api.load_host_library()
    for fn in ("fig_polish_apply", "fighost_polish_shift", "fighost_polish_touched", "fighost_polish_counted", "fighost_polish_sites", "fighost_polish_best", "fighost_polish_accept",
               "fighost_polish_keep", "fighost_polish_insert", "fighost_polish_remove", "fighost_run_write_polished"):
        assert hasattr(host, fn), fn
    root = util.extract_golden("unmapped_small", str(tmp_path))
    r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, {"FIGFILL_POLISH": "1"})
    assert r.returncode != 0 and "fig_batch_polish" in r.stderr
    for fn in ("gappolished.txt", "gapout.txt"):
        assert not os.path.exists(os.path.join(root, "tmp", fn)), fn
    emu = C.CDLL(util.EMULIB)
    assert not hasattr(emu, "fig_batch_polish")


# ------------------------------------------------------------------------------------- GPU
class _Eng:
    """an engine with the model and the batch of a hand-made case resident"""

    def __init__(self, H):
        self.H = H

    def __enter__(self):
        self.eng = api.Engine(0)
        try:
            self.eng.set_model(self.H.model)
            self.eng.upload(self.H.batch)
        except Exception:
            self.eng.close()
            raise
        return self.eng

    def __exit__(self, *a):
        self.eng.close()


def _no_call(I):
    return I.call.tobytes() == b"." * len(I.call) and I.call_end.tobytes() == b"." * len(I.call_end)


@pytest.mark.gpu
def test_planted_edits_are_applied(planted, multi):
    """fig_batch_polish on planted_case() and on the three multi-error gaps: every field the restatement's, bit for bit; the polished
    strings equal the truth; Engine.indel on Polish.result() makes no call, and its ll_gapped sums to ll_after"""
    for H, Wt, truths in ((planted[0], planted[1], [planted[1]["strings"][0]] * 3), multi):
        with _Eng(H) as eng:
            P = eng.polish(H.result(), H.origin)
            compare(P, Wt)
            for s, t in zip(P.strings(), truths):
                assert s.tobytes() == t.tobytes()
            R = P.result()
            I = eng.indel(R, H.origin)
            assert _no_call(I) and list(I.state) == [1] * len(truths)
            for g in range(len(truths)):
                assert fsum(I.ll_gapped[int(H.u_off[g]):int(H.u_off[g + 1])]) == P.ll_after[g]     # every read is aligned under both strings here
            q = eng.quality(R, H.origin)
            assert len(q[1]) == int(R.str_off[-1]) and list(q[2]) == [1] * len(truths)
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_rejected_call_is_left_alone(split):
    """the 60/40 reads under ins 0.2 / del 1e-12: a call, no edit, REJECTED, the string and the offsets the caller's; the same reads
    under clean_model(): accepted, the truth restored"""
    Hr, Wr, Ha, Wa, truth, _ = split
    with _Eng(Hr) as eng:
        I = eng.indel(Hr.result(), Hr.origin)
        assert I.call.tobytes().replace(b".", b"") == b"I" and I.call[SPLIT_AT] == ord("I")
        P = eng.polish(Hr.result(), Hr.origin)
        compare(P, Wr)
        assert P.state[0] == ON | REJECTED and not P.edit.any() and P.strings()[0].tobytes() == Hr.raw[:100].tobytes() and list(P.draw_pos) == list(Hr.draw_pos[:Hr.NU])
    with _Eng(Ha) as eng:
        P = eng.polish(Ha.result(), Ha.origin)
        compare(P, Wa)
        assert P.state[0] == ON | EDITED and P.strings()[0].tobytes() == truth.tobytes()


@pytest.mark.gpu
def test_one_base_per_site_and_round(homo2):
    """the homopolymer two bases short: the truth after two rounds at the default; with max_rounds = 1 one base, EDITED | CAPPED; with
    max_rounds = 8 what the default gives"""
    H, W4, W1, truth = homo2
    with _Eng(H) as eng:
        P4 = eng.polish(H.result(), H.origin)
        compare(P4, W4)
        assert P4.strings()[0].tobytes() == truth.tobytes() and P4.rounds[0] == 2
        P1 = eng.polish(H.result(), H.origin, max_rounds=1)
        compare(P1, W1)
        assert P1.state[0] == ON | EDITED | CAPPED and P1.n_ins[0] == 1
        compare(eng.polish(H.result(), H.origin, max_rounds=8), W4)
        compare(eng.polish(H.result(), H.origin, max_rounds=4), W4)


@pytest.mark.gpu
def test_edges_on_the_device(edges):
    """the edge case (sites at x = 0 and x = n, a DEL that leaves n = 1, a 'D' call at n = 1, eighteen called columns, 2 / 63 / 64 / 65
    reads of the lengths 1 .. 200 mixed, N bases and N columns beside the site, offsets at and beyond the touched bounds, undrawn
    reads, two gaps that are off, a gap with no call): every field the restatement's, bit for bit, over buffers that came in as
    0xFF bytes"""
    H, Wt, truths = edges
    with _Eng(H) as eng:
        P = eng.polish(H.result(), H.origin)
        compare(P, Wt)
        I = eng.indel(P.result(), H.origin)
        g = EDGE_NAMES.index("many")
        assert I.call[int(P.result().str_off[g]):int(P.result().str_off[g + 1])].tobytes() == b"." * 400


@pytest.mark.gpu
def test_off_means_off_and_every_einval():
    """trp.HandPlace's gap list with its off states: the restatement over the gaps that are on, zeros, the own length and the caller's
    offsets everywhere else; without origins the ORIGINAL gap is on too; a partial-mode model polishes nothing; a NULL member, a
    max_rounds outside 0..8, a drawn offset of 2^20 in a gap that is on and a freed batch are FIG_EINVAL."""
    H = trp.HandPlace()
    Wt = expected(H)
    with _Eng(H) as eng:
        P = eng.polish(H.result(), H.origin)
        compare(P, Wt)
        assert [int(s & ON) for s in P.state] == trp.STATE
        for g in np.flatnonzero(P.state == 0):
            a, b = int(H.str_off[g]), int(H.str_off[g + 1])
            assert not P.edit[a:b].any() and P.polished_len[g] == H.filled_len[g] and P.ll_before[g] == 0.0 and P.ll_after[g] == 0.0
            assert list(P.draw_pos[int(H.u_off[g]):int(H.u_off[g + 1])]) == list(H.draw_pos[int(H.u_off[g]):int(H.u_off[g + 1])])
        compare(eng.polish(H.result(), None), expected(H, state=[1, 1, 1, 1, 1, 0, 0, 1, 1]))
        r, keep = eng._filled_struct("polish", H.result())
        nu, total, n = H.NU, int(H.str_off[-1]), len(H.filled_len)
        bufs = dict(edit=np.zeros(total, np.int32), edit_end=np.zeros(n, np.int32), polished_len=np.zeros(n, np.int32), draw_pos=np.zeros(nu, np.int32), n_ins=np.zeros(n, np.int32),
                    n_del=np.zeros(n, np.int32), rounds=np.zeros(n, np.int32), ll_before=np.zeros(n), ll_after=np.zeros(n), state=np.zeros(n, np.uint8))

        def call(skip=None, rounds=0):
            gp = api.FigGapPolish()
            for f, typ in api.FigGapPolish._fields_:
                if f != skip:
                    setattr(gp, f, api._p(bufs[f], typ))
            return eng.lib.fig_batch_polish(eng.ctx, C.byref(r), None, rounds, C.byref(gp))
        assert call() == 0
        for f, _ in api.FigGapPolish._fields_:
            assert call(skip=f) == -1, f
        assert call(rounds=-1) == -1 and call(rounds=9) == -1 and call(rounds=8) == 0 and call(rounds=1) == 0
        assert eng.lib.fig_batch_polish(eng.ctx, C.byref(r), None, 0, None) == -1 and eng.lib.fig_batch_polish(eng.ctx, None, None, 0, None) == -1
        for k, v, ok in ((int(H.u_off[2]) + 1, 1 << 20, False), (int(H.u_off[2]) + 1, -(1 << 20), False), (int(H.u_off[2]) + 1, (1 << 20) - 1, True), (int(H.u_off[6]) + 1, 1 << 20, True)):
            B = trp.HandPlace()
            B.draw_pos[k] = v
            if ok:
                eng.polish(B.result(), B.origin)
            else:
                with pytest.raises(RuntimeError):
                    eng.polish(B.result(), B.origin)
        eng.free_batch()
        with pytest.raises(RuntimeError):
            eng.polish(H.result(), H.origin)
    Pm = trp.HandPlace(mode="partial")
    with _Eng(Pm) as eng:
        P = eng.polish(Pm.result(), Pm.origin)
        assert len(P.draw_pos) == 0 and not P.state.any() and not P.edit.any() and not P.rounds.any() and list(P.polished_len) == list(Pm.filled_len)


@pytest.mark.gpu
def test_deterministic_and_read_only(planted, homo2):
    """a second call returns the same bytes; fig_batch_indel before and after the call returns the same bytes; the caller's `filled`
    is unchanged"""
    for H in (planted[0], homo2[0]):
        with _Eng(H) as eng:
            res = H.result()
            before = [np.array(a).tobytes() for a in (res.filled_len, res.str_off, res.raw) + tuple(res.draw)]
            fields = [f for f, _ in api.FigGapIndel._fields_]
            I0 = eng.indel(res, H.origin)
            P0 = eng.polish(res, H.origin)
            I1 = eng.indel(res, H.origin)
            P1 = eng.polish(res, H.origin)
            for f in fields:
                assert np.asarray(getattr(I0, f)).tobytes() == np.asarray(getattr(I1, f)).tobytes(), f
            for f, _ in api.FigGapPolish._fields_:
                assert np.asarray(getattr(P0, f)).tobytes() == np.asarray(getattr(P1, f)).tobytes(), f
            assert before == [np.array(a).tobytes() for a in (res.filled_len, res.str_off, res.raw) + tuple(res.draw)]
            tie.compare(I1, tie.expected(H))


class _GoldenView:
    """a golden's fill under the attribute names expected() reads"""

    def __init__(self, F, state):
        self.NU, self.filled_len, self.str_off, self.raw, self.u_off, self.draw_pos, self.rev = F.nu, F.filled_len, F.str_off, F.raw, F.u_off, F.draw_pos, F.u_rev
        self.seqs = [F.u_seq[int(F.u_seq_off[k]):int(F.u_seq_off[k + 1])] for k in range(F.nu)]
        self.state = state
        self.F = F

    def geometry(self, g):
        F = self.F
        c = int(F.gap_contig[g])
        return F.contig[int(F.contig_off[c]):int(F.contig_off[c + 1])], int(F.start[g]), int(F.G0[g])


def run_golden_polish(root, rounds=0):
    """A golden filled as figfill fills it (draw and support planes) with the polish while the batch is resident, then a second plain
    fill -> Fill with .P, .second and what the restatement needs"""
    from test_base_support import Fill, _take
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
        F.tabs = tie.indel_tables(cm); F.unmapped = bool(cm.unmapped_flag); F.nu = nu
        eng = api.Engine(0)
        try:
            eng.set_model_struct(cm)
            eng.upload_struct(cb)
            reach = np.zeros(max(n, 1), dtype=np.uint8); reach[:n] = eng.probe_reach()
            preset = np.zeros(max(n, 1), dtype=np.uint8)
            host.fighost_run_ot_presets(h, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
            eng.set_ot_preset(preset[:n])
            res = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, polish=True, polish_rounds=rounds, keep_resident=True)
            F.second = _take(Fill(), eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.P = res.polish
        return F
    finally:
        host.fighost_run_close(h)


@pytest.fixture(scope="module")
def pfills(tmp_path_factory):
    """name -> golden filled with the draw and support planes and the polish; computed once per module, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden_polish(util.extract_golden(name, str(tmp_path_factory.mktemp(name))))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "bench_b160"])
def test_goldens_end_to_end(name, pfills):
    """A golden filled as figfill fills it, then the polish: states by the rule and every field the restatement's, bit for bit (whatever
    that is on a real fill; it is printed); a second fill of the still resident batch returns the bytes of the first."""
    F = pfills(name)
    assert F.unmapped
    state = []
    for g in range(F.n):
        n = int(F.filled_len[g]); org = int(F.origin[g])
        state.append(int(n > 0 and int(F.draw_len[2 * g]) == n and int(F.draw_len[2 * g + 1]) < 0 and bool(org & F_) and not org & O_))
    V = _GoldenView(F, state)
    Wt = expected(V, tabs=F.tabs)
    compare(F.P, Wt)
    print(f"{name}: gaps on {sum(state)}, states {sorted(set(int(s) for s in F.P.state))}, rounds {int(F.P.rounds.sum())}, inserted {int(F.P.n_ins.sum())}, removed {int(F.P.n_del.sum())}")
    assert sum(state) > 0 and (F.P.ll_before[np.array(state, dtype=bool)] != 0.0).any()
    for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
        assert np.array_equal(getattr(F, f), getattr(F.second, f)), f


@pytest.mark.gpu
def test_gappolished_file_is_the_same_from_every_host_path(pfills, tmp_path, monkeypatch):
    """unmapped_small with FIGFILL_POLISH=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 and two-rank figfill_mp leave the same
    gappolished.txt, which is the file of Engine.polish's result; the reference's files stay byte-identical in every run; without the
    variable the file is absent and gapout.txt, draw.txt and filledContigs.fa are what the runs with it wrote."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    name = "unmapped_small"
    for v in ("FIGFILL_SUPPORT", "FIGFILL_QUALITY", "FIGFILL_PLACEMENT", "FIGFILL_QUALITY_MINPQ", "FIGFILL_SOFTQUALITY", "FIGFILL_INDEL", "FIGFILL_POLISH", "FIGFILL_POLISH_ROUNDS"):
        monkeypatch.delenv(v, raising=False)
    roots = [util.extract_golden(name, str(tmp_path / f"r{k}")) for k in range(4)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    r = util.run([util.FIGFILL] + argv, roots[3])
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[0], {"FIGFILL_POLISH": "1"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[1], {"FIGFILL_POLISH": "1", "FIGFILL_DEVICES": "0,0"})
    assert r.returncode == 0, r.stderr
    monkeypatch.setenv("FIGFILL_POLISH", "1")                               # the spawned ranks inherit it
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
    files = [util.read(os.path.join(root, "tmp", "gappolished.txt")) for root in roots[:3]]
    assert files[0] == files[1] == files[2]
    F = pfills(name)
    exp = _gapout(roots[0])
    lines = files[0].splitlines()
    strs = F.P.strings()
    assert len(lines) == len(exp) == F.n
    for g, (ln, e) in enumerate(zip(lines, exp)):
        f = ln.split("\t")
        assert len(f) == 10 and f[:5] == e[:5]
        assert f[5:9] == [str(int(F.P.polished_len[g])), str(int(F.P.state[g])), str(int(F.P.n_ins[g])), str(int(F.P.n_del[g]))] and f[9] == strs[g].tobytes().decode()
    assert any(int(ln.split("\t")[6]) & ON for ln in lines)
    for k, root in enumerate(roots):
        assert os.path.exists(os.path.join(root, "tmp", "gappolished.txt")) == (k < 3)
        assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt")) and not os.path.exists(os.path.join(root, "tmp", "gapindel.txt"))
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
        for fn in ("gapout.txt", "draw.txt", "filledContigs.fa"):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(roots[3], "tmp", fn)), (root, fn)
    r = util.run([util.FIGFILL] + argv, roots[3], {"FIGFILL_POLISH": "1", "FIGFILL_POLISH_ROUNDS": "9"})
    assert r.returncode != 0 and "fig_batch_polish" in r.stderr
