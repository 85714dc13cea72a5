"""Per-base quality of filled bases (fig_gap_quality / fig_batch_quality, include/figbird_hip.h).

There is no reference for this feature; the header's definition is the specification.  The exact comparisons use a numpy
restatement of it: per gap, its drawn reads in ascending read index, each adding `lm[k]` (read base == true base) or
`le[k] + lt[true][read]` to the four log-likelihoods of the columns it covers, one vectorised `+=` per read and true base (a read
touches a column once, so the order of the additions per column is the read order -- np.sum would reorder and is not used).  The
tables come from fighost_quality_tables, the same code the library runs.  The device only adds table entries in that order, so
the plane must match bit for bit: every comparison is on the int64 view, no tolerance."""
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
from test_base_support import CODE, INT_MIN, Fill, _gapout, _open_run, _take

NINF = -math.inf


# ------------------------------------------------------------------------------------- the restatement
def tables(cm):
    """fig_model struct -> lm [L], le [L], lt [4, 4] (row = true base, column = read base)"""
    host = api.load_host_library()
    L = int(cm.max_read_length)
    lm = np.zeros(L); le = np.zeros(L); lt = np.zeros(16)
    assert host.fighost_quality_tables(C.byref(cm), api._p(lm, api.c_double_p), api._p(le, api.c_double_p), api._p(lt, api.c_double_p)) == 0
    return lm, le, lt.reshape(4, 4)


def restate(n, reads, tabs):
    """reads: (offset, uint8 ASCII array, reversed) of the drawn reads in read order -> float64 [n, 4]"""
    lm, le, lt = tabs
    LL = np.zeros((max(n, 0), 4))
    for o, seq, rev in reads:
        j = np.arange(len(seq), dtype=np.int64)
        x = o + j
        s = CODE[seq]
        ok = (x >= 0) & (x < n) & (s < 4)
        j, x, s = j[ok], x[ok], s[ok]
        k = (len(seq) - 1 - j) if rev else j
        for b in range(4):
            LL[x, b] = LL[x, b] + np.where(s == b, lm[k], le[k] + lt[b, s])       # x holds no index twice
    return LL


def phred_of(ll, raw):
    host = api.load_host_library()
    ll = np.ascontiguousarray(ll, dtype=np.float64); raw = np.ascontiguousarray(raw, dtype=np.uint8)
    out = np.full(max(len(raw), 1), 0xFF, dtype=np.uint8)
    host.fighost_quality_phred(len(raw), api._p(ll if len(ll) else np.zeros((1, 4)), api.c_double_p),
                               C.cast((raw if len(raw) else np.zeros(1, np.uint8)).ctypes.data, C.c_char_p), api._p(out, api.c_u8_p))
    return out[:len(raw)]


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------- the hand-made case
READ_LENS = (31, 77, 150, 200)


def hand_model(mode):
    """L = 200; e[k] different for every k (a wrong reverse index shows), one of them 0; a matrix with distinct off-diagonals,
    one of them 0."""
    L = 200
    e = 0.001 + 0.0001 * np.arange(L) + 1e-6 * (np.arange(L) % 7)
    e[17] = 0.0
    T = np.zeros(25)
    for b in range(5):
        for s in range(5):
            T[b * 5 + s] = 0.0 if b == s else (3 + 7 * b + s) / 100.0
    T[1 * 5 + 2] = 0.0
    assert len(set(e)) == L and len({T[b * 5 + s] for b in range(4) for s in range(4) if b != s}) == 12
    return api.Model(e=e, ins=np.full(L, 1e-4), dele=np.full(L, 1e-4), T=T, insd=np.full(1000, 1e-3), Tmin=0, Tmax=999, cutoff=0,
                     partial_flag=1 if mode == "partial" else 0, unmapped_flag=1 if mode == "unmapped" else 0, script_itr=1,
                     max_distance=500, read_length=200, neg_overlap=30, partial_len=100)


class Hand:
    """A resident batch and a `filled` made by hand.  gaps: per gap (n, unmapped reads, partial reads, evidence 'u' / 'p',
    draw length of the evidence header, origin).  lens: the read lengths, dealt in turn; last_n: the first read of every length
    ends in an N."""

    def __init__(self, mode, gaps, seed, lens=READ_LENS, last_n=False):
        rng = np.random.default_rng(seed)
        self.mode, self.gaps = mode, gaps
        self.model = hand_model(mode)
        ng = len(gaps)
        G0, flank = 50, 300
        contig = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ng * (flank + G0) + flank).copy()
        starts = np.array([flank + g * (flank + G0) for g in range(ng)], dtype=np.int64)
        for st in starts:
            contig[st:st + G0] = ord("N")

        def reads_of(count, n):
            seqs, offs = [], []
            for r in range(count):
                ln = lens[r % len(lens)]
                s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln).copy()
                if r % 5 == 4:
                    s[rng.choice(ln, size=min(ln, 2), replace=False)] = ord("N")
                if last_n and r < len(lens):
                    s[-1] = ord("N")
                seqs.append(s)
                offs.append(INT_MIN if r % 7 == 6 else int(rng.integers(-ln - 2, n + 3)))
            return seqs, offs

        u_off, p_off, u_seq, p_seq, u_pos, p_pos = [0], [0], [], [], [], []
        for n, nu, npart, _, _, _ in gaps:
            s, o = reads_of(nu, n); u_seq += s; u_pos += o; u_off.append(u_off[-1] + nu)
            s, o = reads_of(npart, n); p_seq += s; p_pos += o; p_off.append(p_off[-1] + npart)
        NU, NP = u_off[-1], p_off[-1]
        cat = lambda v: np.concatenate(v) if v else np.zeros(1, dtype=np.uint8)
        soff = lambda v: np.concatenate([[0], np.cumsum([len(s) for s in v])]).astype(np.int64)
        i32 = lambda v: np.asarray(v if len(v) else [0], dtype=np.int32)
        self.u_seqs, self.p_seqs = u_seq, p_seq
        self.u_rev = np.asarray([r % 2 for g in range(ng) for r in range(gaps[g][1])] or [0], dtype=np.uint8)     # alternating within a gap
        self.u_off, self.p_off = np.asarray(u_off, dtype=np.int64), np.asarray(p_off, dtype=np.int64)
        self.batch = api.GapBatch(
            contig_off=np.array([0, len(contig)], dtype=np.int64), contig_seq=contig,
            gap_contig=np.zeros(ng, dtype=np.int32), gap_start=starts, gap_len=np.full(ng, G0, dtype=np.int32),
            gap_stat2=np.zeros(3 * ng, dtype=np.int32), gap_fillflag=np.ones(ng, dtype=np.int32),
            u_read_off=self.u_off, u_anchor_pos=i32([100] * NU), u_is_reverse=self.u_rev, u_seq_off=soff(u_seq), u_seq=cat(u_seq),
            p_read_off=self.p_off, p_clipped_index=i32([10] * NP), p_match=i32([1 + r % 4 for r in range(NP)]), p_pos=i32([100] * NP),
            p_ref_pos=i32([-1] * NP), p_seq_off=soff(p_seq), p_seq=cat(p_seq), p_qual=np.full(max(int(soff(p_seq)[-1]), 1), ord("I"), dtype=np.uint8),
            gap_ot_preset=np.zeros(ng, dtype=np.uint8) if mode == "partial" else None)
        if mode == "partial":          # a partial-mode upload packs no unmapped reads: the draw planes hold the partial reads alone
            u_pos, NU = [], 0
        self.NU = NU
        self.filled_len = np.array([g[0] for g in gaps], dtype=np.int32)
        self.str_off = np.concatenate([[0], np.cumsum(self.filled_len)]).astype(np.int64)
        self.raw = rng.choice(np.frombuffer(b"ACGTACGTACGTN", dtype=np.uint8), size=max(int(self.str_off[-1]), 1)).copy()
        self.draw_pos = i32(u_pos + p_pos)
        self.draw_isz = np.zeros(len(self.draw_pos), dtype=np.int32)
        self.draw_len = np.full(2 * ng, -1, dtype=np.int32)
        for g, (n, _, _, ev, dl, _) in enumerate(gaps):
            self.draw_len[2 * g + (1 if ev == "p" else 0)] = dl
        self.origin = np.array([g[5] for g in gaps], dtype=np.int32)
        self.state = np.array([1 if (g[0] > 0 and g[4] == g[0] and g[5] & 1 and not g[5] & 2) else 0 for g in gaps], dtype=np.uint8)

    def evidence(self, g):
        """-> [(offset or INT_MIN, seq, is_partial, aux)] of gap g's evidence reads, in read order"""
        if self.gaps[g][3] == "p":
            return [(int(self.draw_pos[self.NU + k]), self.p_seqs[k], 1, int(self.batch.p_match[k])) for k in range(int(self.p_off[g]), int(self.p_off[g + 1]))]
        return [(int(self.draw_pos[k]), self.u_seqs[k], 0, int(self.u_rev[k])) for k in range(int(self.u_off[g]), int(self.u_off[g + 1]))]

    def expected(self):
        """the whole plane by the restatement: off gaps all zero"""
        tabs = tables(self.model.cstruct())
        LL = np.zeros((int(self.str_off[-1]), 4))
        for g in range(len(self.gaps)):
            if self.state[g]:
                reads = [(o, s, (not part) and (aux & 1)) for o, s, part, aux in self.evidence(g) if o != INT_MIN]
                LL[int(self.str_off[g]):int(self.str_off[g + 1])] = restate(int(self.filled_len[g]), reads, tabs)
        return LL

    def result(self):
        return api.FillResult(self.filled_len, np.zeros_like(self.filled_len), None, str_off=self.str_off, raw=self.raw,
                              draw=(self.draw_pos, self.draw_isz, self.draw_len))


F_, O_, T_ = api.SUP_FINAL, api.SUP_ORIGINAL, api.SUP_TIEBREAK


def hand_unmapped():
    """n = 1, 65, 257, 600, 300 with 3, 70, 130, 40, 20 evidence reads: gap 1 is switched off by ORIGINAL in its origin, gap 2 takes its
    evidence from its 130 PARTIAL reads (and carries unmapped reads it must not use), gap 4 is switched off by a draw length that is
    not n.  On: the 64-read chunk boundary twice (gap 2), the 256-column block boundary (gaps 2, 3), n = 1 (gap 0), reversed
    unmapped reads over 600 columns (gap 3)."""
    return Hand("unmapped", [(1, 3, 2, "u", 1, F_), (65, 70, 2, "u", 65, F_ | O_), (257, 4, 130, "p", 257, F_ | T_), (600, 40, 2, "u", 600, F_), (300, 20, 2, "u", 301, F_)], 20261019)


def hand_partial():
    """the partial-mode model: two gaps with 5 and 70 partial reads (one chunk boundary)"""
    return Hand("partial", [(40, 0, 5, "p", 40, F_), (300, 0, 70, "p", 300, F_ | T_)], 77)


EDGE_LENS = (1, 16, 17, 32, 33, 199)


def hand_edge_lengths():
    """One gap of 40 columns with 65 unmapped reads (one chunk boundary) of the lengths at which a staged read's layout changes: the
    2-bit word count at 16 | 17 and 32 | 33, the N-mask word count at 32 | 33, the four-lane word split at 1 (one lane) and 199
    (all twenty words); the first read of every length ends in an N."""
    return Hand("unmapped", [(40, 65, 2, "u", 40, F_)], 20261020, lens=EDGE_LENS, last_n=True)


def test_edge_length_case_is_valid():
    """Every length of the edge-length case has a drawn read that overlaps the string of its (on) gap, and a read whose last base
    is N; the restatement's plane is not trivial."""
    H = hand_edge_lengths()
    assert list(H.state) == [1]
    ev = H.evidence(0)
    assert len(ev) == 65 and {len(s) for _, s, *_ in ev} == set(EDGE_LENS)
    for ln in EDGE_LENS:
        assert any(len(s) == ln and o != INT_MIN and o < 40 and o + ln > 0 for o, s, *_ in ev), f"no drawn read of length {ln} on the string"
        assert any(len(s) == ln and s[-1] == ord("N") for _, s, *_ in ev), f"no read of length {ln} ends in N"
    LL = H.expected()
    assert LL.shape == (40, 4) and LL.any() and not np.isnan(LL).any()


def test_hand_case_is_not_vacuous():
    """The hand-made case holds what it is meant to exercise: reads left of column 0, hanging over either end, missing the string,
    undrawn, with N bases, both orientations; and terms of -inf from the zero table entries reach the expected plane."""
    H = hand_unmapped()
    assert list(H.state) == [1, 0, 1, 1, 0]
    ev = H.evidence(3)
    n = 600
    assert any(o != INT_MIN and o < 0 for o, *_ in ev) and any(o != INT_MIN and o + len(s) > n for o, s, *_ in ev)
    assert any(o == INT_MIN for o, *_ in ev) and any((s == ord("N")).sum() == 2 for _, s, *_ in ev)
    assert {aux & 1 for *_, aux in ev} == {0, 1}
    assert any(o != INT_MIN and (o >= 257 or o + len(s) <= 0) for o, s, *_ in H.evidence(2))
    LL = H.expected()
    assert np.isneginf(LL).any() and not np.isnan(LL).any() and (LL[np.isfinite(LL)] <= 0).all()
    assert not LL[int(H.str_off[1]):int(H.str_off[2])].any() and not LL[int(H.str_off[4]):].any()


# ------------------------------------------------------------------------------------- CPU
def test_quality_abi_surface():
    """The call is declared with exactly its prototype, bound and exported; fig_gap_quality is 24 bytes; fig_gap_results did not
    grow and the version did not move; the emulation library, which lacks the call, still loads -- and asking it for a quality is
    an error that names the call."""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert re.search(r"^int fig_batch_quality\(fig_ctx \*ctx, const fig_gap_results \*filled, const int32_t \*origin, fig_gap_quality \*q\);", hdr, flags=re.M)
    assert "fig_batch_quality" in api.EXPORTS
    assert hasattr(C.CDLL(util.pbuild.LIB), "fig_batch_quality")
    assert re.search(r"#define FIG_ABI_VERSION 1\b", hdr)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu %d %d %zu %zu %zu\\n",sizeof(fig_gap_quality),sizeof(fig_gap_results),'
           'FIG_QUAL_OFF,FIG_QUAL_ON,offsetof(fig_gap_quality,loglik),offsetof(fig_gap_quality,phred),offsetof(fig_gap_quality,state));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out[0] == C.sizeof(api.FigGapQuality) == 24
    assert out[1] == C.sizeof(api.FigGapResults) == 128
    assert out[2:4] == [api.QUAL_OFF, api.QUAL_ON] == [0, 1]
    assert out[4:] == [api.FigGapQuality.loglik.offset, api.FigGapQuality.phred.offset, api.FigGapQuality.state.offset] == [0, 8, 16]
    emu = api.load_library(util.EMULIB)
    assert not hasattr(emu, "fig_batch_quality") and emu.fig_version() == 1
    eng = api.Engine(0, lib_path=util.EMULIB)
    try:
        eng.n_gaps = 0
        with pytest.raises(RuntimeError, match="fig_batch_quality"):
            eng.quality(api.FillResult(np.zeros(1, np.int32), np.zeros(1, np.int32), None, str_off=np.zeros(1, np.int64)))
        with pytest.raises(RuntimeError, match="fig_batch_quality"):
            eng.fill_resident(quality=True)
    finally:
        eng.close()
    host = api.load_host_library()
    for fn in ("fighost_quality_tables", "fighost_quality_phred", "fighost_quality_gaps_on", "fighost_run_write_quality"):
        assert hasattr(host, fn), fn


def test_tables_are_log10_of_the_model():
    """lm[k] = log10(1 - e[k]), le[k] = log10(e[k]), lt[b][s] = log10(T[b*5+s]), entry by entry EQUAL to math.log10 of the same
    doubles (both are the C library's log10; `1 - e[k]` in Python is the double fig_model_tables rounds to).  e[k] = 0 and a zero
    matrix entry give -inf, not NaN."""
    m = hand_model("unmapped")
    lm, le, lt = tables(m.cstruct())
    lg = lambda v: math.log10(v) if v > 0 else NINF
    assert same_bits(lm, [lg(1 - float(x)) for x in m.e])
    assert same_bits(le, [lg(float(x)) for x in m.e])
    assert same_bits(lt, [[lg(float(m.T[b * 5 + s])) for s in range(4)] for b in range(4)])
    assert le[17] == NINF and lt[1, 2] == NINF and all(lt[b, b] == NINF for b in range(4))
    assert not np.isnan(lm).any() and not np.isnan(le).any() and not np.isnan(lt).any()
    assert np.isfinite(lm).all() and np.isneginf(le).sum() == 1 and np.isneginf(lt).sum() == 5


@pytest.mark.parametrize("ll,c,want", [
    ([0.0, -1.0, NINF, NINF], "A", 10),          # perr = 0.1 / 1.1: 10.41
    ([-5.0, -5.0, -5.0, -5.0], "G", 1),          # perr = 0.75: 1.25
    ([0.0, -1.0, NINF, NINF], "N", 0),
    ([NINF, NINF, NINF, NINF], "A", 0),
    ([0.0, NINF, NINF, NINF], "A", 93),          # perr == 0
    ([NINF, NINF, -700.0, -1100.0], "G", 93),    # perr == 0 by underflow of pow(10, -400)
    ([-3.0, 0.0, NINF, NINF], "A", 0),           # the called base is not the maximum: perr = 1 / 1.001
    ([-3.0, 0.0, NINF, NINF], "C", 30),          # perr = 0.001 / 1.001: 30.004
    ([0.0, -2.0, -2.0, -2.0], "A", 15),          # perr = 0.03 / 1.03: 15.36
    ([0.0, 0.0, 0.0, 0.0], "a", 0),              # not one of ACGT
])
def test_phred_by_hand(ll, c, want):
    """Cases far from a rounding boundary of floor(-10*log10(perr) + 0.5)."""
    assert list(phred_of([ll], np.frombuffer(c.encode(), dtype=np.uint8))) == [want]


def test_on_off_rule():
    """All eight origin masks and no origins at all, draw headers absent / equal to n / unequal to n / both set, on either side,
    n = 0 and n < 0: ON iff n > 0, exactly one header >= 0 and equal to n, and (origins given) FINAL without ORIGINAL."""
    host = api.load_host_library()
    rows = []
    for n in (0, -3, 1, 57):
        for hdr in [(-1, -1), (n, -1), (-1, n), (n + 1, -1), (-1, n - 1), (n, n), (0, -1), (-1, 0), (n, 0)]:
            for org in [None] + list(range(8)):
                rows.append((n, hdr, org))
    fl = np.array([r[0] for r in rows], dtype=np.int32)
    dl = np.array([h for r in rows for h in r[1]], dtype=np.int32)
    want = np.array([1 if (n > 0 and ((lu >= 0) != (lp >= 0)) and (lu if lu >= 0 else lp) == n and (org is None or (org & 1 and not org & 2))) else 0
                     for n, (lu, lp), org in rows], dtype=np.uint8)
    for given in (False, True):
        sel = np.array([(r[2] is not None) == given for r in rows])
        st = np.full(int(sel.sum()), 0xFF, dtype=np.uint8)
        org = np.array([r[2] or 0 for r in rows], dtype=np.int32)[sel]
        f, d = np.ascontiguousarray(fl[sel]), np.ascontiguousarray(dl.reshape(-1, 2)[sel])
        host.fighost_quality_gaps_on(len(st), api._p(f, api.c_i32_p), api._p(d, api.c_i32_p), api._p(org, api.c_i32_p) if given else None, api._p(st, api.c_u8_p))
        assert np.array_equal(st, want[sel])
    pick = lambda n, hdr, org: int(want[rows.index((n, hdr, org))])
    assert pick(57, (57, -1), None) == pick(57, (-1, 57), 1) == pick(57, (57, -1), 5) == pick(1, (1, -1), 1) == 1
    assert pick(57, (57, -1), 0) == pick(57, (57, -1), 2) == pick(57, (57, -1), 3) == pick(57, (57, -1), 4) == pick(57, (57, -1), 7) == 0
    assert pick(57, (-1, -1), 1) == pick(57, (58, -1), 1) == pick(57, (57, 57), 1) == pick(57, (57, 0), None) == pick(0, (0, -1), 1) == 0


def test_quality_writer_format(tmp_path):
    """fighost_run_write_quality on hand-made arrays: `g contig start G0 n state Q`, Q = n characters of Phred+33, empty for n <= 0."""
    root = util.extract_golden("partial_small", str(tmp_path))
    exp = _gapout(root)
    assert len(exp) == 3
    host, h = _open_run(root)
    fl = np.array([4, 0, 2], dtype=np.int32)
    off = np.array([0, 4, 4, 6], dtype=np.int64)
    ph = np.array([0, 10, 93, 41, 7, 60], dtype=np.uint8)
    st = np.array([1, 0, 1], dtype=np.uint8)
    err = C.create_string_buffer(512)
    cwd = os.getcwd(); os.chdir(root)
    try:
        rc = host.fighost_run_write_quality(h, api._p(fl, api.c_i32_p), api._p(off, api.c_i64_p), api._p(ph, api.c_u8_p), api._p(st, api.c_u8_p), err, 512)
    finally:
        os.chdir(cwd)
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    head = ["\t".join(e[:4]) for e in exp]
    want = f"{head[0]}\t4\t1\t!+~J\n{head[1]}\t0\t0\t\n{head[2]}\t2\t1\t(]\n"
    assert util.read(os.path.join(root, "tmp", "gapquality.txt")) == want
    assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))


def test_kernel_arithmetic_on_the_cpu(tmp_path):
    """The function fig_quality_kernel calls per (column, read) pair, compiled as plain C++ into a program of its own with
    AddressSanitizer and UBSan (tests/quality_column_main.cpp; run directly), over the on-gaps of the hand-made case: the plane it
    prints equals the numpy restatement bit for bit."""
    H = hand_unmapped()
    exe = str(tmp_path / "quality_column")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "quality_column_main.cpp")])
    on = [g for g in range(len(H.gaps)) if H.state[g]]
    lines = ["200", " ".join(float(v).hex() for v in H.model.e), " ".join(float(v).hex() for v in H.model.T), str(len(on))]
    for g in on:
        ev = H.evidence(g)
        lines.append(f"{int(H.filled_len[g])} {len(ev)}")
        lines += [f"{o} {len(s)} {part} {aux} {s.tobytes().decode()}" for o, s, part, aux in ev]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([int(t, 16) for t in r.stdout.split()], dtype=np.uint64).view(np.float64).reshape(-1, 4)
    LL = H.expected()
    want = np.concatenate([LL[int(H.str_off[g]):int(H.str_off[g + 1])] for g in on])
    assert len(got) == 1 + 257 + 600 and same_bits(got, want)


def test_edge_lengths_on_the_cpu(tmp_path):
    """The edge-length case through the same stand-alone program (tests/quality_column_main.cpp, AddressSanitizer and UBSan): the
    plane equals the numpy restatement bit for bit."""
    H = hand_edge_lengths()
    exe = str(tmp_path / "quality_column")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "quality_column_main.cpp")])
    ev = H.evidence(0)
    lines = ["200", " ".join(float(v).hex() for v in H.model.e), " ".join(float(v).hex() for v in H.model.T), "1", f"40 {len(ev)}"]
    lines += [f"{o} {len(s)} {part} {aux} {s.tobytes().decode()}" for o, s, part, aux in ev]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([int(t, 16) for t in r.stdout.split()], dtype=np.uint64).view(np.float64).reshape(-1, 4)
    assert same_bits(got, H.expected())


def test_figfill_on_a_library_without_the_call_fails_loudly(tmp_path):
    """FIGFILL_QUALITY=1 with the emulation behind figfill: a non-zero exit that names the missing call, and no gapquality.txt."""
    root = util.extract_golden("partial_small", str(tmp_path))
    r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, {"FIGFILL_QUALITY": "1"})
    assert r.returncode != 0 and "fig_batch_quality" in r.stderr
    assert not os.path.exists(os.path.join(root, "tmp", "gapquality.txt"))


# ------------------------------------------------------------------------------------- GPU
def _quality_raw(eng, H, origin):
    """fig_batch_quality through ctypes with the caller's buffers filled with 0xFF bytes before the call"""
    r = api.FigGapResults()
    r.filled_len = api._p(H.filled_len, api.c_i32_p); r.str_off = api._p(H.str_off, api.c_i64_p)
    r.str = C.cast(H.raw.ctypes.data, C.c_char_p); r.str_capacity = len(H.raw)
    r.draw_pos = api._p(H.draw_pos, api.c_i32_p); r.draw_isz = api._p(H.draw_isz, api.c_i32_p); r.draw_len = api._p(H.draw_len, api.c_i32_p)
    total = int(H.str_off[-1])
    ll = np.zeros((total, 4)); ll.view(np.uint8)[...] = 0xFF
    ph = np.full(total, 0xFF, dtype=np.uint8); st = np.full(len(H.gaps), 0xFF, dtype=np.uint8)
    q = api.FigGapQuality(); q.loglik = api._p(ll, api.c_double_p); q.phred = api._p(ph, api.c_u8_p); q.state = api._p(st, api.c_u8_p)
    rc = eng.lib.fig_batch_quality(eng.ctx, C.byref(r), api._p(origin, api.c_i32_p) if origin is not None else None, C.byref(q))
    return rc, ll, ph, st


def _check_hand(H):
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        rc, ll, ph, st = _quality_raw(eng, H, H.origin)
        assert rc == 0
        LL = H.expected()
        assert list(st) == list(H.state)
        assert same_bits(ll, LL), f"columns {np.flatnonzero((ll.view(np.int64) != LL.view(np.int64)).any(axis=1))[:8]} differ"
        on_col = np.repeat(H.state.astype(bool), H.filled_len)
        assert np.array_equal(ph, np.where(on_col, phred_of(ll, H.raw[:len(ll)]), 0))       # (a gap that is off has Phred 0 by definition)
        for g in range(len(H.gaps)):
            a, b = int(H.str_off[g]), int(H.str_off[g + 1])
            if not H.state[g]:
                assert not ll[a:b].any() and not ph[a:b].any(), f"gap {g} is off"
            else:
                assert (ph[a:b] <= 93).all() and not ph[a:b][H.raw[a:b] == ord("N")].any()
        # the Python face gives the same arrays
        ll2, ph2, st2 = eng.quality(H.result(), H.origin)
        assert same_bits(ll2, ll) and np.array_equal(ph2, ph) and np.array_equal(st2, st)
        # no origins: the ORIGINAL gap is on as well, the others are unchanged
        rc, ll3, _, st3 = _quality_raw(eng, H, None)
        assert rc == 0 and list(st3) == [1 if (g[0] > 0 and g[4] == g[0]) else 0 for g in H.gaps]
        same = np.repeat(st3 == st, H.filled_len)
        assert same_bits(ll3[same], ll[same])
        eng.free_batch()
        assert _quality_raw(eng, H, H.origin)[0] == -1                # no resident batch
    finally:
        eng.close()
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_hand_made_placements_unmapped_model():
    """fig_batch_quality on a resident hand-made batch and hand-made placements (hand_unmapped), no fill: the plane equals the
    restatement bit for bit, Phred is fighost_quality_phred of that plane and string, states are as configured, off gaps are all
    zero although the buffers came in as 0xFF bytes."""
    _check_hand(hand_unmapped())


@pytest.mark.gpu
def test_hand_made_placements_partial_model():
    """The same in a partial-mode model (gap_ot_preset given, so the upload probes nothing): 5 and 70 partial reads."""
    _check_hand(hand_partial())


@pytest.mark.gpu
def test_edge_lengths_on_the_device():
    """fig_batch_quality on the edge-length case (read lengths 1, 16, 17, 32, 33, 199; 65 reads; 40 columns): bit for bit the
    restatement, and everything else test_hand_made_placements_unmapped_model asks of a hand-made case."""
    _check_hand(hand_edge_lengths())


@pytest.mark.gpu
def test_offset_out_of_bounds_is_refused():
    """A drawn offset with |o| >= 2^20 in a gap that is on is FIG_EINVAL, on either side; in a gap that is off it is not looked at."""
    H = hand_partial()
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        for v in (1 << 20, -(1 << 20)):
            B = hand_partial()
            B.draw_pos[3] = v
            assert _quality_raw(eng, B, B.origin)[0] == -1
        B = hand_partial()
        B.draw_pos[3] = (1 << 20) - 1
        assert _quality_raw(eng, B, B.origin)[0] == 0
        B = hand_partial()
        B.draw_pos[3] = 1 << 20; B.origin[0] = api.SUP_ORIGINAL
        rc, ll, _, st = _quality_raw(eng, B, B.origin)
        assert rc == 0 and list(st) == [0, 1] and not ll[:40].any()
    finally:
        eng.close()


def run_golden_quality(root, keep=False):
    """test_base_support.run_golden with the quality on top: fill with draw and support planes, then Engine.quality with the
    returned origins while the batch is resident.  keep=True: a second plain fill of the still resident batch as well.
    -> Fill with .loglik / .phred / .state / .u_rev (and .second)"""
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        ids = np.arange(max(n, 1), dtype=np.int64)
        cm = api.FigModel(); host.fighost_run_model(h, C.byref(cm))
        cb = api.FigGapBatch(); su = C.c_int64(); sp = C.c_int64()
        assert host.fighost_run_shard(h, api._p(ids, api.c_i64_p), n, C.byref(cb), C.byref(su), C.byref(sp)) == 0
        F = Fill()
        F.G0 = np.ctypeslib.as_array(cb.gap_len, shape=(n,)).copy()
        F.u_off = np.ctypeslib.as_array(cb.u_read_off, shape=(n + 1,)).copy()
        F.p_off = np.ctypeslib.as_array(cb.p_read_off, shape=(n + 1,)).copy()
        F.u_seq_off = np.ctypeslib.as_array(cb.u_seq_off, shape=(int(su.value) + 1,)).copy() if su.value else np.zeros(1, dtype=np.int64)
        F.p_seq_off = np.ctypeslib.as_array(cb.p_seq_off, shape=(int(sp.value) + 1,)).copy() if sp.value else np.zeros(1, dtype=np.int64)
        F.u_seq = np.frombuffer(cb.u_seq or b"", dtype=np.uint8)
        F.p_seq = np.frombuffer(cb.p_seq or b"", dtype=np.uint8)
        F.u_rev = np.ctypeslib.as_array(cb.u_is_reverse, shape=(int(su.value),)).copy() if su.value else np.zeros(0, dtype=np.uint8)
        F.unmapped = bool(cm.unmapped_flag)
        F.tabs = tables(cm)
        eng = api.Engine(0)
        try:
            eng.set_model_struct(cm)
            eng.upload_struct(cb)
            reach = np.zeros(max(n, 1), dtype=np.uint8); reach[:n] = eng.probe_reach()
            preset = np.zeros(max(n, 1), dtype=np.uint8)
            host.fighost_run_ot_presets(h, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
            eng.set_ot_preset(preset[:n])
            res = eng.fill_struct(cb, int(su.value), int(sp.value), draw=True, resident=True, support=True, quality=True, keep_resident=keep)
            if keep:
                F.second = _take(Fill(), eng.fill_struct(cb, int(su.value), int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.loglik, F.phred, F.state = res.quality
        return F
    finally:
        host.fighost_run_close(h)


def drawn_reads(F, g):
    """-> (draw length, [(offset, read, reversed)] of the drawn reads of gap g in read order) or (None, [])"""
    lu, lp = int(F.draw_len[2 * g]), int(F.draw_len[2 * g + 1])
    if lu >= 0:
        ks = range(int(F.u_off[g]), int(F.u_off[g + 1]))
        return lu, [(int(F.draw_pos[k]), F.u_seq[F.u_seq_off[k]:F.u_seq_off[k + 1]], bool(F.u_rev[k])) for k in ks if F.draw_pos[k] != INT_MIN]
    if lp >= 0:
        nu = int(F.u_off[-1])
        ks = range(int(F.p_off[g]), int(F.p_off[g + 1]))
        return lp, [(int(F.draw_pos[nu + k]), F.p_seq[F.p_seq_off[k]:F.p_seq_off[k + 1]], False) for k in ks if F.draw_pos[nu + k] != INT_MIN]
    return None, []


def check_golden_quality(F):
    """every gap of a filled golden: state by the rule, plane by the restatement, Phred by the host function; -> gaps that are on"""
    assert (np.diff(F.u_off) <= 3000).all() and (np.diff(F.p_off) <= 3001).all()      # (no read cap: batch index = draw-plane index)
    total = int(F.str_off[F.n])
    assert F.loglik.shape == (total, 4) and F.phred.shape == (total,) and F.state.shape == (F.n,)
    on = []
    for g in range(F.n):
        n = int(F.filled_len[g])
        a, b = int(F.str_off[g]), int(F.str_off[g + 1])
        dl, reads = drawn_reads(F, g)
        org = int(F.origin[g])
        want_on = n > 0 and dl == n and bool(org & api.SUP_FINAL) and not org & api.SUP_ORIGINAL
        assert int(F.state[g]) == int(want_on), f"gap {g}"
        if not want_on:
            assert not F.loglik[a:b].any() and not F.phred[a:b].any(), f"gap {g} is off"
            continue
        on.append(g)
        assert same_bits(F.loglik[a:b], restate(n, reads, F.tabs)), f"gap {g}: plane differs from the restatement over {len(reads)} drawn reads"
        s = F.raw[a:b]
        assert np.array_equal(F.phred[a:b], phred_of(F.loglik[a:b], s))
        assert (F.phred[a:b] <= 93).all() and not F.phred[a:b][s == ord("N")].any()
    return on


@pytest.fixture(scope="module")
def qfills(tmp_path_factory):
    """name -> golden filled with the draw, support and quality planes; computed once per module, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden_quality(util.extract_golden(name, str(tmp_path_factory.mktemp(name))), keep=(name == "unmapped_small"))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "partial_brackets", "bench_b160"])
def test_goldens_end_to_end(name, qfills):
    """A golden filled as figfill fills it, then Engine.quality with the returned origins: per gap the state follows the rule, the
    plane equals the restatement over the drawn reads bit for bit (reverse bits from the shard view's u_is_reverse), every called
    base of an on-gap has a Phred in 0..93 and every N has 0."""
    F = qfills(name)
    on = check_golden_quality(F)
    if name == "bench_b160":            # what tests/test_base_support.py pins of this gap
        assert 0 in on and int(F.filled_len[0]) == 305 and len(drawn_reads(F, 0)[1]) == 657 and F.unmapped
        called = F.raw[:305] != ord("N")
        assert called.any() and F.phred[:305][called].max() > 0
    if name == "unmapped_small":
        assert on, "an unmapped-mode golden without a gap that is on"


@pytest.mark.gpu
def test_a_partial_mode_gap_is_on(qfills):
    """Against vacuity: across partial_brackets and the other partial-mode goldens at least one gap is on (and then compared exactly)."""
    from test_base_support import GPU_GOLDENS
    names = ["partial_brackets"] + [n for n in GPU_GOLDENS if n != "partial_brackets" and n.startswith("partial")]
    for name in names:
        F = qfills(name)
        if not F.unmapped and check_golden_quality(F):
            return
    pytest.fail(f"no partial-mode gap is on in {names}")


@pytest.mark.gpu
def test_off_means_off(qfills, tmp_path):
    """unmapped_small: lengths, strings, gaptofill, the draw planes and the support plane of a fill are identical with and without a
    following fig_batch_quality, and a second fill of the still resident batch after the quality call returns the same bytes."""
    from test_base_support import run_golden
    on = qfills("unmapped_small")
    off = run_golden(util.extract_golden("unmapped_small", str(tmp_path)), support=True)
    for other in (off, on.second):
        for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
            assert np.array_equal(getattr(on, f), getattr(other, f)), f


@pytest.mark.gpu
def test_gapquality_file_is_the_same_from_every_host_path(tmp_path, monkeypatch):
    """threads3 with FIGFILL_QUALITY=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 and two-rank figfill_mp leave the same
    gapquality.txt (8 lines, the first five fields gapout.txt's, n characters each, at least one gap on), the reference's files stay
    byte-identical in every run, gapsupport.txt appears in none of them; without the variable neither file appears."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    monkeypatch.delenv("FIGFILL_SUPPORT", raising=False)
    monkeypatch.delenv("FIGFILL_QUALITY", raising=False)
    roots = [util.extract_golden("threads3", str(tmp_path / f"r{k}")) for k in range(4)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    r = util.run([util.FIGFILL] + argv, roots[3])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(os.path.join(roots[3], "tmp", "gapquality.txt")) and not os.path.exists(os.path.join(roots[3], "tmp", "gapsupport.txt"))
    r = util.run([util.FIGFILL] + argv, roots[0], {"FIGFILL_QUALITY": "1"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[1], {"FIGFILL_QUALITY": "1", "FIGFILL_DEVICES": "0,0"})
    assert r.returncode == 0, r.stderr
    monkeypatch.setenv("FIGFILL_QUALITY", "1")                              # the spawned ranks inherit it
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_mp_worker, args=(k, 2, port, roots[2], "threads3", q, None)) for k in range(2)]
    for p in ps:
        p.start()
    outs = [q.get(timeout=600) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(rc == 0 for _, rc in outs)
    files = [util.read(os.path.join(root, "tmp", "gapquality.txt")) for root in roots[:3]]
    assert files[0] == files[1] == files[2]
    lines = files[0].splitlines()
    exp = _gapout(roots[0])
    assert len(lines) == len(exp) == 8
    for ln, e in zip(lines, exp):
        f = ln.split("\t")
        assert len(f) == 7 and f[:5] == e[:5] and f[5] in ("0", "1")
        assert len(f[6]) == max(int(f[4]), 0) and all(33 <= ord(c) <= 33 + 93 for c in f[6])
        if f[5] == "0":
            assert set(f[6]) <= {"!"}
    assert any(ln.split("\t")[5] == "1" for ln in lines)
    for root in roots:
        assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
