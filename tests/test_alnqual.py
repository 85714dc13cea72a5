"""Per-base quality over gapped read alignments (fig_batch_alnqual, include/figbird_hip.h: fig_gap_alnqual).

The restatement below is numpy and independent of fig_alnqual_host.h: test_indel_evidence's band for H and the back-pointers, the
steps of a read's path listed from the end by a loop of its own and replayed forwards into the planes read by read, and
test_base_quality's Phred.  Doubles of the device are compared with it on their int64 view and everything else for equality: the
device only adds table entries in a fixed order and compares.
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
import test_indel_evidence as tie
import test_polish as tpo
import test_recruit as tre
from test_base_support import CODE, INT_MIN, Fill, _gapout, _open_run, _take

NINF = -math.inf
W = 7
NONE = 15
F_, O_ = api.SUP_FINAL, api.SUP_ORIGINAL
ACGT = tie.ACGT
PAD = tie.PAD
_Eng = tpo._Eng


# ------------------------------------------------------------------------------------- the restatement
def steps_of(BP, ln, d_end):
    """the raw steps of the path from (ln, d_end) along the back-pointers, FIRST step first: (kind, i, d) of the cell a step ends in,
    kind 0 DIAG, 1 INS, 2 DEL -> (steps, d_start)"""
    out = []
    i, d = ln, d_end
    while i > 0:
        p = int(BP[i, d + W])
        out.append((p, i, d))
        if p == 0:
            i -= 1
        elif p == 1:
            i -= 1; d += 1
        else:
            d -= 1
        assert -W <= d <= W
    return out[::-1], d


def flat_steps(ln):
    return [(0, i, 0) for i in range(1, ln + 1)], 0


def map_of(steps, ln):
    """the column map of a path: per window column c = x - (o* - 7), 0 <= c < ln + 14, d + 7 of the DIAG step that lands on it, or 15"""
    m = [NONE] * (ln + 2 * W)
    for kind, i, d in steps:
        if kind == 0:
            c = i - 1 + d + W
            assert m[c] == NONE                                  # DIAG steps visit strictly increasing columns
            m[c] = d + W
    return m


def replay(steps, seq, rev, o, n, emitted, tabs, LL, depth, agree, skip):
    """one read's steps, forwards, into the planes of its gap"""
    lm, le, lt = tabs[:3]
    ln = len(seq)
    code = CODE[seq]
    n_ins = n_del = 0
    for kind, i, d in steps:
        if kind == 1:
            n_ins += 1
        elif kind == 2:
            n_del += 1
            x = o + i + d - 1
            if 0 <= x < n:
                skip[x] += 1
        else:
            j = i - 1
            x = o + j + d
            s = int(code[j])
            if not 0 <= x < n or s > 3:
                continue
            k = ln - 1 - j if rev else j
            for b in range(4):
                LL[x, b] = LL[x, b] + (lm[k] if s == b else le[k] + lt[b, s])
            depth[x] += 1
            agree[x] += int(emitted[x] == ACGT[s])
    return n_ins, n_del


def restate_gap(S, n, emitted, reads, tabs):
    """reads: [(seq, rev, ostar)] of the aligned reads of a gap in read order -> per-read dicts (with `map` and `span`) and the planes"""
    LL = np.zeros((n, 4)); depth = np.zeros(n, np.int32); agree = np.zeros(n, np.int32); skip = np.zeros(n, np.int32)
    out = []
    if not reads:
        return out, LL, depth, agree, skip
    H, BP, _ = tie.band(S, reads, tabs)
    with np.errstate(invalid="raise"):
        for a, (seq, rev, o) in enumerate(reads):
            ln = len(seq)
            best, d_end = NINF, 0
            for dd in tie.END_ORDER:
                if H[a, dd + W] > best:
                    best, d_end = float(H[a, dd + W]), dd
            steps, d_start = steps_of(BP[a], ln, d_end) if best > NINF else flat_steps(ln)
            n_ins, n_del = replay(steps, seq, rev, o, n, emitted, tabs, LL, depth, agree, skip)
            out.append(dict(ll_gapped=best, n_ins=n_ins, n_del=n_del, d_end=d_end, d_start=d_start, map=map_of(steps, ln), span=(o + d_start, o + ln - 1 + d_end)))
    return out, LL, depth, agree, skip


def _geometry(H, g):
    if hasattr(H, "geometry"):
        return H.geometry(g)
    return H.contig, int(H.starts[g]), trp.G0


def expected(H, tabs=None, state=None, gaps=None):
    """The restatement of a whole case (a trp.HandPlace, a tie.Case or a golden's view) -> dict of the arrays of fig_gap_alnqual, plus
    `aligned` [NU], `maps` and `spans` (per read, None for an unaligned one).  gaps: restate these gaps only."""
    tabs = tabs or tie.indel_tables(H.model.cstruct())
    state = H.state if state is None else state
    NU, ng = H.NU, len(H.filled_len)
    total = int(H.str_off[ng])
    w = dict(loglik=np.zeros((total, 4)), depth=np.zeros(total, np.int32), agree=np.zeros(total, np.int32), skip=np.zeros(total, np.int32),
             phred=np.zeros(total, np.uint8), ll_gapped=np.zeros(NU), n_ins=np.zeros(NU, np.int32), n_del=np.zeros(NU, np.int32), d_end=np.zeros(NU, np.int32),
             d_start=np.full(NU, INT_MIN, np.int32), state=np.asarray(state, dtype=np.uint8), aligned=np.zeros(NU, bool), maps=[None] * NU, spans=[None] * NU)
    for g in (range(ng) if gaps is None else gaps):
        if not state[g]:
            continue
        n = int(H.filled_len[g])
        ks = [k for k in range(int(H.u_off[g]), int(H.u_off[g + 1])) if tie.is_aligned(int(H.draw_pos[k]), len(H.seqs[k]), n)]
        a, b = int(H.str_off[g]), int(H.str_off[g]) + n
        contig, start, G0 = _geometry(H, g)
        S = tie.columns(contig, start, G0, H.raw[a:b])
        rs, LL, dp, ag, sk = restate_gap(S, n, H.raw[a:b], [(H.seqs[k], int(H.rev[k]), int(H.draw_pos[k])) for k in ks], tabs)
        for k, r in zip(ks, rs):
            w["aligned"][k] = True
            for f in ("ll_gapped", "n_ins", "n_del", "d_end", "d_start"):
                w[f][k] = r[f]
            w["maps"][k] = r["map"]; w["spans"][k] = r["span"]
        w["loglik"][a:b] = LL; w["depth"][a:b] = dp; w["agree"][a:b] = ag; w["skip"][a:b] = sk
        w["phred"][a:b] = tbq.phred_of(LL, H.raw[a:b])
    return w


FIELDS_D = ("loglik", "ll_gapped")
FIELDS_I = ("depth", "agree", "skip", "phred", "n_ins", "n_del", "d_end", "d_start", "state")
PLANES = ("loglik", "depth", "agree", "skip", "phred")


def compare(A, want, H=None, gaps=None):
    """every array of the device against the restatement's: doubles on their int64 view, everything else equal.  gaps (with H): the
    planes and the per-read arrays of these gaps only"""
    cols = reads = None
    if gaps is not None:
        cols = np.zeros(len(want["depth"]), bool); reads = np.zeros(len(want["ll_gapped"]), bool)
        for g in gaps:
            cols[int(H.str_off[g]):int(H.str_off[g + 1])] = True; reads[int(H.u_off[g]):int(H.u_off[g + 1])] = True
    for f in FIELDS_D + FIELDS_I:
        got, wt = np.asarray(getattr(A, f)), np.asarray(want[f])
        assert got.shape == wt.shape, f
        if gaps is not None and f != "state":
            m = cols if f in PLANES else reads
            got, wt = got[m], wt[m]
        if f in FIELDS_D:
            got, wt = np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(wt).view(np.int64)
        bad = np.argwhere(got != wt)
        assert not len(bad), f"{f}: elements {bad[:8].tolist()}: got {got[tuple(bad[0])]}, want {wt[tuple(bad[0])]}"


def gap_planes(H, A, g):
    a, b = int(H.str_off[g]), int(H.str_off[g + 1])
    get = (lambda f: A[f]) if isinstance(A, dict) else (lambda f: getattr(A, f))
    return {f: np.asarray(get(f))[a:b] for f in PLANES}


def ungapped(H, g, tabs=None):
    """tbq.restate of gap g: the ungapped quality of the same input -> (loglik [n, 4], phred [n])"""
    tabs = tabs or tbq.tables(H.model.cstruct())
    n = int(H.filled_len[g]); a = int(H.str_off[g])
    reads = [(int(H.draw_pos[k]), H.seqs[k], int(H.rev[k])) for k in range(int(H.u_off[g]), int(H.u_off[g + 1])) if H.draw_pos[k] != INT_MIN]
    LL = tbq.restate(n, reads, tabs)
    return LL, tbq.phred_of(LL, H.raw[a:a + n])


# ------------------------------------------------------------------------------------- hand-made cases
@pytest.fixture(scope="module")
def planted():
    H = tie.planted_case()
    return H, expected(H)


def ins_model():
    """tie.clean_model() whose insertion rate is 1e-4 at the read bases 30, 31 and 32 and 1e-30 everywhere else: a forward read with
    three bases too many there can only insert exactly those three, whatever they are"""
    m = tie.clean_model()
    m.ins = np.full(len(m.e), 1e-30); m.ins[30:33] = 1e-4
    return m


def nins_case():
    """One gap of 100 columns and one forward read drawn at 10: 30 bases of the string, then G N T, then 30 more bases of the string.
    The N base lies inside the INS run."""
    rng = np.random.default_rng(20261025)
    s = rng.choice(ACGT, size=100).copy()
    rd = np.concatenate([s[10:40], np.frombuffer(b"GNT", dtype=np.uint8), s[40:70]])
    return tie.Case([dict(string=s, reads=[(rd, 0, 10)])], ins_model())


BLOCK_NS = (1, 255, 256, 257, 513)


def _copy(rng, full, lo, t, ln, sub=0.01):
    """ln bases of `full` (element x - lo is column x) from column t on, with substitutions"""
    return tie.mutate(rng, full[t - lo:t - lo + ln], sub)


def steps_case():
    """The shapes of the step rules, under tie.clean_model(), every read forward unless said otherwise and copied from the gap's own
    columns (flanks of 300 random bases either side):
      gap 0, n = 90   a read over columns -30 .. 39 that lacks column 0; one over 50 .. 119 that lacks column 89 = n - 1; one over
                      50 .. 119 with two bases too many before column 90 = n (an INS run whose next column is n); a read with an N base on
                      column 20; two reads over column 60, one of which lacks it, and a reverse read that lacks it too
      gaps 1 .. 5     n = 1, 255, 256, 257, 513: reads across the ends of every column block, some with a base removed or added, and for
                      n >= 255 a read drawn at n - 1, one at n (unaligned), one at -(len - 1) and one at -len (unaligned)
      gap 6, n = 80   65 reads of which the first 64 are undrawn: a chunk with no aligned read before one with one
    """
    rng = np.random.default_rng(20261026)
    gaps = []
    left = rng.choice(ACGT, size=300); right = rng.choice(ACGT, size=300)
    s = rng.choice(ACGT, size=90).copy()
    s[0:2] = np.frombuffer(b"GA", dtype=np.uint8); left[-1] = ord("C")                     # column 0 differs from both neighbours
    s[87:90] = np.frombuffer(b"CAG", dtype=np.uint8); right[0] = ord("T")
    s[59:62] = np.frombuffer(b"CAG", dtype=np.uint8)
    full = np.concatenate([left, s, right]); lo = -300
    col = lambda a, b: full[a - lo:b - lo].copy()
    extra = np.frombuffer(b"AA", dtype=np.uint8) if s[89] != ord("A") and right[0] != ord("A") else np.frombuffer(b"CC", dtype=np.uint8)
    withn = col(5, 65); withn[15] = ord("N")
    reads = [(np.concatenate([col(-30, 0), col(1, 40)]), 0, -30), (np.concatenate([col(50, 89), col(90, 120)]), 0, 50),
             (np.concatenate([col(50, 90), extra, col(90, 120)]), 0, 50), (withn, 0, 5), (col(30, 95), 0, 30),
             (np.concatenate([col(30, 60), col(61, 96)]), 0, 30), (np.concatenate([col(25, 60), col(61, 99)]), 1, 25)]
    gaps.append(dict(string=s, reads=reads, left=left, right=right))
    for n in BLOCK_NS:
        left = rng.choice(ACGT, size=300); right = rng.choice(ACGT, size=300)
        s = rng.choice(ACGT, size=n).copy()
        full = np.concatenate([left, s, right])
        reads = []
        for e, ln in ((0, 40), (n, 33)) + tuple((b, 64) for b in range(256, n + 1, 256)):  # reads centred on the ends and the block edges
            for kind in range(3):
                t = e - ln // 2 + kind
                q = _copy(rng, full, -300, t, ln + 1)
                q = np.delete(q, ln // 3) if kind == 1 else np.insert(q, ln // 3, ACGT[kind])[:ln + 1] if kind == 2 else q
                reads.append((q[:ln], kind & 1, t))
        if n >= 255:
            for o, ln in ((n - 1, 31), (n, 31), (-30, 31), (-31, 31)):
                reads.append((_copy(rng, full, -300, o, ln), 0, o))
        gaps.append(dict(string=s, reads=reads, left=left, right=right))
    left = rng.choice(ACGT, size=300); right = rng.choice(ACGT, size=300)
    s = rng.choice(ACGT, size=80).copy()
    full = np.concatenate([left, s, right])
    reads = [(_copy(rng, full, -300, int(rng.integers(-20, 60)), 50), r & 1, INT_MIN) for r in range(64)] + [(_copy(rng, full, -300, 10, 50), 0, 10)]
    gaps.append(dict(string=s, reads=reads, left=left, right=right))
    return tie.Case(gaps, tie.clean_model(), seed=7)


@pytest.fixture(scope="module")
def stepsc():
    H = steps_case()
    return H, expected(H)


@pytest.fixture(scope="module")
def edges():
    H = tie.edge_case()
    return H, expected(H)


# ------------------------------------------------------------------------------------- CPU
def test_step_rules_by_hand():
    """A path with one INS run and one DEL run, written down by hand as back-pointers: which base lands on which column, which columns
    are skipped, the map's nibbles at the window columns 0 and len + 13, the span at both ends; a -inf read takes the flat path; the
    host library packs, unpacks and spans as the restatement does."""
    host = api.load_host_library()
    ln, o = 10, 100
    BP = np.zeros((ln + 1, 15), dtype=np.int8)
    # from (10, +7): bases 9 .. 7 on d = +7; DEL DEL at row 7 (d 7 -> 5); bases 6 .. 4 on d = +5; INS of bases 3 and 2 (d 5 -> 7); bases 1, 0 on d = +7
    BP[7, 7 + W] = 2; BP[7, 6 + W] = 2
    BP[4, 5 + W] = 1; BP[3, 6 + W] = 1
    steps, d_start = steps_of(BP, ln, 7)
    assert d_start == 7 and [k for k, _, _ in steps] == [0, 0, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0]
    m = map_of(steps, ln)
    base_on = {o - W + c: c - v for c, v in enumerate(m) if v != NONE}                    # column -> base j = c - nibble
    assert base_on == {107: 0, 108: 1, 109: 4, 110: 5, 111: 6, 114: 7, 115: 8, 116: 9}
    LL = np.zeros((400, 4)); dp = np.zeros(400, np.int32); ag = np.zeros(400, np.int32); sk = np.zeros(400, np.int32)
    tabs = tie.indel_tables(tie.clean_model().cstruct())
    seq = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    assert replay(steps, seq, 0, o, 400, np.full(400, ord("A"), np.uint8), tabs, LL, dp, ag, sk) == (2, 2)
    assert list(np.flatnonzero(sk)) == [112, 113] and list(np.flatnonzero(dp)) == sorted(base_on) and list(np.flatnonzero(ag)) == [107, 109, 115]          # bases 0, 4 and 8 are A
    assert m[ln + 13] == 14 and m[0] == NONE and (o + d_start, o + ln - 1 + 7) == (107, 116)
    # the other corner: everything on d = -7 lands base 0 on window column 0
    steps2, ds2 = steps_of(np.zeros((ln + 1, 15), dtype=np.int8), ln, -7)
    m2 = map_of(steps2, ln)
    assert ds2 == -7 and m2[0] == 0 and m2[ln - 1] == 0 and m2[ln] == NONE and m2[ln + 13] == NONE
    # the host library: nibble c in the low half of byte c / 2 for even c; bytes in use; span; flat path
    for mm in (m, m2):
        buf = np.full(108, 0xFF, dtype=np.uint8)
        for c, v in enumerate(mm):
            host.fighost_alnqual_set_nibble(api._p(buf, api.c_u8_p), c, v)
        assert [host.fighost_alnqual_nibble(api._p(buf, api.c_u8_p), c) for c in range(ln + 14)] == mm
        assert list(buf[:12]) == [mm[2 * i] | (mm[2 * i + 1] << 4) for i in range(12)] and (buf[12:] == 0xFF).all()
    assert host.fighost_alnqual_map_bytes(ln) == 12 and host.fighost_alnqual_map_bytes(200) == 107 and host.fighost_alnqual_map_bytes(1) == 8
    sp = np.zeros(2, np.int32)
    host.fighost_alnqual_span(o, ln, 7, 7, api._p(sp, api.c_i32_p)); assert list(sp) == [107, 116]
    host.fighost_alnqual_span(-9, ln, -7, -7, api._p(sp, api.c_i32_p)); assert list(sp) == [-16, -7]
    buf = np.full(108, 0xFF, dtype=np.uint8); o4 = np.full(4, -1, np.int32)
    host.fighost_alnqual_flat(api._p(buf, api.c_u8_p), ln, api._p(o4, api.c_i32_p))
    fs, fd = flat_steps(ln)
    assert list(o4) == [0, 0, 0, 0] and fd == 0 and [host.fighost_alnqual_nibble(api._p(buf, api.c_u8_p), c) for c in range(ln + 14)] == map_of(fs, ln) == [NONE] * 7 + [7] * ln + [NONE] * 7
    # the on rule is the indel pass's
    fl = np.array([5, 5, 0, 5], np.int32); dl = np.array([5, -1, 5, -1, 0, -1, 4, -1], np.int32); org = np.array([F_, F_ | O_, F_, F_], np.int32)
    st = np.full(4, 0xFF, np.uint8); st2 = np.full(4, 0xFF, np.uint8)
    host.fighost_alnqual_gaps_on(1, 4, api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p), api._p(st, api.c_u8_p))
    host.fighost_indel_gaps_on(1, 4, api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p), api._p(st2, api.c_u8_p))
    assert list(st) == list(st2) == [1, 0, 0, 0]
    host.fighost_alnqual_gaps_on(0, 4, api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), None, api._p(st, api.c_u8_p))
    assert list(st) == [0, 0, 0, 0]


def test_abi_surface():
    """the header declares the call and the struct, the version stays 1, the Python struct has the header's eleven pointers, and the
    library exports the call"""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert "#define FIG_ABI_VERSION 1" in hdr and "int fig_batch_alnqual(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, fig_gap_alnqual *out);" in hdr
    body = hdr[hdr.index("typedef struct fig_gap_alnqual {"):hdr.index("} fig_gap_alnqual;")]
    names = [ln.split(";")[0].split("*")[-1].strip() for ln in body.splitlines()[1:] if "*" in ln.split("/*")[0]]
    assert names == [f for f, _ in api.FigGapAlnqual._fields_] and len(names) == 11
    assert "fig_batch_alnqual" in api.EXPORTS and "alnqual" in api.FillResult.__dataclass_fields__ and (api.ALNQ_OFF, api.ALNQ_ON) == (0, 1)
    nm = subprocess.run(["nm", "-D", "--defined-only", util.pbuild.LIB], capture_output=True, text=True, check=True).stdout
    assert " T fig_batch_alnqual" in nm and " T fig_batch_indel" in nm


def test_alnquality_writer_format(tmp_path):
    """fighost_run_write_alnquality on hand-made arrays: `g contig start G0 n state Q`, n the length that was scored (not the filled
    length of gapout.txt), Q = n characters of Phred+33"""
    root = util.extract_golden("unmapped_small", str(tmp_path))
    exp = _gapout(root)
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        ln = np.arange(2, 2 + n, dtype=np.int32); ln[0] = 0
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        ph = (np.arange(int(off[-1])) * 7 % 94).astype(np.uint8); ph[1] = 93
        st = (np.arange(n) % 2).astype(np.uint8)
        err = C.create_string_buffer(512)
        cwd = os.getcwd(); os.chdir(root)
        try:
            rc = host.fighost_run_write_alnquality(h, api._p(ln, api.c_i32_p), api._p(off, api.c_i64_p), api._p(ph, api.c_u8_p), api._p(st, api.c_u8_p), err, 512)
        finally:
            os.chdir(cwd)
    finally:
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    want = "".join("\t".join(exp[g][:4]) + f"\t{ln[g]}\t{st[g]}\t" + (ph[int(off[g]):int(off[g + 1])] + 33).astype(np.uint8).tobytes().decode() + "\n" for g in range(n))
    got = util.read(os.path.join(root, "tmp", "gapalnquality.txt"))
    assert n >= 2 and got == want and "~" in got
    assert not os.path.exists(os.path.join(root, "tmp", "gapquality.txt"))


def test_figfill_names_a_missing_call(tmp_path):
    """FIGFILL_ALNQUALITY=1 on a library without fig_batch_alnqual (the one-lane emulation) is an error that names the call, before
    anything is filled or written; the host library has the bindings"""
    host = api.load_host_library()
    for fn in ("fighost_alnqual_gaps_on", "fighost_alnqual_map_bytes", "fighost_alnqual_nibble", "fighost_alnqual_set_nibble", "fighost_alnqual_flat", "fighost_alnqual_span",
               "fighost_run_write_alnquality"):
        assert hasattr(host, fn), fn
    root = util.extract_golden("unmapped_small", str(tmp_path))
    r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, {"FIGFILL_ALNQUALITY": "1"})
    assert r.returncode != 0 and "fig_batch_alnqual" in r.stderr and "FIGFILL_ALNQUALITY" in r.stderr
    for fn in ("gapalnquality.txt", "gapout.txt"):
        assert not os.path.exists(os.path.join(root, "tmp", fn)), fn


def test_planted_case_is_not_vacuous(planted):
    """The restatement alone, on the planted case.  Gap 0 (unedited; no read has an event): loglik and Phred equal the ungapped
    restatement bit for bit.  Gap 1 (the homopolymer one base short): Phred 93 on all 100 columns where the ungapped quality falls to
    0, and agree < depth on the planted substitutions only.  Gap 2 (a base too many at column 52): below 30 on column 52 only, where 29
    reads skip the column and the Phred is 1; 93 around it."""
    H, Wt = planted
    ev = [[Wt["n_ins"][k] + Wt["n_del"][k] for k in range(int(H.u_off[g]), int(H.u_off[g + 1]))] for g in range(3)]
    P = [gap_planes(H, Wt, g) for g in range(3)]
    U = [ungapped(H, g) for g in range(3)]
    print([sum(1 for v in e if v) for e in ev], [int(u[1].min()) for u in U], [int(p["phred"].min()) for p in P], [int((p["agree"] < p["depth"]).sum()) for p in P],
          [list(np.flatnonzero(u[1] < 30)) for u in U])
    assert Wt["aligned"].all() and [sum(1 for v in e if v) for e in ev] == [0, 21, 29]
    assert not Wt["d_end"][:40].any() and tbq.same_bits(P[0]["loglik"], U[0][0]) and P[0]["phred"].tobytes() == U[0][1].tobytes() and (P[0]["phred"] == 93).all()
    assert len(P[1]["phred"]) == 100 and (P[1]["phred"] == 93).all() and U[1][1].min() == 0 and list(np.flatnonzero(U[1][1] < 30)) == [37, 38, 40, 41, 42, 44]
    assert (P[1]["agree"] < P[1]["depth"]).sum() == 11 and not P[1]["skip"].any()
    assert list(np.flatnonzero(P[2]["phred"] < 30)) == [tie.UNIQUE_AT] and P[2]["phred"][tie.UNIQUE_AT] == 1 and P[2]["skip"][tie.UNIQUE_AT] == 29
    assert (np.delete(P[2]["phred"], tie.UNIQUE_AT) == 93).all() and list(np.flatnonzero(U[2][1] < 30)) == [45, 50, 51, 52] and U[2][1].min() == 0
    assert list(np.flatnonzero(P[2]["skip"])) == [tie.UNIQUE_AT] and P[2]["depth"][tie.UNIQUE_AT] == 0


def test_hand_cases_are_not_vacuous(stepsc, edges):
    """The restatement alone: the step case and the edge cases hold the shapes they are named for."""
    H, Wt = stepsc
    P0 = gap_planes(H, Wt, 0)
    k0 = int(H.u_off[0])
    assert Wt["aligned"][k0:k0 + 7].all() and list(Wt["n_del"][k0:k0 + 7]) == [1, 1, 0, 0, 0, 1, 1] and list(Wt["n_ins"][k0:k0 + 7]) == [0, 0, 2, 0, 0, 0, 0]
    assert P0["skip"][0] == 1 and P0["skip"][89] == 1 and P0["skip"][60] == 2 and P0["depth"][60] >= 1 and P0["skip"].sum() == 4
    steps_ins = Wt["maps"][k0 + 2]
    assert [c - v for c, v in enumerate(steps_ins) if v != NONE] == list(range(40)) + list(range(42, 72))        # bases 40, 41 inserted: their next column is 90 = n
    assert Wt["spans"][k0 + 2] == (50, 119) and Wt["d_end"][k0 + 2] == -2 and Wt["d_start"][k0 + 2] == 0
    assert H.seqs[k0 + 3][15] == ord("N") and Wt["maps"][k0 + 3][15 + W] == 7                                    # the N base has a nibble and no depth
    d20 = sum(1 for k in range(k0, k0 + 7) if Wt["spans"][k][0] <= 20 <= Wt["spans"][k][1])
    assert P0["depth"][20] == d20 - 1 and P0["skip"][20] == 0
    for g, n in enumerate(BLOCK_NS, start=1):
        ks = range(int(H.u_off[g]), int(H.u_off[g + 1]))
        assert int(H.filled_len[g]) == n and sum(Wt["aligned"][k] for k in ks) >= 6
        if n >= 255:
            assert [bool(Wt["aligned"][k]) for k in list(ks)[-4:]] == [True, False, True, False]
            assert any(Wt["n_ins"][k] + Wt["n_del"][k] > 0 for k in ks)
    P6 = gap_planes(H, Wt, 6)
    k6 = int(H.u_off[6])
    assert not Wt["aligned"][k6:k6 + 64].any() and Wt["aligned"][k6 + 64] and P6["depth"].max() == 1 and P6["depth"].sum() == 50
    # the N base inside an INS run
    Nc = nins_case()
    Wn = expected(Nc)
    assert Wn["n_ins"][0] == 3 and Wn["n_del"][0] == 0 and [c - v for c, v in enumerate(Wn["maps"][0]) if v != NONE] == list(range(30)) + list(range(33, 63))
    assert Wn["depth"].sum() == 60 and not Wn["skip"].any()
    # the edge case of the indel pass: N columns, undrawn and unaligned reads, the ends of the placement range, events of both kinds
    E, We = edges
    al = We["aligned"]
    assert (E.raw == ord("N")).any() and (We["agree"][E.raw[:len(We["agree"])] == ord("N")] == 0).all() and (We["depth"][E.raw[:len(We["depth"])] == ord("N")] > 0).any()
    assert (~al).sum() > 10 and (We["n_ins"][al] > 0).sum() > 5 and (We["n_del"][al] > 0).sum() > 5 and We["skip"].any()
    # the band's reach: 7 found with d_end at +-7, 8 not found
    B = tie.band_case()
    Wb = expected(B)
    assert list(Wb["d_end"]) == [7, 0, -7, 0] and list(Wb["d_start"]) == [0, 0, 0, 0] and list(Wb["n_del"]) == [7, 0, 0, 0] and list(Wb["n_ins"]) == [0, 0, 7, 0]
    assert list(np.flatnonzero(Wb["skip"])) == list(range(60, 67))
    # ins = del = 0 and a read whose every path is -inf: the flat path, -inf in loglik, the ungapped quality
    Z = tie.edge_case(model=tie.zero_rate_model())
    Wz = expected(Z)
    k = int(Z.u_off[8])
    Pz = gap_planes(Z, Wz, 8)
    Uz = ungapped(Z, 8)
    assert Wz["ll_gapped"][k] == NINF and Wz["maps"][k] == [NONE] * 7 + [7] * 40 + [NONE] * 7 and np.isneginf(Pz["loglik"]).any()
    assert tbq.same_bits(Pz["loglik"], Uz[0]) and Pz["phred"].tobytes() == Uz[1].tobytes() and not Wz["n_ins"].any() and not Wz["n_del"].any()


def case_lines(H, Wt, tabs):
    lm, le, lt, lI, lD = tabs
    hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v).reshape(-1))
    lines = [str(len(lm)), hx(lm), hx(le), hx(lt), hx(lI), hx(lD)]
    on = [g for g in range(len(H.filled_len)) if Wt["state"][g]]
    lines.append(str(len(on)))
    for g in on:
        n = int(H.filled_len[g]); a = int(H.str_off[g])
        S = tie.columns(H.contig, int(H.starts[g]), trp.G0, H.raw[a:a + n])
        ks = [k for k in range(int(H.u_off[g]), int(H.u_off[g + 1])) if Wt["aligned"][k]]
        lines += [f"{n} {len(ks)}", H.raw[a:a + n].tobytes().decode()]
        for k in ks:
            o, ln = int(H.draw_pos[k]), len(H.seqs[k])
            lines += [f"{o} {ln} {int(H.rev[k])}", "".join(str(int(c)) for c in S[PAD + o - W:PAD + o + ln + W]), H.seqs[k].tobytes().decode()]
    return lines, on


def test_kernel_pieces_on_the_cpu(planted, stepsc, edges, tmp_path):
    """The __host__ __device__ pieces of fig_alnqual.h and fig_alnqual_host.h compiled as plain C++ into a program of its own with
    AddressSanitizer and UBSan (tests/alnqual_main.cpp; run directly), over the planted, the step, the edge, the band, the zero-rate
    and the N-in-an-insertion case: inside the program the kernels' form (16-lane band, packed pointers, nibble map, the column walk
    over the reads in chunks) equals a sequential restatement in every map entry and every plane; its output equals the numpy
    restatement."""
    exe = str(tmp_path / "alnqual")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "alnqual_main.cpp")])
    B = tie.band_case(); Z = tie.edge_case(model=tie.zero_rate_model()); Nc = nins_case()
    nreads = ncols = 0
    for tag, (H, Wt) in (("planted", planted), ("steps", stepsc), ("edges", edges), ("band", (B, expected(B))), ("zero", (Z, expected(Z))), ("nins", (Nc, expected(Nc)))):
        lines, on = case_lines(H, Wt, tie.indel_tables(H.model.cstruct()))
        case = tmp_path / f"{tag}.txt"
        case.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(case)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines()]
        it = iter(rows)
        f64 = lambda t: np.array([int(t, 16)], dtype=np.uint64).view(np.float64)[0]
        for g in on:
            a, n = int(H.str_off[g]), int(H.filled_len[g])
            for k in range(int(H.u_off[g]), int(H.u_off[g + 1])):
                if not Wt["aligned"][k]:
                    continue
                t = next(it)
                assert t[0] == "R" and tbq.same_bits([f64(t[1])], [Wt["ll_gapped"][k]]), (tag, k)
                assert [int(v) for v in t[2:8]] == [Wt["n_ins"][k], Wt["n_del"][k], Wt["d_end"][k], Wt["d_start"][k], Wt["spans"][k][0], Wt["spans"][k][1]], (tag, k)
                assert [int(c, 16) for c in t[8]] == Wt["maps"][k], (tag, k)
                nreads += 1
            for x in range(n):
                t = next(it)
                assert t[0] == "C" and tbq.same_bits([f64(v) for v in t[1:5]], Wt["loglik"][a + x]), (tag, g, x)
                assert [int(v) for v in t[5:8]] == [Wt["depth"][a + x], Wt["agree"][a + x], Wt["skip"][a + x]], (tag, g, x)
                ncols += 1
        assert next(it, None) is None
    assert nreads > 400 and ncols > 2000


# ------------------------------------------------------------------------------------- GPU
PER_READ = ("ll_gapped", "n_ins", "n_del", "d_end", "d_start")


def same_per_read(A, I):
    for f in PER_READ:
        assert np.asarray(getattr(A, f)).tobytes() == np.asarray(getattr(I, f)).tobytes(), f


@pytest.mark.gpu
def test_planted_case_on_the_device(planted):
    """fig_batch_alnqual on the planted case: every output the restatement's, bit for bit; the five per-read arrays are Engine.indel's;
    so Phred 93 across the short homopolymer, and one column below 30 where 29 reads skip the extra base."""
    H, Wt = planted
    with _Eng(H) as eng:
        A = eng.alnqual(H.result(), H.origin)
        I = eng.indel(H.result(), H.origin)
    compare(A, Wt)
    same_per_read(A, I)
    P = [gap_planes(H, A, g) for g in range(3)]
    assert (P[1]["phred"] == 93).all() and list(np.flatnonzero(P[2]["phred"] < 30)) == [tie.UNIQUE_AT] and P[2]["skip"][tie.UNIQUE_AT] == 29
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["steps", "edges", "band", "zero", "nins"])
def test_edges_on_the_device(which, stepsc, edges):
    """The step case (DEL over columns 0 and n - 1, an INS run before column n, an N base on a column, a column one read skips and
    another covers, n = 1, 255, 256, 257 and 513, the ends of the placement range and one beyond, a chunk with no aligned read), the
    indel pass's edge case (1 .. 65 reads, lengths 1 .. 200 mixed, N bases and columns, undrawn reads), the band's reach, zero indel
    rates with an all -inf read, and an N base inside an INS run: every output the restatement's over 0xFF buffers, the per-read
    arrays Engine.indel's; the all -inf read's gap equals Engine.quality."""
    H, Wt = {"steps": lambda: stepsc, "edges": lambda: edges, "band": lambda: (tie.band_case(), None), "zero": lambda: (tie.edge_case(model=tie.zero_rate_model()), None),
             "nins": lambda: (nins_case(), None)}[which]()
    Wt = Wt or expected(H)
    with _Eng(H) as eng:
        A = eng.alnqual(H.result(), H.origin)
        I = eng.indel(H.result(), H.origin)
        Q = eng.quality(H.result(), H.origin) if which == "zero" else None
    compare(A, Wt)
    same_per_read(A, I)
    if which == "zero":
        a, b = int(H.str_off[8]), int(H.str_off[9])
        assert np.isneginf(A.loglik[a:b]).any() and tbq.same_bits(A.loglik[a:b], Q[0][a:b]) and A.phred[a:b].tobytes() == Q[1][a:b].tobytes()


@pytest.mark.gpu
def test_recruit_and_polish_compose(planted):
    """tre.withheld_case() composed recruit -> alnqual and recruit -> polish -> alnqual: on the merged plane the recruits are counted in
    depth and every output is the restatement's; after the polish all three gaps are Phred 93 with skip all zero and equal
    Engine.quality on Polish.result() bit for bit wherever no read has an event."""
    H, kinds, truth = tre.withheld_case()
    with _Eng(H) as eng:
        res = H.result()
        A0 = eng.alnqual(res, H.origin)
        R = eng.recruit(res, H.origin)
        M = R.result()
        A1 = eng.alnqual(M, H.origin)
        Pl = eng.polish(M, H.origin)
        PR = Pl.result()
        A2 = eng.alnqual(PR, H.origin)
        Q2 = eng.quality(PR, H.origin)
        I2 = eng.indel(PR, H.origin)
    compare(A0, expected(H))
    Hm = H.merged(R.draw_pos, R.draw_isz)
    compare(A1, expected(Hm))
    assert R.n_recruited[1] >= 15 and R.n_recruited[2] >= 15
    for g in (1, 2):
        a, b = int(H.str_off[g]), int(H.str_off[g + 1])
        assert A1.depth[a:b].sum() > A0.depth[a:b].sum() + 15 * 40 and (A1.depth[a:b] >= A0.depth[a:b]).all()
    assert A0.depth[:int(H.str_off[1])].tobytes() == A1.depth[:int(H.str_off[1])].tobytes()
    assert [s.tobytes() for s in Pl.strings()] == [truth.tobytes()] * 3
    assert len(A2.phred) == 303 and (A2.phred == 93).all() and not A2.skip.any() and list(A2.state) == [1, 1, 1]
    same_per_read(A2, I2)
    for g in range(3):
        ks = range(int(H.u_off[g]), int(H.u_off[g + 1]))
        a, b = int(PR.str_off[g]), int(PR.str_off[g + 1])
        # a column is clean when every read that reaches it, drawn flat or along its path, lies on d = 0 throughout
        clean = np.ones(b - a, bool)
        for k in ks:
            o, ln = int(PR.draw[0][k]), len(H.seqs[k])
            if o == INT_MIN or (A2.n_ins[k] == 0 and A2.n_del[k] == 0 and A2.d_end[k] == 0 and A2.d_start[k] == 0):
                continue
            lo = max(min(o, o + int(A2.d_start[k])), 0); hi = min(max(o + ln - 1, o + ln - 1 + int(A2.d_end[k])), b - a - 1)
            if A2.d_start[k] != INT_MIN and lo <= hi:
                clean[lo:hi + 1] = False
        print(g, int(clean.sum()), "clean columns of", b - a)
        assert g != 0 or clean.all()                              # (a recruit seeded on the far side of a site stays one diagonal off after the polish)
        assert tbq.same_bits(A2.loglik[a:b][clean], Q2[0][a:b][clean]) and A2.phred[a:b][clean].tobytes() == Q2[1][a:b][clean].tobytes()


@pytest.mark.gpu
def test_off_means_off_and_every_einval():
    """trp.HandPlace's gap list with its off states (by origin, by header, partial evidence): the restatement over the gaps that are
    on, defaults everywhere else over buffers that came in as 0xFF bytes; without origins the ORIGINAL gap is on too; a partial-mode
    model aligns nothing; a NULL member, a NULL struct, a drawn offset of 2^20 in a gap that is on and a freed batch are FIG_EINVAL."""
    H = trp.HandPlace()
    Wt = expected(H)
    with _Eng(H) as eng:
        A = eng.alnqual(H.result(), H.origin)
        compare(A, Wt)
        assert list(A.state) == trp.STATE and Wt["aligned"].sum() > 100 and (~Wt["aligned"]).sum() > 30
        for g in np.flatnonzero(A.state == 0):
            a, b = int(H.str_off[g]), int(H.str_off[g + 1])
            ks = slice(int(H.u_off[g]), int(H.u_off[g + 1]))
            assert not A.loglik[a:b].any() and not A.depth[a:b].any() and not A.agree[a:b].any() and not A.skip[a:b].any() and not A.phred[a:b].any()
            assert list(A.d_start[ks]) == [INT_MIN] * int(H.u_off[g + 1] - H.u_off[g]) and not A.ll_gapped[ks].any() and not A.d_end[ks].any()
        compare(eng.alnqual(H.result(), None), expected(H, state=[1, 1, 1, 1, 1, 0, 0, 1, 1]))
        r, keep = eng._filled_struct("alnqual", H.result())
        nu, n, total = H.NU, len(H.filled_len), int(H.str_off[-1])
        size = {"loglik": total * 4, "depth": total, "agree": total, "skip": total, "phred": total, "state": n}
        bufs = {f: np.zeros(max(size.get(f, nu), 1), dtype=np.float64 if t is api.c_double_p else np.uint8 if t is api.c_u8_p else np.int32) for f, t in api.FigGapAlnqual._fields_}

        def call(skip=None, filled=r):
            aq = api.FigGapAlnqual()
            for f, typ in api.FigGapAlnqual._fields_:
                if f != skip:
                    setattr(aq, f, api._p(bufs[f], typ))
            return eng.lib.fig_batch_alnqual(eng.ctx, C.byref(filled), None, C.byref(aq))
        assert call() == 0
        for f, _ in api.FigGapAlnqual._fields_:
            assert call(skip=f) == -1, f
        assert eng.lib.fig_batch_alnqual(eng.ctx, C.byref(r), None, None) == -1 and eng.lib.fig_batch_alnqual(eng.ctx, None, None, None) == -1
        for k, v, ok in ((int(H.u_off[2]) + 1, 1 << 20, False), (int(H.u_off[2]) + 1, -(1 << 20), False), (int(H.u_off[2]) + 1, (1 << 20) - 1, True), (int(H.u_off[6]) + 1, 1 << 20, True)):
            B = trp.HandPlace()
            B.draw_pos[k] = v
            if ok:
                eng.alnqual(B.result(), B.origin)
            else:
                with pytest.raises(RuntimeError):
                    eng.alnqual(B.result(), B.origin)
        bad = H.result()
        bad.str_off = bad.str_off.copy(); bad.str_off[2] -= 1                  # the string of gap 1 no longer has filled_len bytes
        with pytest.raises(RuntimeError):
            eng.alnqual(bad, H.origin)
        eng.free_batch()
        with pytest.raises(RuntimeError):
            eng.alnqual(H.result(), H.origin)
    Pm = trp.HandPlace(mode="partial")
    with _Eng(Pm) as eng:
        A = eng.alnqual(Pm.result(), Pm.origin)
        assert len(A.ll_gapped) == 0 and not A.state.any() and not A.loglik.any() and not A.depth.any() and not A.skip.any() and not A.phred.any()


@pytest.mark.gpu
def test_deterministic_and_read_only(planted, edges):
    """a second call returns the same bytes; fig_batch_quality and fig_batch_indel on the caller's `filled` before and after the call
    return the same bytes; the caller's `filled` is unchanged"""
    for H in (planted[0], edges[0]):
        with _Eng(H) as eng:
            res = H.result()
            before = [np.array(a).tobytes() for a in (res.filled_len, res.str_off, res.raw) + tuple(res.draw)]
            I0 = eng.indel(res, H.origin); Q0 = eng.quality(res, H.origin)
            A0 = eng.alnqual(res, H.origin)
            I1 = eng.indel(res, H.origin); Q1 = eng.quality(res, H.origin)
            A1 = eng.alnqual(res, H.origin)
            for f, _ in api.FigGapIndel._fields_:
                assert np.asarray(getattr(I0, f)).tobytes() == np.asarray(getattr(I1, f)).tobytes(), f
            for a, b in zip(Q0, Q1):
                assert a.tobytes() == b.tobytes()
            for f, _ in api.FigGapAlnqual._fields_:
                assert np.asarray(getattr(A0, f)).tobytes() == np.asarray(getattr(A1, f)).tobytes(), f
            assert before == [np.array(a).tobytes() for a in (res.filled_len, res.str_off, res.raw) + tuple(res.draw)]


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


def run_golden_alnqual(root):
    """A golden filled as figfill fills it (draw and support planes), with the quality, the indel pass and the alnqual of the fill's
    own result, then the chain recruit -> polish -> alnqual, all while the batch is resident, then a second plain fill -> Fill with
    .A, .I, .Q, .chain (the FillResult of the chain), .second and what the restatement needs"""
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
            res = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, quality=True, indel=True, alnqual=True, keep_resident=True)
            F.chain = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, recruit=True, polish=True, alnqual=True, keep_resident=True)
            F.second = _take(Fill(), eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.A, F.I, F.Q = res.alnqual, res.indel, res.quality
        return F
    finally:
        host.fighost_run_close(h)


@pytest.fixture(scope="module")
def afills(tmp_path_factory):
    """name -> golden filled with the planes above; computed once per module, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden_alnqual(util.extract_golden(name, str(tmp_path_factory.mktemp(name))))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "bench_b160"])
def test_goldens_end_to_end(name, afills):
    """A golden filled as figfill fills it, then the quality over gapped alignments: states by the rule; the per-read arrays are the
    indel pass's; no read has an event there, so loglik and Phred equal Engine.quality's bit for bit on every gap that is on for both;
    every output the restatement's -- over all gaps of unmapped_small and over the first four gaps of bench_b160; a second fill of
    the still resident batch returns the bytes of the first."""
    F = afills(name)
    assert F.unmapped
    state = []
    for g in range(F.n):
        n = int(F.filled_len[g]); org = int(F.origin[g])
        state.append(int(n > 0 and int(F.draw_len[2 * g]) == n and int(F.draw_len[2 * g + 1]) < 0 and bool(org & F_) and not org & O_))
    assert list(F.A.state) == state == list(F.I.state) and sum(state) > 0
    same_per_read(F.A, F.I)
    events = int(((F.A.n_ins + F.A.n_del) > 0).sum())
    both = [g for g in range(F.n) if state[g] and F.Q[2][g]]
    print(f"{name}: gaps on {sum(state)} of {F.n}, on for the quality as well {len(both)}, reads with an event {events}, reads off the drawn diagonal {int((F.A.d_end != 0).sum())}, "
          f"columns {int(F.A.depth.size)}, skipped {int(F.A.skip.sum())}")
    assert both
    for g in both:
        a, b = int(F.str_off[g]), int(F.str_off[g + 1])
        assert tbq.same_bits(F.A.loglik[a:b], F.Q[0][a:b]) and F.A.phred[a:b].tobytes() == F.Q[1][a:b].tobytes(), g
    V = _GoldenView(F, state)
    gaps = None if name == "unmapped_small" else list(range(min(4, F.n)))
    Wt = expected(V, tabs=F.tabs, gaps=gaps)
    compare(F.A, Wt, H=V, gaps=gaps)
    assert Wt["aligned"].any() and Wt["depth"].any()
    for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
        assert np.array_equal(getattr(F, f), getattr(F.second, f)), f


def _q33(ph):
    return (np.asarray(ph, dtype=np.uint8) + 33).astype(np.uint8).tobytes().decode()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True])
def test_gapalnquality_file_is_the_same_from_every_host_path(chain, afills, tmp_path, monkeypatch):
    """unmapped_small with FIGFILL_ALNQUALITY=1 -- beside FIGFILL_QUALITY=1 and FIGFILL_INDEL=1, or at the end of FIGFILL_RECRUIT=1 and
    FIGFILL_POLISH=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 and two-rank figfill_mp leave the same gapalnquality.txt,
    which is the file of the API composition; the reference's files stay byte-identical in every run; without the variable the file
    is absent and every other file is what the runs with it wrote."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    name = "unmapped_small"
    for v in ("FIGFILL_SUPPORT", "FIGFILL_QUALITY", "FIGFILL_PLACEMENT", "FIGFILL_QUALITY_MINPQ", "FIGFILL_SOFTQUALITY", "FIGFILL_INDEL", "FIGFILL_POLISH", "FIGFILL_POLISH_ROUNDS",
              "FIGFILL_RECRUIT", "FIGFILL_RECRUIT_MARGIN", "FIGFILL_ALNQUALITY", "FIGFILL_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    roots = [util.extract_golden(name, str(tmp_path / f"r{k}")) for k in range(4)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    base = {"FIGFILL_RECRUIT": "1", "FIGFILL_POLISH": "1"} if chain else {"FIGFILL_QUALITY": "1", "FIGFILL_INDEL": "1"}
    others = ("gaprecruit.txt", "gappolished.txt") if chain else ("gapquality.txt", "gapindel.txt")
    on = dict(base, FIGFILL_ALNQUALITY="1")
    r = util.run([util.FIGFILL] + argv, roots[3], base)
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
    files = [util.read(os.path.join(root, "tmp", "gapalnquality.txt")) for root in roots[:3]]
    assert files[0] == files[1] == files[2]
    F = afills(name)
    A = F.chain.alnqual if chain else F.A
    fin = A.filled                                                # the FillResult that was scored
    exp = _gapout(roots[0])
    lines = files[0].splitlines()
    assert len(lines) == len(exp) == F.n
    for g, (ln, e) in enumerate(zip(lines, exp)):
        f = (ln + "\t").split("\t")[:7] if ln.endswith("\t") else ln.split("\t")
        a, n = int(fin.str_off[g]), int(fin.filled_len[g])
        assert len(f) == 7 and f[:4] == e[:4] and f[4] == str(n) and f[5] == str(int(A.state[g])) and f[6] == _q33(A.phred[a:a + max(n, 0)]), g
    assert any(ln.split("\t")[5] == "1" for ln in lines)
    if chain:
        assert [int(ln.split("\t")[4]) for ln in lines] == [int(v) if s & api.POLISH_ON else int(fl) for v, s, fl in zip(F.chain.polish.polished_len, F.chain.polish.state, F.filled_len)]
    for k, root in enumerate(roots):
        assert os.path.exists(os.path.join(root, "tmp", "gapalnquality.txt")) == (k < 3)
        assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
        for fn in ("gapout.txt", "draw.txt", "filledContigs.fa") + others:
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(roots[3], "tmp", fn)), (root, fn)
