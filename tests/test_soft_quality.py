"""Per-base quality that sums over read placements (fig_gap_softqual / fig_batch_softqual, include/figbird_hip.h).

There is no reference for this feature; the header's definition is the specification.  The comparisons use a numpy restatement of
it, per scored read: Lr over the valid offsets exactly as test_read_placement.restate_read computes it (vectorised over offsets,
one add per base in ascending j: bit-equal to the device by construction), then the active cut, u = 10^d, Z (math.fsum) and
p = u / Z in doubles, and the contributions of all reads accumulated in np.longdouble and rounded once (per read the sum over j of
p[x - j] * t_j is a convolution of the weight row with the read's terms, done in longdouble; -inf terms are tracked apart).

The bar: state exact; the 0.0 and +-inf entries of both planes exact on the bit pattern; every finite non-zero entry within
|got - want| <= 1e-9 * |want| + 1e-300.  All terms of an entry have one sign, so any summation order stays within terms * 2^-53
relative (at most 3000 reads x 200 covering placements = 6e5 terms: 7e-11); a weight carries exp10's error at |d| <= 300
(300 ln10 ulp, 8e-14) and a few ulp from the division: 1e-9 leaves a factor above 10.  phred equals fighost's Phred of the
returned eloglik exactly, and the restatement's Phred wherever the restatement's unrounded value lies further than 1e-3 from a
rounding boundary; at most 2 % of the on-columns may be left out that way."""
import ctypes as C
import math
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import util
from figbird_amd import api
import test_base_quality as tbq
from test_base_support import CODE, INT_MIN, Fill, _gapout, _open_run, _take
from test_read_placement import EDGE_LENS, FLANK, G0, GAPS, STATE, F_, HandPlace, columns, isz_of, place_tables

NINF = -math.inf
LQ = float.fromhex("-0x1.34413509f79ffp-1")
CUT = -300.0
RG = 8                                   # FIG_SQ_RG (fig_softqual.h): reads of a row group
LD = np.longdouble


# ------------------------------------------------------------------------------------- the restatement
def read_scores(S, n, seq, rev, pos, gap_start, G0_, tabs):
    """one read -> (the valid offsets, Lr of each): test_read_placement.restate_read's arithmetic"""
    lm, le, lt, li, Tmin, Tmax, MI = tabs
    ln = len(seq)
    o = np.arange(-(ln - 1), n, dtype=np.int64)
    isz = isz_of(pos, gap_start, G0_, n, ln, o)
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
    return o, Lr


def read_terms(seq, rev, tabs):
    """-> (acgt [len] bool, s [len], t [len, 4]: the term of base j under true base b, 0.0 for a base outside ACGT)"""
    lm, le, lt = tabs[:3]
    ln = len(seq)
    s = CODE[seq]
    acgt = s < 4
    j = np.arange(ln)
    k = (ln - 1 - j) if rev else j
    sc = np.where(acgt, s, 0)
    t = np.zeros((ln, 4))
    for b in range(4):
        t[:, b] = np.where(acgt, np.where(sc == b, lm[k], le[k] + lt[b, sc]), 0.0)
    return acgt, sc, t


def host_mz(ll_drawn, ll_other, sum_other):
    """fighost_softqual_mz of one read -> (M, Z, takes part)"""
    host = api.load_host_library()
    a, b, c = (np.array([v], dtype=np.float64) for v in (ll_drawn, ll_other, sum_other))
    M = np.full(1, np.nan); Z = np.full(1, np.nan); part = np.full(1, 0xFF, dtype=np.uint8)
    assert host.fighost_softqual_mz(1, api._p(a, api.c_double_p), api._p(b, api.c_double_p), api._p(c, api.c_double_p), api._p(M, api.c_double_p), api._p(Z, api.c_double_p), api._p(part, api.c_u8_p)) == 0
    return float(M[0]), float(Z[0]), int(part[0])


def weights(o, Lr):
    """-> None for a read that takes no part, else (p [len(o)] with 0.0 for an inactive placement, M, Z, cut: a finite score lies below
    the cut).  The library's host half is held against it on the way: with the first valid placement taken as the drawn one, M / Z
    from the placement pass's three outputs are M exactly and Z within 1e-12 (sum_other holds the terms below the cut too)."""
    if not len(o):
        return None
    M = float(Lr.max())
    rest = Lr[1:]
    top = float(rest.max()) if len(rest) else NINF
    Mh, Zh, part = host_mz(float(Lr[0]), top, 0.0 if M == NINF else math.fsum(float(10.0 ** (v - M)) for v in rest if v > NINF))
    assert part == int(M > NINF)
    if M == NINF:
        return None
    d = Lr - M
    act = d >= CUT
    u = np.zeros(len(o))
    u[act] = np.power(10.0, d[act])
    Z = math.fsum(u[act])
    assert Mh == M and abs(Zh - Z) <= 1e-12 * Z
    return u / Z, M, Z, bool((np.isfinite(Lr) & ~act).any())


def restate_gap(S, n, reads, gap_start, G0_, tabs):
    """reads: (sequence, reversed, anchor) of the gap's scored reads in read order -> dict: wcount / eloglik float64 [n, 4], the
    unrounded longdouble eloglik, and what the non-vacuity test asks about"""
    W = np.zeros((n, 4), dtype=LD); E = np.zeros((n, 4), dtype=LD); Einf = np.zeros((n, 4), dtype=bool); hit = np.zeros(n, dtype=bool)
    info = dict(cut=0, minf=0, part=0, active=0, split=0)
    for seq, rev, pos in reads:
        o, Lr = read_scores(S, n, seq, rev, pos, gap_start, G0_, tabs)
        w = weights(o, Lr)
        if w is None:
            info["minf"] += int(len(o) > 0)
            continue
        p, M, Z, cut = w
        info["cut"] += int(cut); info["part"] += 1; info["active"] += int((p > 0).sum()); info["split"] += int(len(p) > 1 and np.sort(p)[-2] > 1e-4)
        ln = len(seq)
        row = np.zeros(n + ln - 1, dtype=LD)
        row[o + ln - 1] = p
        pos_row = (row > 0).astype(np.float64)
        acgt, s, t = read_terms(seq, rev, tabs)
        sl = slice(ln - 1, ln - 1 + n)
        hit |= np.convolve(pos_row, acgt.astype(np.float64))[sl] > 0.5
        for b in range(4):
            W[:, b] += np.convolve(row, (acgt & (s == b)).astype(LD))[sl]
            tb = t[:, b]
            inf = np.isinf(tb)
            E[:, b] += np.convolve(row, np.where(inf, 0.0, tb).astype(LD))[sl]
            if inf.any():
                Einf[:, b] |= np.convolve(pos_row, inf.astype(np.float64))[sl] > 0.5
    e64 = E.astype(np.float64)
    e64[Einf] = NINF
    El = E.copy(); El[Einf] = NINF
    return dict(wcount=W.astype(np.float64), eloglik=e64, exact=El, hit=hit, **info)


def phred_margin(exact, raw):
    """the restatement's Phred per column and whether its unrounded value lies further than 1e-3 from a rounding boundary"""
    n = len(raw)
    far = np.ones(n, dtype=bool)
    ll = np.asarray(exact, dtype=LD)
    for x in range(n):
        c = int(CODE[raw[x]])
        m = ll[x].max()
        if c > 3 or m == NINF:
            continue
        w = np.where(np.isinf(ll[x]), LD(0), np.power(LD(10), ll[x] - m))
        num = sum(w[b] for b in range(4) if b != c)
        perr = num / (num + w[c])
        if perr == 0:
            continue
        q = float(-10 * np.log10(perr) + LD(0.5))
        far[x] = abs(q - round(q)) > 1e-3
    return tbq.phred_of(np.asarray(exact, dtype=np.float64), raw), far


def restate_hand(H):
    """the restatement over every gap of a HandPlace that is on -> (wcount [total, 4], eloglik [total, 4], phred, far, per-gap dicts)"""
    tabs = place_tables(H.model.cstruct())
    total = int(H.str_off[-1])
    W = np.zeros((total, 4)); E = np.zeros((total, 4)); ph = np.zeros(total, dtype=np.uint8); far = np.ones(total, dtype=bool)
    per = {}
    sc = H.scored()
    for g in range(len(H.gaps)):
        if not H.state[g]:
            continue
        a, b = int(H.str_off[g]), int(H.str_off[g + 1])
        reads = [(H.seqs[k], int(H.rev[k]), H.pos[k]) for k in range(int(H.u_off[g]), int(H.u_off[g + 1])) if sc[k]]
        R = restate_gap(H.S[g], b - a, reads, int(H.starts[g]), G0, tabs)
        W[a:b], E[a:b] = R["wcount"], R["eloglik"]
        ph[a:b], far[a:b] = phred_margin(R["exact"], H.raw[a:b])
        per[g] = R
    return W, E, ph, far, per


def compare_planes(got, want, what):
    """the bar of the module docstring on one plane; returns the largest relative difference over the finite non-zero entries"""
    got = np.ascontiguousarray(got, dtype=np.float64); want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    special = (want == 0) | np.isinf(want)
    bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64))[special].ravel())
    assert not len(bad), f"{what}: {len(bad)} of the 0.0 / inf entries differ, e.g. got {got[special].ravel()[bad[:4]]}, want {want[special].ravel()[bad[:4]]}"
    g, w = got[~special], want[~special]
    assert np.isfinite(g).all(), what
    d = np.abs(g - w)
    lim = 1e-9 * np.abs(w) + 1e-300
    rel = float((d / np.abs(w)).max()) if len(w) else 0.0
    print(f"{what}: {len(w)} finite non-zero entries, largest |got - want| / |want| = {rel:.3e}")
    assert (d <= lim).all(), f"{what}: {int((d > lim).sum())} entries outside the bound, largest relative difference {rel:.3e}"
    return rel


def compare_phred(phred, eloglik, raw, on_cols, want_ph, far):
    """phred is fighost's Phred of the returned eloglik; the restatement's wherever that is far from a boundary; <= 2 % are not"""
    assert np.array_equal(phred[on_cols], tbq.phred_of(eloglik, raw)[on_cols])
    assert (phred[~on_cols] == 0).all()
    assert (~far[on_cols]).sum() <= 0.02 * on_cols.sum()
    sel = on_cols & far
    assert np.array_equal(phred[sel], want_ph[sel])


def on_columns(state, filled_len):
    return np.repeat(np.asarray(state, dtype=bool), np.maximum(filled_len, 0))


# ------------------------------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def hand():
    """test_read_placement's hand-made case as it stands, and its restatement: built once, never modified"""
    H = HandPlace()
    return H, restate_hand(H)


@pytest.fixture(scope="module")
def hand_edge():
    """test_read_placement's edge-length case (read lengths 1, 16, 17, 32, 33, 199; 65 reads; 40 columns) and its restatement"""
    H = HandPlace(seed=20261020, gaps=[(40, 65, 0, "u", 40, F_, "")], state=[1], lens=EDGE_LENS, last_n=True)
    return H, restate_hand(H)


ROWGROUP_READS = (RG - 1, RG, RG + 1, 2 * RG + 1)


@pytest.fixture(scope="module")
def hand_rowgroups():
    """four gaps of 40 columns with RG-1, RG, RG+1 and 2 RG+1 reads: the edges of a row group of weight rows; and a fifth gap that is
    on but has no drawn read, so that none of its columns has a contribution.  The model's e[17] and T[C][G] are not 0 here: the far
    placements of the long reads are finite and lie below the -300 cut (under the hand-made model they are -inf)."""
    H = HandPlace(seed=20261021, gaps=[(40, r, 0, "u", 40, F_, "") for r in ROWGROUP_READS] + [(40, 3, 0, "u", 40, F_, "")], state=[1] * 5)
    H.model.e[17] = 0.0123; H.model.T[1 * 5 + 2] = 0.05
    H.draw_pos[int(H.u_off[4]):int(H.u_off[5])] = INT_MIN
    return H, restate_hand(H)


UNIT32 = np.frombuffer(b"ACGGTCATTGCAAGCTTGACCATGGATCGTAC", dtype=np.uint8)


def ambiguous_case():
    """One gap of 64 columns at low coverage: the string is a 32-base unit twice, the second copy differing in base 30.  Four reads
    of 15 bases, exact copies, all placements valid under a flat insert-size table: reads 0 and 1 lie inside the part the copies
    share and fit both equally well; reads 2 and 3 cover the base that differs and fit once.  Every read is drawn at its first
    fit.  Made from a HandPlace by overwriting its string, reads and anchors in place, in the batch as well."""
    H = HandPlace(seed=20261023, gaps=[(64, 4, 0, "u", 64, F_, "")], state=[1], lens=(15,))
    second = UNIT32.copy(); second[30] = ord("A") if second[30] != ord("A") else ord("C")
    H.raw[:] = np.concatenate([UNIT32, second])
    st = int(H.starts[0])
    H.S[0] = columns(H.contig, st, G0, H.raw)
    soff = H.batch.u_seq_off
    for k, (src, o) in enumerate(((UNIT32[0:15], 0), (UNIT32[5:20], 5), (UNIT32[16:31], 16), (second[17:32], 49))):
        H.seqs[k][:] = src; H.batch.u_seq[int(soff[k]):int(soff[k + 1])] = src
        H.rev[k] = 0
        H.pos[k] = st - 500; H.batch.u_anchor_pos[k] = st - 500            # left anchor: isz(o) = 515 + o, inside the thresholds everywhere
        H.draw_pos[k] = o
    return H


@pytest.fixture(scope="module")
def hand_ambiguous():
    H = ambiguous_case()
    return H, restate_hand(H)


def case_file(H, path):
    """the case file of tests/placement_read_main.cpp and tests/softqual_column_main.cpp over the on-gaps of H -> the gaps written"""
    m = H.model
    on = [g for g in range(len(H.gaps)) if H.state[g]]
    lines = ["200", " ".join(float(v).hex() for v in m.e), " ".join(float(v).hex() for v in m.T), f"{len(m.insd)} {m.Tmin} {m.Tmax}",
             " ".join(float(v).hex() for v in m.insd), str(len(on))]
    for g in on:
        n, st = int(H.filled_len[g]), int(H.starts[g])
        left = [CODE[H.contig[st - k]] if st - k >= 0 else 4 for k in range(1, FLANK + 1)]
        right = [CODE[H.contig[st + G0 + k]] if st + G0 + k < len(H.contig) else 4 for k in range(FLANK)]
        ks = range(int(H.u_off[g]), int(H.u_off[g + 1]))
        lines += [f"{n} {st} {G0} {len(ks)}", "".join(str(int(c)) for c in left + right), H.raw[int(H.str_off[g]):int(H.str_off[g + 1])].tobytes().decode() or "-"]
        lines += [f"{int(H.draw_pos[k])} {len(H.seqs[k])} {int(H.rev[k])} {H.pos[k]} {H.seqs[k].tobytes().decode()}" for k in ks]
    path.write_text("\n".join(lines) + "\n")
    return on


@pytest.fixture(scope="module")
def column_program(tmp_path_factory):
    """tests/softqual_column_main.cpp as a program of its own with AddressSanitizer and UBSan"""
    exe = str(tmp_path_factory.mktemp("softqual") / "softqual_column")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "softqual_column_main.cpp")])
    return exe


def run_program(exe, H, tmp_path, *mode):
    on = case_file(H, tmp_path / "case.txt")
    r = subprocess.run([exe, str(tmp_path / "case.txt"), *mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([int(t, 16) for t in r.stdout.split()], dtype=np.uint64).view(np.float64).reshape(-1, 8)
    cols = np.concatenate([np.arange(int(H.str_off[g]), int(H.str_off[g + 1])) for g in on])
    assert len(got) == len(cols)
    return got[:, :4], got[:, 4:], cols


# ------------------------------------------------------------------------------------- CPU
def test_softqual_abi_surface(tmp_path):
    """The call is declared with exactly its prototype, bound and exported; fig_gap_softqual is four pointers, 32 bytes;
    fig_gap_results did not grow and the version did not move; NULL members are FIG_EINVAL; the emulation library, which lacks the
    call, still loads -- and asking it for the soft quality is an error that names the call, in Python and through figfill (before
    anything is written)."""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert re.search(r"^int fig_batch_softqual\(fig_ctx \*ctx, const fig_gap_results \*filled, const int32_t \*origin,\s*fig_read_placement \*placement_or_null, fig_gap_softqual \*out\);", hdr, flags=re.M)
    assert "fig_batch_softqual" in api.EXPORTS
    lib = C.CDLL(util.pbuild.LIB)
    assert hasattr(lib, "fig_batch_softqual")
    assert re.search(r"#define FIG_ABI_VERSION 1\b", hdr)
    names = ["wcount", "eloglik", "phred", "state"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu %d %d", sizeof(fig_gap_softqual), sizeof(fig_gap_results), '
           'FIG_SOFTQ_OFF, FIG_SOFTQ_ON);' + "".join(f'printf(" %zu", offsetof(fig_gap_softqual, {f}));' for f in names) + 'printf("\\n");return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert out[0] == C.sizeof(api.FigGapSoftqual) == 32
    assert out[1] == C.sizeof(api.FigGapResults) == 128
    assert out[2:4] == [api.SOFTQ_OFF, api.SOFTQ_ON] == [0, 1]
    assert out[4:] == [getattr(api.FigGapSoftqual, f).offset for f in names] == [0, 8, 16, 24]
    # NULL members: refused before the context is looked at
    full = api.load_library()
    buf = np.zeros(8)
    for missing in [None] + names:
        sq = api.FigGapSoftqual()
        for f in names:
            if f != missing:
                setattr(sq, f, C.cast(buf.ctypes.data, dict(api.FigGapSoftqual._fields_)[f]))
        rc = full.fig_batch_softqual(None, None, None, None, C.byref(sq))
        assert rc == -1, missing                                 # FIG_EINVAL (every member given: the NULL context)
    sq = api.FigGapSoftqual()
    for f in names:
        setattr(sq, f, C.cast(buf.ctypes.data, dict(api.FigGapSoftqual._fields_)[f]))
    assert full.fig_batch_softqual(None, None, None, C.byref(api.FigReadPlacement()), C.byref(sq)) == -1
    assert full.fig_batch_softqual(None, None, None, None, None) == -1
    emu = api.load_library(util.EMULIB)
    assert not hasattr(emu, "fig_batch_softqual") and emu.fig_version() == 1
    eng = api.Engine(0, lib_path=util.EMULIB)
    try:
        eng.n_gaps = 0
        with pytest.raises(RuntimeError, match="fig_batch_softqual"):
            eng.softqual(api.FillResult(np.zeros(1, np.int32), np.zeros(1, np.int32), None, str_off=np.zeros(1, np.int64)))
        with pytest.raises(RuntimeError, match="fig_batch_softqual"):
            eng.fill_resident(softqual=True)
    finally:
        eng.close()
    host = api.load_host_library()
    for fn in ("fighost_softqual_gaps_on", "fighost_softqual_active", "fighost_softqual_mz", "fighost_run_write_softquality"):
        assert hasattr(host, fn), fn
    assert [f.name for f in api.FillResult.__dataclass_fields__.values()][-1] == "softqual"
    root = util.extract_golden("partial_small", str(tmp_path / "r"))
    r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, {"FIGFILL_SOFTQUALITY": "1"})
    assert r.returncode != 0 and "fig_batch_softqual" in r.stderr
    for fn in ("gapsoftquality.txt", "gapquality.txt", "gapplacement.txt", "gapout.txt"):
        assert not os.path.exists(os.path.join(root, "tmp", fn)), fn


def test_on_off_rule():
    """Table-driven: FIG_SOFTQ_ON exactly where the placement is FIG_PLACE_ON."""
    host = api.load_host_library()
    rows = [(n, hdr, org) for n in (0, -3, 1, 57) for hdr in [(-1, -1), (n, -1), (-1, n), (n + 1, -1), (n, n), (n, 0), (0, -1)] for org in [None] + list(range(8))]
    seen = set()
    for given in (False, True):
        sel = [r for r in rows if (r[2] is not None) == given]
        fl = np.array([r[0] for r in sel], dtype=np.int32); dl = np.array([h for r in sel for h in r[1]], dtype=np.int32)
        org = np.array([r[2] or 0 for r in sel], dtype=np.int32)
        for unm in (1, 0):
            st = np.full(len(sel), 0xFF, dtype=np.uint8); pl = np.full(len(sel), 0xFF, dtype=np.uint8)
            args = (unm, len(sel), api._p(fl, api.c_i32_p), api._p(dl, api.c_i32_p), api._p(org, api.c_i32_p) if given else None)
            assert host.fighost_softqual_gaps_on(*args, api._p(st, api.c_u8_p)) == 0
            assert host.fighost_placement_gaps_on(*args, api._p(pl, api.c_u8_p)) == 0
            want = [1 if (unm and n > 0 and lu == n and lp < 0 and (o is None or (o & 1 and not o & 2))) else 0 for n, (lu, lp), o in sel]
            assert list(st) == want == list(pl)
            seen |= set(st)
    assert seen == {api.SOFTQ_OFF, api.SOFTQ_ON}


_mz = host_mz


def test_active_cut_and_mz_by_hand():
    """The cut is d >= -300 exactly; M / Z from the three outputs of the placement pass: a read whose placements are all -inf takes
    no part; one placement at d = -300 exactly is active and one the next double below is not; Z = sum_other + 10^(ll_drawn - M)."""
    host = api.load_host_library()
    act = lambda d: int(host.fighost_softqual_active(C.c_double(d)))
    assert act(0.0) == 1 and act(-299.999) == 1 and act(-300.0) == 1
    assert act(np.nextafter(-300.0, -math.inf)) == 0 and act(-301.0) == 0 and act(NINF) == 0 and act(math.nan) == 0
    assert _mz(NINF, NINF, 0.0)[2] == 0                          # no valid placement at all, or every valid placement -inf
    assert _mz(-7.0, NINF, 0.0) == (-7.0, 1.0, 1)                # the drawn placement alone
    assert _mz(NINF, -7.0, 1.0) == (-7.0, 1.0, 1)                # drawn where no placement is: the others carry it
    assert _mz(-7.0, -7.0, 2.0) == (-7.0, 3.0, 1)                # three equal placements
    M, Z, part = _mz(-10.0, -7.0, 1.0)                           # the drawn one three decades below the best
    assert (M, part) == (-7.0, 1) and abs(Z - 1.001) < 1e-15
    # the restatement on the same edges: scores 0, -300 and the next double below -300
    below = float(np.nextafter(-300.0, -math.inf))
    p, M, Z, cut = weights(np.arange(3), np.array([0.0, -300.0, below]))
    assert M == 0.0 and p[0] > 0 and p[1] > 0 and p[2] == 0.0 and cut and abs(p[1] / p[0] - 1e-300) < 1e-312
    assert weights(np.arange(2), np.array([NINF, NINF])) is None and weights(np.arange(0), np.zeros(0)) is None
    p, M, Z, cut = weights(np.arange(2), np.array([-5.0, NINF]))
    assert list(p) == [1.0, 0.0] and not cut


def test_softquality_writer_format(tmp_path):
    """fighost_run_write_softquality on hand-made arrays: gapquality.txt's format, `g contig start G0 n state Q`, in
    gapsoftquality.txt."""
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
        rc = host.fighost_run_write_softquality(h, api._p(fl, api.c_i32_p), api._p(off, api.c_i64_p), api._p(ph, api.c_u8_p), api._p(st, api.c_u8_p), err, 512)
    finally:
        os.chdir(cwd)
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    head = ["\t".join(e[:4]) for e in exp]
    want = f"{head[0]}\t4\t1\t!+~J\n{head[1]}\t0\t0\t\n{head[2]}\t2\t1\t(]\n"
    assert util.read(os.path.join(root, "tmp", "gapsoftquality.txt")) == want
    assert not os.path.exists(os.path.join(root, "tmp", "gapquality.txt"))


def hard_quality(H, g):
    """fig_gap_quality's loglik of gap g by its restatement: every drawn read at its drawn offset"""
    tabs = tbq.tables(H.model.cstruct())
    ks = [k for k in range(int(H.u_off[g]), int(H.u_off[g + 1])) if H.draw_pos[k] != INT_MIN]
    return tbq.restate(int(H.filled_len[g]), [(int(H.draw_pos[k]), H.seqs[k], bool(H.rev[k])) for k in ks], tabs)


def test_hand_case_is_not_vacuous(hand, hand_rowgroups):
    """The restatement of the hand-made case holds what the device test is meant to exercise: a column with eloglik = -inf, a read
    with M = -inf, a soft Phred below the hard one on gap 2's near-repeat, both planes with finite
    non-zero entries -- and at most 2 % of the on-columns within 1e-3 of a rounding boundary of the Phred.  A column of an on-gap
    with no contribution the hand-made case cannot hold as it stands (wherever one read of a gap takes part, its placements cover
    every column), and a read cut by the -300 rule neither (e[17] = 0 and T[C][G] = 0 make the far placements of its long reads
    -inf, not small): the row-group case carries a gap that is on with no drawn read and reads with finite scores below the cut,
    checked here as well."""
    H, (W, E, ph, far, per) = hand
    on = on_columns(H.state, H.filled_len)
    assert list(H.state) == STATE and on.sum() == 1 + 65 + 257 + 600 + 12 + 300
    assert np.isneginf(E[on]).any() and (np.isfinite(E[on]) & (E[on] != 0)).sum() > 1000 and not np.isnan(E).any()
    hit = np.concatenate([per[g]["hit"] if g in per else np.zeros(int(H.filled_len[g]), dtype=bool) for g in range(len(GAPS))])
    assert (W[on & ~hit] == 0).all() and (E[on & ~hit] == 0).all() and (W[on & hit].sum(axis=1) > 0).all()
    assert (W[~on] == 0).all() and (E[~on] == 0).all()
    assert per[0]["minf"] >= 1
    assert all(r["active"] > r["part"] for g, r in per.items() if r["part"] and H.filled_len[g] > 1)     # more than one placement per read carries weight
    a, b = int(H.str_off[2]), int(H.str_off[3])
    frac = np.abs(W[a:b] - np.round(W[a:b]))
    assert per[2]["split"] >= 3 and (frac > 1e-4).any(), "no read of gap 2's near-repeat has a second placement that carries weight"
    assert (~far[on]).sum() <= 0.02 * on.sum()
    R, (Wr, Er, phr, _, perr) = hand_rowgroups
    a, b = int(R.str_off[4]), int(R.str_off[5])
    assert R.state[4] == 1 and not perr[4]["hit"].any() and (Wr[a:b] == 0).all() and (Er[a:b] == 0).all() and (Wr[:a].sum(axis=1) > 0).all()
    assert sum(r["cut"] for r in perr.values()) > 0 and sum(r["part"] for r in perr.values()) > 20
    assert set(phr[a:b]) <= {0, 1} and (phr[a:b] == 1).any()      # the uniform prior: perr = 3 / 4 under a called base
    print(f"columns within 1e-3 of a rounding boundary: {int((~far[on]).sum())} of {int(on.sum())}")


def test_an_ambiguous_read_lowers_the_phred(hand_ambiguous):
    """The low-coverage repeat: the reads that fit both copies carry half their weight on each, the reads over the differing base
    all of it on one; where a column's only evidence is a read that could lie elsewhere too, the soft Phred is below the Phred
    that takes the drawn placement as given -- and above it under the other copy, which the drawn placement leaves bare."""
    H, (W, E, ph, far, per) = hand_ambiguous
    tabs = place_tables(H.model.cstruct())
    best = []
    for k in range(4):
        o, Lr = read_scores(H.S[0], 64, H.seqs[k], 0, H.pos[k], int(H.starts[0]), G0, tabs)
        assert len(o) == 64 + 14
        p = weights(o, Lr)[0]
        best.append(sorted(zip(p, o), reverse=True)[:2])
    for k, o1 in ((0, 0), (1, 5)):
        assert {best[k][0][1], best[k][1][1]} == {o1, o1 + 32} and abs(best[k][0][0] - 0.5) < 1e-6 and abs(best[k][1][0] - 0.5) < 1e-6
    assert best[2][0][1] == 16 and best[3][0][1] == 49 and best[2][0][0] > 0.99 and best[3][0][0] > 0.99
    hard = tbq.phred_of(hard_quality(H, 0), H.raw)
    assert (ph[:5] < hard[:5]).all() and (hard[:5] > 20).all() and (ph[:5] > 0).all() and (ph[32:37] > hard[32:37]).all() and (hard[32:37] == 1).all()
    assert (~far).sum() <= 0.02 * 64
    assert abs(W[0].sum() - 0.5) < 1e-6 and abs(W[32].sum() - 0.5) < 1e-6 and abs(W[60].sum() - 1.0) < 1e-3     # (a one-substitution placement of another read lends column 60 1.5e-4)


def test_other_cases_stay_under_the_cap(hand_edge, hand_rowgroups):
    """The 2 % cap of the Phred comparison holds for the restatement of the edge-length and the row-group cases too."""
    for H, (W, E, ph, far, per) in (hand_edge, hand_rowgroups):
        on = on_columns(H.state, H.filled_len)
        assert (~far[on]).sum() <= 0.02 * on.sum() and (W[on].sum(axis=1) > 0).any()
    H = hand_rowgroups[0]
    assert [int(H.u_off[g + 1] - H.u_off[g]) for g in range(4)] == list(ROWGROUP_READS) and len(H.gaps) == 5


def test_kernel_arithmetic_on_the_cpu(hand, hand_edge, column_program, tmp_path):
    """The functions fig_softqual_kernel calls -- the weight of one placement, one column against one read's row of weights --
    compiled as plain C++ into a program of its own with AddressSanitizer and UBSan (tests/softqual_column_main.cpp; run
    directly), over the hand-made case and the edge-length case: both planes against the restatement at the module's bar."""
    for name, (H, (W, E, ph, far, per)) in (("hand", hand), ("edge", hand_edge)):
        d = tmp_path / name; d.mkdir()
        gw, ge, cols = run_program(column_program, H, d)
        compare_planes(gw, W[cols], f"{name}: wcount"); compare_planes(ge, E[cols], f"{name}: eloglik")


def dyadic_planes(H, g):
    """the planes of gap g with the weight of valid placement o of read r replaced as tests/softqual_column_main.cpp replaces it,
    added in the kernel's order (reads ascending, j ascending) in doubles"""
    tabs = place_tables(H.model.cstruct())
    n = int(H.filled_len[g])
    Wc = np.zeros((n, 4)); El = np.zeros((n, 4))
    x = np.arange(n)
    for r, k in enumerate(range(int(H.u_off[g]), int(H.u_off[g + 1]))):
        if H.draw_pos[k] == INT_MIN:
            continue
        seq, rev = H.seqs[k], int(H.rev[k])
        o, Lr = read_scores(H.S[g], n, seq, rev, H.pos[k], int(H.starts[g]), G0, tabs)
        if weights(o, Lr) is None:
            continue
        ln = len(seq)
        row = np.zeros(n + ln - 1)
        row[o + ln - 1] = np.where((o + 1000 + 2 * r) % 3 == 0, 0.0, 1.0 / (1 << ((o + 1000 + r) % 4)))
        acgt, s, t = read_terms(seq, rev, tabs)
        for j in range(ln):
            if not acgt[j]:
                continue
            p = row[x - j + ln - 1]
            m = p != 0
            Wc[m, s[j]] = Wc[m, s[j]] + p[m]
            for b in range(4):
                El[m, b] = El[m, b] + p[m] * t[j, b]
    return Wc, El


def test_exact_weights_give_exact_planes(hand_edge, hand_rowgroups, column_program, tmp_path):
    """With every weight a power of two (or 0.0) the products are exact and the order of the additions is the kernel's: the planes
    of the stand-alone program equal a sequential restatement bit for bit."""
    for name, (H, _) in (("edge", hand_edge), ("rowgroups", hand_rowgroups)):
        d = tmp_path / name; d.mkdir()
        gw, ge, cols = run_program(column_program, H, d, "dyadic")
        want = [dyadic_planes(H, g) for g in range(len(H.gaps))]
        Wc = np.concatenate([w[0] for w in want]); El = np.concatenate([w[1] for w in want])
        assert tbq.same_bits(gw, Wc[cols]) and tbq.same_bits(ge, El[cols]) and (Wc > 0).any()
        assert name == "edge" or (np.isfinite(El) & (El != 0)).sum() > 100       # (the edge case's model has zeros: -inf in every entry)


# ------------------------------------------------------------------------------------- GPU
def _filled(H):
    r = api.FigGapResults()
    r.filled_len = api._p(H.filled_len, api.c_i32_p); r.str_off = api._p(H.str_off, api.c_i64_p)
    r.str = C.cast(H.raw.ctypes.data, C.c_char_p); r.str_capacity = len(H.raw)
    r.draw_pos = api._p(H.draw_pos, api.c_i32_p); r.draw_isz = api._p(H.draw_isz, api.c_i32_p); r.draw_len = api._p(H.draw_len, api.c_i32_p)
    return r


def _softqual_raw(eng, H, origin):
    """fig_batch_softqual through ctypes, no placement asked for, the caller's buffers filled with 0xFF bytes before the call"""
    r = _filled(H)
    total = max(int(H.str_off[-1]), 1)
    wc = np.zeros((total, 4)); wc.view(np.uint8)[...] = 0xFF
    el = np.zeros((total, 4)); el.view(np.uint8)[...] = 0xFF
    ph = np.full(total, 0xFF, dtype=np.uint8); st = np.full(len(H.gaps), 0xFF, dtype=np.uint8)
    sq = api.FigGapSoftqual(); sq.wcount = api._p(wc, api.c_double_p); sq.eloglik = api._p(el, api.c_double_p); sq.phred = api._p(ph, api.c_u8_p); sq.state = api._p(st, api.c_u8_p)
    rc = eng.lib.fig_batch_softqual(eng.ctx, C.byref(r), api._p(origin, api.c_i32_p) if origin is not None else None, None, C.byref(sq))
    return rc, api.SoftQual(wc, el, ph, st)


def check_against(H, Q, want, what):
    W, E, ph, far, per = want
    on = on_columns(H.state, H.filled_len)
    assert list(Q.state) == list(H.state), what
    r1 = compare_planes(Q.wcount, W, f"{what}: wcount"); r2 = compare_planes(Q.eloglik, E, f"{what}: eloglik")
    compare_phred(Q.phred, Q.eloglik, H.raw, on, ph, far)
    return max(r1, r2)


def on_device(H, fn):
    eng = api.Engine(0)
    try:
        eng.set_model(H.model)
        eng.upload(H.batch)
        return fn(eng)
    finally:
        eng.close()


@pytest.mark.gpu
def test_hand_made_batch(hand):
    """fig_batch_softqual on the resident hand-made batch, no fill: n = 1 / 65 / 257 / 600 / 12 / 300 (one column, the column-block
    edges 256 / 257, three blocks), 3 / 70 / 130 / 40 reads (the read-chunk edges 64 / 65 and 128 / 130), both anchor sides and
    orientations, N in reads, flanks and string, gaps beyond the contig ends, undrawn reads, reads drawn at invalid offsets, off
    gaps.  All planes at the bar over buffers that came in as 0xFF bytes; the Python face gives the same bytes; the placement
    handed over by the same call equals fig_batch_placement's field by field, bit for bit; without origins the ORIGINAL gap is on
    too; |o*| = 2^20 in a gap that is on and a freed batch are FIG_EINVAL."""
    H, want = hand

    def body(eng):
        rc, Q = _softqual_raw(eng, H, H.origin)
        assert rc == 0
        check_against(H, Q, want, "hand")
        Q2 = eng.softqual(H.result(), H.origin, placement=True)
        assert tbq.same_bits(Q2.wcount, Q.wcount) and tbq.same_bits(Q2.eloglik, Q.eloglik) and np.array_equal(Q2.phred, Q.phred) and np.array_equal(Q2.state, Q.state)
        P = eng.placement(H.result(), H.origin)
        for f in ("ll_drawn", "ll_other", "sum_other"):
            assert tbq.same_bits(getattr(Q2.placement, f), getattr(P, f)), f
        for f in ("off_other", "n_valid", "pq", "state"):
            assert np.array_equal(getattr(Q2.placement, f), getattr(P, f)), f
        assert (P.pq != 255).any() and P.state.any()
        rc, Q3 = _softqual_raw(eng, H, None)
        assert rc == 0 and list(Q3.state) == [1, 1, 1, 1, 1, 0, 0, 1, 1]
        keep = np.ones(len(H.raw), dtype=bool); keep[int(H.str_off[4]):int(H.str_off[5])] = False
        assert tbq.same_bits(Q3.eloglik[keep], Q.eloglik[keep]) and (Q3.wcount[~keep] > 0).any()
        for k, v, want_rc in ((int(H.u_off[2]) + 1, 1 << 20, -1), (int(H.u_off[2]) + 1, (1 << 20) - 1, 0), (int(H.u_off[6]) + 1, 1 << 20, 0)):
            B = HandPlace()
            B.draw_pos[k] = v
            assert _softqual_raw(eng, B, B.origin)[0] == want_rc, (k, v)
        eng.free_batch()
        assert _softqual_raw(eng, H, H.origin)[0] == -1
    on_device(H, body)
    assert "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_row_group_edges(hand_rowgroups):
    """Four gaps of 40 columns with RG-1, RG, RG+1 and 2 RG+1 reads, and a gap that is on with no drawn read (all 0.0, Phred 1
    under a called base)."""
    H, want = hand_rowgroups
    rc, Q = on_device(H, lambda eng: _softqual_raw(eng, H, H.origin))
    assert rc == 0
    check_against(H, Q, want, "row groups")


@pytest.mark.gpu
def test_ambiguous_reads_on_the_device(hand_ambiguous):
    """The low-coverage repeat on the device: the planes at the bar, and the soft Phred below fig_batch_quality's on the columns whose
    only evidence is a read that fits both copies (and above it under the other copy)."""
    H, want = hand_ambiguous

    def body(eng):
        rc, Q = _softqual_raw(eng, H, H.origin)
        return rc, Q, eng.quality(H.result(), H.origin)[1]
    rc, Q, hard = on_device(H, body)
    assert rc == 0
    check_against(H, Q, want, "ambiguous")
    assert (Q.phred[:5] < hard[:5]).all() and (Q.phred[32:37] > hard[32:37]).all()


@pytest.mark.gpu
def test_edge_lengths_on_the_device(hand_edge):
    """Read lengths 1, 16, 17, 32, 33, 199; 65 reads; 40 columns; the first read of every length ends in an N."""
    H, want = hand_edge
    rc, Q = on_device(H, lambda eng: _softqual_raw(eng, H, H.origin))
    assert rc == 0
    check_against(H, Q, want, "edge lengths")


@pytest.mark.gpu
def test_degenerate_posterior_is_the_hard_quality():
    """A model with Tmin == Tmax and no zero entry: every read has at most one valid placement, and every read that has one is drawn
    there (the others are not drawn).  Then p = 1: eloglik equals fig_batch_quality's loglik bit for bit, wcount the A..T columns
    of the integer pile-up exactly, phred the quality's."""
    T0 = 600
    H = HandPlace(seed=20261022, gaps=[(65, 70, 0, "u", 65, F_, ""), (257, 130, 0, "u", 257, F_, ""), (300, 20, 0, "u", 300, F_, "")], state=[1, 1, 1])
    m = H.model
    m.e[17] = 0.0123; m.T[1 * 5 + 2] = 0.05; m.insd[500] = 1.0 / 1200
    m.Tmin = m.Tmax = T0
    pile = np.zeros((len(H.raw), 4))
    drawn = 0
    for g in range(len(H.gaps)):
        n, st = int(H.filled_len[g]), int(H.starts[g])
        for k in range(int(H.u_off[g]), int(H.u_off[g + 1])):
            ln = len(H.seqs[k])
            o = T0 - (st - H.pos[k] + ln) if H.pos[k] < st else H.pos[k] + (n - G0) - st + ln - T0
            if not -(ln - 1) <= o <= n - 1:
                H.draw_pos[k] = INT_MIN
                continue
            assert int(isz_of(H.pos[k], st, G0, n, ln, o)) == T0
            H.draw_pos[k] = o; drawn += 1
            x = o + np.arange(ln); s = CODE[H.seqs[k]]
            ok = (x >= 0) & (x < n) & (s < 4)
            np.add.at(pile, (int(H.str_off[g]) + x[ok], s[ok]), 1.0)
    assert drawn > 40

    def body(eng):
        rc, Q = _softqual_raw(eng, H, H.origin)
        ll, ph, st = eng.quality(H.result(), H.origin)
        return rc, Q, ll, ph, st
    rc, Q, ll, ph, st = on_device(H, body)
    assert rc == 0 and list(Q.state) == [1, 1, 1] == list(st)
    assert tbq.same_bits(Q.eloglik, ll) and (ll != 0).any()
    assert tbq.same_bits(Q.wcount, pile) and pile.sum() > 1000
    assert np.array_equal(Q.phred, ph)


@pytest.mark.gpu
def test_tandem_gap(hand):
    """The period-12 gap (n = 12, exact copies, a flat insert-size table): a read lies on each of its c copies a multiple of 12 away
    with weight 1 / c, so the weight on column x sums to sum_r (copies of r covering x) / c_r within 1e-6, and at least 1 - 1e-6 of
    every column's weight sits on the emitted base."""
    H, _ = hand
    rc, Q = on_device(H, lambda eng: _softqual_raw(eng, H, H.origin))
    assert rc == 0
    g = [i for i in range(len(GAPS)) if GAPS[i][6] == "tandem"][0]
    n, a = GAPS[g][0], int(H.str_off[g])
    want = np.zeros(n)
    for k in range(int(H.u_off[g]), int(H.u_off[g + 1])):
        ln, o = len(H.seqs[k]), int(H.draw_pos[k])
        copies = [c for c in range(-(ln - 1), n) if (c - o) % 12 == 0]
        for x in range(n):
            want[x] += sum(1 for c in copies if c <= x <= c + ln - 1) / len(copies)
    tot = Q.wcount[a:a + n].sum(axis=1)
    assert (want > 1).all() and np.abs(tot - want).max() < 1e-6
    called = Q.wcount[a:a + n][np.arange(n), CODE[H.raw[a:a + n]]]
    assert (called >= (1 - 1e-6) * tot).all()


@pytest.mark.gpu
def test_partial_mode_model_launches_nothing(monkeypatch, capfd):
    """The same batch under a partial-mode model: every gap is off, the planes are all 0.0 and the Phred all 0 over poisoned
    buffers, and the [figsoftq] line shows 0 gaps and no kernel time."""
    monkeypatch.setenv("FIG_SCHED_LOG", "1")
    H = HandPlace(mode="partial")
    rc, Q = on_device(H, lambda eng: _softqual_raw(eng, H, H.origin))
    err = capfd.readouterr().err
    assert rc == 0 and not Q.state.any() and (Q.wcount == 0).all() and (Q.eloglik == 0).all() and (Q.phred == 0).all()
    line = [ln for ln in err.splitlines() if ln.startswith("[figsoftq]")]
    assert len(line) == 1 and re.match(r"\[figsoftq\] gaps on 0 of 9, columns 0, reads 0, active placements 0, placement kernel 0\.000 ms, softqual kernel 0\.000 ms$", line[0]), line


def run_golden_softqual(root):
    """A golden filled as figfill fills it with softqual=True while the batch is resident, then a second plain fill -> Fill with
    .Q, .second and what the restatement needs"""
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
            res = eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True, softqual=True, keep_resident=True)
            F.second = _take(Fill(), eng.fill_struct(cb, nu, int(sp.value), draw=True, resident=True, support=True), n)
        finally:
            eng.close()
        _take(F, res, n)
        F.Q = res.softqual
        return F
    finally:
        host.fighost_run_close(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "bench_b160"])
def test_goldens_end_to_end(name, tmp_path):
    """A golden filled through api with softqual=True: states by the rule, both planes against the restatement at the bar, the
    Phred as defined; a fill of the still resident batch afterwards returns identical bytes."""
    F = run_golden_softqual(util.extract_golden(name, str(tmp_path)))
    assert F.unmapped
    total = int(F.str_off[F.n])
    W = np.zeros((total, 4)); E = np.zeros((total, 4)); ph = np.zeros(total, dtype=np.uint8); far = np.ones(total, dtype=bool)
    state = np.zeros(F.n, dtype=np.uint8)
    for g in range(F.n):
        n = int(F.filled_len[g]); org = int(F.origin[g])
        state[g] = n > 0 and int(F.draw_len[2 * g]) == n and int(F.draw_len[2 * g + 1]) < 0 and bool(org & api.SUP_FINAL) and not org & api.SUP_ORIGINAL
        if not state[g]:
            continue
        c = int(F.gap_contig[g])
        a = int(F.str_off[g])
        S = columns(F.contig[int(F.contig_off[c]):int(F.contig_off[c + 1])], int(F.start[g]), int(F.G0[g]), F.raw[a:a + n])
        reads = [(F.u_seq[int(F.u_seq_off[k]):int(F.u_seq_off[k + 1])], int(F.u_rev[k]), int(F.u_pos[k]))
                 for k in range(int(F.u_off[g]), int(F.u_off[g + 1])) if F.draw_pos[k] != INT_MIN]
        R = restate_gap(S, n, reads, int(F.start[g]), int(F.G0[g]), F.tabs)
        W[a:a + n], E[a:a + n] = R["wcount"], R["eloglik"]
        ph[a:a + n], far[a:a + n] = phred_margin(R["exact"], F.raw[a:a + n])
    assert np.array_equal(F.Q.state, state) and state.any()
    compare_planes(F.Q.wcount, W, f"{name}: wcount"); compare_planes(F.Q.eloglik, E, f"{name}: eloglik")
    compare_phred(F.Q.phred, F.Q.eloglik, F.raw, on_columns(state, F.filled_len), ph, far)
    for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len", "support", "origin"):
        assert np.array_equal(getattr(F, f), getattr(F.second, f)), f


@pytest.mark.gpu
def test_gapsoftquality_file_is_the_same_from_every_host_path(tmp_path, monkeypatch):
    """unmapped_small with FIGFILL_SOFTQUALITY=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 and two-rank figfill_mp leave
    the same gapsoftquality.txt, in gapquality.txt's format; the reference's files stay byte-identical in every run; without the
    variable no such file appears, and gapquality.txt, gapplacement.txt and gapsupport.txt are the bytes they are with it."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    name = "unmapped_small"
    for v in ("FIGFILL_SUPPORT", "FIGFILL_QUALITY", "FIGFILL_PLACEMENT", "FIGFILL_QUALITY_MINPQ", "FIGFILL_SOFTQUALITY"):
        monkeypatch.delenv(v, raising=False)
    roots = [util.extract_golden(name, str(tmp_path / f"r{k}")) for k in range(6)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    others = {"FIGFILL_QUALITY": "1", "FIGFILL_PLACEMENT": "1", "FIGFILL_SUPPORT": "1"}
    runs = [(roots[0], {"FIGFILL_SOFTQUALITY": "1"}), (roots[1], {"FIGFILL_SOFTQUALITY": "1", "FIGFILL_DEVICES": "0,0"}), (roots[3], {}),
            (roots[4], others), (roots[5], dict(others, FIGFILL_SOFTQUALITY="1"))]
    for root, env in runs:
        r = util.run([util.FIGFILL] + argv, root, env)
        assert r.returncode == 0, r.stderr
    monkeypatch.setenv("FIGFILL_SOFTQUALITY", "1")                          # the spawned ranks inherit it
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
    files = [util.read(os.path.join(root, "tmp", "gapsoftquality.txt")) for root in (roots[0], roots[1], roots[2], roots[5])]
    assert files[0] == files[1] == files[2] == files[3]
    exp = _gapout(roots[0])
    lines = files[0].splitlines()
    assert len(lines) == len(exp)
    for ln, e in zip(lines, exp):
        f = ln.split("\t")
        assert len(f) == 7 and f[:5] == e[:5] and f[5] in "01" and len(f[6]) == max(int(f[4]), 0) and (f[5] == "1" or set(f[6]) <= {"!"})
    assert any(ln.split("\t")[5] == "1" for ln in lines)
    side = ("gapquality.txt", "gapplacement.txt", "gapsupport.txt")
    for k, root in enumerate(roots):
        assert os.path.exists(os.path.join(root, "tmp", "gapsoftquality.txt")) == (k in (0, 1, 2, 5))
        for fn in side:
            assert os.path.exists(os.path.join(root, "tmp", fn)) == (k in (4, 5)), (k, fn)
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
    for fn in side:
        assert util.read(os.path.join(roots[4], "tmp", fn)) == util.read(os.path.join(roots[5], "tmp", fn)), fn
