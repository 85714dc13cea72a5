"""The search paths of the MLE pass (fig_hot_mle, figbird_amd/csrc/fig_engine_hot.h) on directed cases against the oracle.

The pass prunes: hints, a record sweep and deferred survivors in its lane-per-read path; a swept filter, pair-chain rounds with
a survivor hand-over or a plain chain in its wave-per-read path; two copies of the accept test and pile-up; four memory forms
behind fig_mle_dispatch.  The oracle is the full scan in the reference's order, so every case is compared with it, and the
cases (tools/mle_cases.py) are built so that a read's maximum is not simply its hint: gaps inside tandem repeats, where
placements one period apart have bit-equal products and "first maximum wins" decides.

Per case one oracle run (Figbird.cpp-main mode, level-3 trace) and one fill through the C ABI with the candidate records,
both planes and the draw planes on.  compare_with_oracle (tests/test_estep_forms.py): strings, filled_len, gaptofill and
candidate records exact; likelihood and both planes at 0 with the emulation and at the parity contract's 1e-6 on the device;
placeReads calls and algorithmic flops equal.  compare_draw: the finalize pass's arg-max of every read -- position and
insert size of each drawn read, and which reads are not drawn -- equals the oracle's draw file.

Evidence that a path ran: the static routing predicate of every read (tools/mle_cases.route), the restated memory-form
predicates (tools/mle_cases.mle_form) on the class the library logs, the ratio mle_exec_flops / mle_alg_flops (printed for
every case; asserted below 1 only where the mismatch filter applies to every candidate under a sharp model), and one
not-vacuous test per dimension on the oracle's own outputs.

The non-monotone marker (fig_model_fmm = 2.0) is reached from a myout.sam (case e_nonmono: a deletion in front of, and a
substitution at, the same read position of every model pair), so it is compared with the oracle like every other case; no model
is injected through set_model_struct.

Memory forms (lds, use_serial, nci_lds, use_kf) the cases reach, and those they cannot: see FORMS_EXPECTED.

MEASURED on an MI355X (mle_exec_flops / mle_alg_flops, default schedule; * = asserted below 1, the filter being sharp there):
  a  p7 0.0899*  p20 0.0426*  p20_e8 0.0507*  p40 0.0220*  p50 0.0289*
  b  L31 0.1143*  L32 0.1004*  L33 0.0973*  L47 0.0488*  L48 0.0533*  L49 0.0518*  L63 0.0420*  L64 0.0408*  L65 0.0398*  short 0.0423*
  c  slot0 0.0564*  slot31 0.0559*  slot32 0.0574*  rowgroup 0.1014*  chunk1 0.4836*  last 0.0568*  all 1.0000 (plain chain only)
     t_63 0.0599*  t_64 0.0575*  t_65 0.0594*  w256_1 0.0631*  w256_255 0.1801*  w256_256 0.1797*  w256_257 0.1788*
     w512_511 0.1841*  w512_512 0.1848*  w512_513 0.1910*
  d  12 0.5362*  20 0.5836*  30 0.6176*   (72-to-112-column classes: no factor buffers, so reads without a hint take the whole chain)
  e  e005 0.1538*  e08 0.1409*  e30 0.2223  e60 1.0068  e85 1.0072  denorm 1.0075  nonmono 1.0104   (above 1: the hint is evaluated twice)
  f  lds 0.1470*  1250 0.0984*  1400_L200 0.8024* (no factor buffers)  tiled 0.2451*  slab 0.9567 (fig_hot_mle<false>: prefix pruning only)
     lds_e85 0.9326  1250_e85 0.9589  1400_L200_e85 0.9594  short_e85 1.0165
  FIG_SCHED=seq: the same figures to the fourth decimal, except b_L63 0.0379, b_L64 0.0355, b_L65 0.0333 and a_p50 0.0290 (results
  identical; presumably the hints a candidate's first pass starts from differ between the schedules -- not examined).
"""
import os
import re

import numpy as np
import pytest

import util
from figbird_amd import api, synth
from tools import estep_cases as ec
from tools import mle_cases as mc
from test_estep_forms import _CLASS_RE, compare_with_oracle
from test_planes import model_of, parse_planes, prepare

CASES = mc.all_cases()
CPU_IDS = [c for c in CASES if c not in mc.FORM_IDS]             # f: form-only, means nothing without the device's class geometry
SEQ_IDS = mc.TANDEM_IDS + mc.POPULATION_IDS
INT_MIN = np.iinfo(np.int32).min
SHARP_FMM = 0.05                                                 # models up to 8 % error here: a mismatch costs at least a factor 20

_DRAW_HDR = re.compile(r"^ *=+\+Gap = (\d+) starting,length = (-?\d+)=+$")
_DRAW_READ = re.compile(r"^ *([A-Za-z]+)\[(\d+) (-?\d+) isz = (-?\d+) ([IEP])\]$")
_ORACLE = {}


def parse_draw(path):
    """The oracle's draw file -> {gap: (header length, {read number: (offset, insert size)})} of the last block of each gap."""
    out, g = {}, None
    for ln in open(path):
        ln = ln.rstrip("\n")
        m = _DRAW_HDR.match(ln)
        if m:
            g = int(m.group(1))
            out[g] = (int(m.group(2)), {})
            continue
        m = _DRAW_READ.match(ln)
        if m:
            assert g is not None and m.group(5) != "P"
            out[g][1][int(m.group(2))] = (int(m.group(3)), int(m.group(4)))
    return out


def oracle_of(cid, tmp_path_factory):
    """As test_estep_forms.oracle_of, on the cases of tools/mle_cases.py and with the draw file: computed once per case id and shared
    (read-only)."""
    if cid not in _ORACLE:
        base = tmp_path_factory.mktemp("mle_" + cid)
        root, case = prepare(CASES[cid](), base)
        tr = os.path.join(str(base), "o.trace")
        r = util.run_oracle_figbird(root, trace=tr, level=3)
        assert r.returncode == 0, r.stderr
        cands, _ = util.parse_trace(tr)
        stats = [ln.rstrip("\n").split("\t")[1:3] for ln in open(tr) if ln.startswith("STATS")]
        gapout = [ln.split("\t") for ln in util.read(os.path.join(root, "tmp", "gapout0.txt")).splitlines()]
        gtf = [int(x) for x in util.read(os.path.join(root, "tmp", "gaptofill0.txt")).split()]
        assert len(gapout) == len(case.gaps) == len(gtf) and len(stats) == 1
        model = model_of(root)
        _ORACLE[cid] = dict(case=case, root=root, model=model, fmm=mc.model_fmm(model), cands=cands, planes=parse_planes(tr), gapout=gapout, gaptofill=gtf,
                            place_calls=int(stats[0][0]), flops=float(stats[0][1]), draw=parse_draw(os.path.join(root, "tmp", "draw0.txt")))
    return _ORACLE[cid]


def fill_with_draw(lib_path, o):
    """test_planes.fill_with_planes with the draw planes on as well -> (FillResult, fig_get_stats)."""
    case, planes = o["case"], o["planes"]
    batch = synth.case_to_batch(case)
    cols = int(max([max(G for G, _, _ in v) for v in planes.values()] + [7])) + 1
    reads = int(np.diff(batch.u_read_off).max()) + 1
    eng = api.Engine(0, lib_path=lib_path)
    eng.set_model(o["model"])
    res = eng.fill(batch, debug_cand=512, plane_cols=cols, plane_reads=reads, draw=True)
    st = eng.stats()
    eng.close()
    return res, st


def compare(o, res, st, tol):
    """test_estep_forms.compare_with_oracle; for a case whose candidate loop the oracle never starts (no CAND record, so no plane
    either) what is left of it: lengths, strings, gaptofill, no candidate record, placeReads calls and algorithmic flops."""
    if o["cands"]:
        return compare_with_oracle(o, res, st, tol)
    assert [int(e[4]) for e in o["gapout"]] == list(res.filled_len) and [e[5] if len(e) > 5 else "" for e in o["gapout"]] == res.strings
    assert o["gaptofill"] == list(res.gaptofill) and all(len(c) == 0 for c in res.cand)
    assert st["place_calls"] == o["place_calls"] and st["alg_flops"] == o["flops"]


def compare_draw(o, res):
    """The draw planes against the oracle's draw file, read by read: the finalize pass's arg-max (offset and insert size) of every
    drawn read, INT32_MIN for every other, the header length per gap.  -> reads compared."""
    dpos, disz, dlen = res.draw
    n = 0
    for g, gap in enumerate(o["case"].gaps):
        base = sum(len(x.unmapped) for x in o["case"].gaps[:g])
        hl, reads = o["draw"].get(g, (-1, {}))
        assert int(dlen[2 * g]) == hl and int(dlen[2 * g + 1]) == -1, f"gap {g}: draw header {int(dlen[2 * g])} vs {hl}"
        for k in range(len(gap.unmapped)):
            if k in reads:
                assert (int(dpos[base + k]), int(disz[base + k])) == reads[k], f"gap {g} read {k}: drawn at {int(dpos[base + k])} isz {int(disz[base + k])}, oracle {reads[k]}"
                n += 1
            else:
                assert int(dpos[base + k]) == INT_MIN, f"gap {g} read {k}: drawn at {int(dpos[base + k])}, not drawn by the oracle"
    return n


def forms_of(o, classes, emu=False):
    """{(gap, G): mle_form} of every candidate the oracle evaluated, on the classes given (restated or read from the log); for a gap
    whose candidate loop it never started, of the probes of checkGapReads instead (all of them ran, each an MLE pass)."""
    case, out = o["case"], {}
    _, cls_of = mc.classes_of(case)
    for g, gap in enumerate(case.gaps):
        cl = classes[cls_of[g]]
        for G in sorted(set(c[0] for c in o["cands"][g])) if g in o["cands"] else mc.probe_lengths(gap.length):
            out[(g, G)] = mc.mle_form(mc.emu_class(cl) if emu else cl, G, o["fmm"])
    return out


def filter_is_sharp(o, forms):
    """The filter applies to most candidates (use_kf: packed consensus in LDS, so the lane path runs) under a model whose mismatch
    factors are at most SHARP_FMM, and most reads are of the model's length without N: there mle_exec_flops < mle_alg_flops.  (A
    pass without the filter costs at most its algorithmic flops plus the hints evaluated twice, a pass with it a small fraction;
    so with the filter on more than half of the candidates the sum stays below.)"""
    routes = [mc.route(r, o["case"].read_len) for g in o["case"].gaps for r in g.unmapped]
    return o["fmm"] <= SHARP_FMM and 2 * sum(f["use_kf"] for f in forms.values()) > len(forms) and 2 * routes.count("lane") > len(routes)


def report_ratio(cid, o, st, forms, where):
    ratio = st["mle_exec_flops"] / st["mle_alg_flops"] if st["mle_alg_flops"] else float("nan")
    sharp = filter_is_sharp(o, forms)
    print(f"{where} {cid}: mle_exec_flops / mle_alg_flops = {st['mle_exec_flops']:.0f} / {st['mle_alg_flops']:.0f} = {ratio:.4f} (fmm {o['fmm']:.4g}, filter sharp: {sharp})")
    if sharp:
        assert st["mle_exec_flops"] < st["mle_alg_flops"], f"{cid}: the pruning saved nothing where the filter applies"


def final_sequence(o, g):
    """(S, origin): the scaffold with the oracle's string in gap g; column x of the gap is S[origin + x]."""
    case, gap, e = o["case"], o["case"].gaps[g], o["gapout"][g]
    s = case.scaffolds[0]
    return s[:gap.start] + (e[5] if len(e) > 5 else "") + s[gap.start + gap.length:], gap.start


def twins(o, g, period):
    """Per drawn read of gap g whose draw header is the filled length: (read, offset, number of placements k periods away, k != 0,
    inside the read's window, at which the final sequence reads exactly as at the drawn placement) -- the ties the search must
    break towards the first maximum.  Also checks the restated window on the oracle's own draws."""
    case, gap = o["case"], o["case"].gaps[g]
    hl, reads = o["draw"].get(g, (-1, {}))
    if hl != int(o["gapout"][g][4]):
        return []
    S, org = final_sequence(o, g)
    out = []
    for k, (pos, _) in sorted(reads.items()):
        r = gap.unmapped[k]
        n = len(r.mate_seq_fastq)
        lo, hi = mc.window(o["model"], r.anchor_pos1, gap.start, hl, n, hl - gap.length)
        assert lo <= pos <= hi, f"gap {g} read {k}: drawn at {pos} outside the restated window {lo} .. {hi}"
        here = S[org + pos:org + pos + n]
        cnt = sum(1 for q in range(lo, hi + 1) if q != pos and (q - pos) % period == 0 and org + q >= 0 and S[org + q:org + q + n] == here)
        out.append((k, pos, cnt))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_predicates_restated_switch_where_the_code_says():
    """tools/mle_cases.mle_form against fig_engine_hot.h:979-996 and :1571-1572 by hand, on classes of fig_pack.h's table."""
    cl = lambda gm, L: mc.with_tile_cols(mc.pc.class_table([gm], L)[0][0], L)
    f = lambda gm, L, G, fmm=0.005: tuple(int(mc.mle_form(cl(gm, L), G, fmm)[k]) for k in ("lds", "use_serial", "nci_lds", "use_kf"))
    # 256 threads, 4 rows of (capGl + L) doubles against 4 factor buffers of 208
    assert f(324, 36, 120) == (1, 1, 1, 1)
    assert f(405, 36, 405) == (1, 1, 0, 1)                  # 4 * 448 - 832 = 960 < (5 * 405 + 1) / 2 + 1 = 1014
    assert f(405, 36, 350) == (1, 1, 1, 1)                  # pile-up of 876 doubles, 84 left for the 30 + 16 + 1 words
    assert f(405, 36, 381) == (1, 1, 1, 0) and f(405, 36, 384) == (1, 1, 0, 1)       # pile-up of 954 fits and leaves 6 | 961 does not fit
    assert f(108, 36, 20) == (1, 0, 1, 1)                   # 4 * 152 = 608 < 832: no factor buffers
    assert f(180, 31, 60) == (1, 1, 0, 0)                   # 864 - 832 = 32 doubles left: no room for 16 + 16 + 1 words
    assert f(324, 36, 120, 0.5) == (1, 1, 1, 0) and f(324, 36, 120, 0.4999) == (1, 1, 1, 1) and f(324, 36, 120, 2.0) == (1, 1, 1, 0)
    # 512 threads: 8 buffers = 1664 doubles; the 1217-1600 class at L = 200 has one row of 1600
    assert cl(1400, 200)["nteams"] == 1 and f(1400, 200, 1400) == (1, 0, 0, 1) and f(1400, 200, 1400, 0.9) == (1, 0, 0, 0)
    assert cl(1250, 36)["nteams"] == 4 and f(1250, 36, 1250) == (1, 1, 1, 1)
    # tiled class: LDS form while 7 ncolE + 1664 + words + 24 fits in front of FigState
    assert cl(2000, 36)["tiles"] >= 2 and f(2000, 36, 2000) == (1, 1, 0, 1)
    assert cl(2600, 36)["tiles"] >= 2 and f(2600, 36, 2600) == (0, 1, 0, 0)
    # the emulation: one lane, one row
    fe = lambda gm, L, G: mc.mle_form(mc.emu_class(cl(gm, L)), G, 0.005)["lane_path"]
    assert fe(324, 36, 120) and fe(108, 36, 20) and not fe(180, 31, 60) and fe(424, 31, 60)
    assert mc.gmax_unmapped(120, 36) == 324 and mc.gmax_unmapped(20, 36) == 108 and mc.gmax_unmapped(405, 36) == 405 and mc.gmax_unmapped(200, 36) == 600
    assert mc.candidate_range(120, 36) == (36, 108) and mc.candidate_range(405, 36) == (405, 405)


def test_cases_cover_the_routes_and_models_they_are_named_for(tmp_path_factory):
    """The static side of every dimension: both orientations in every tandem gap; short reads of both orientations in b_short; reads
    with N in the slots named, beside full-length ones (except `all`); the models' fig_model_fmm on the sides of 0.5 and 1 the
    cases are named for; the denormal case's best possible product below 1e-290 and above 0."""
    for cid in mc.TANDEM_IDS + [f"d_{g}" for g in mc.D_GAPS]:
        g = CASES[cid]().gaps[0]
        assert any(r.anchor_reverse for r in g.unmapped) and any(not r.anchor_reverse for r in g.unmapped), cid
    c = CASES["b_short"]()
    short = [r for r in c.gaps[0].unmapped if mc.route(r, 36) == "wave"]
    assert len(short) == len(mc.B_SHORT) and {r.anchor_reverse for r in short} == {True, False} and min(len(r.mate_seq_fastq) for r in short) == 20
    for w, slots in ec.N_SLOTS.items():
        routes = [mc.route(r, 36) for r in CASES[f"c_{w}"]().gaps[0].unmapped]
        assert [k for k, x in enumerate(routes) if x == "chain"] == slots and routes.count("lane") == 70 - len(set(slots) | set(mc.C_SHORT))
    for kind, (g0, ns) in mc.C_COUNTS.items():
        for n in ns:
            c = CASES[f"c_{kind}_{n}"]()
            assert len(c.gaps[0].unmapped) == n and c.gaps[0].length == g0
            assert n == 1 or mc.route(c.gaps[0].unmapped[n - 1], 36) == "chain"
    assert ec.nt_of_class(mc.gmax_unmapped(405, 36)) == 256 and ec.nt_of_class(mc.gmax_unmapped(500, 36)) == 512
    for g0 in mc.D_GAPS:
        routes = [mc.route(r, 36) for r in CASES[f"d_{g0}"]().gaps[0].unmapped]
        assert [k for k, x in enumerate(routes) if x == "chain"] == mc.D_N_SLOTS and g0 <= 30
    fmm = {cid: oracle_of(cid, tmp_path_factory)["fmm"] for cid in [f"e_{w}" for w in mc.E_RATES] + ["e_denorm", "e_nonmono"]}
    print(fmm)
    assert fmm["e_e005"] < fmm["e_e08"] <= SHARP_FMM < fmm["e_e30"] < 0.5 <= fmm["e_e60"] < fmm["e_e85"] <= 1.0
    assert fmm["e_nonmono"] == 2.0 and fmm["e_denorm"] < 0.5
    m = oracle_of("e_denorm", tmp_path_factory)["model"]
    best = float(np.prod(1.0 - m.e - m.ins - m.dele))
    print("e_denorm: product of an error-free read", best)
    assert 0.0 < best < 1e-290 and len(m.e) == 200


@pytest.mark.parametrize("cid", mc.TANDEM_IDS)
def test_tandem_cases_draw_reads_that_have_a_twin_in_their_window(cid, tmp_path_factory):
    """Not vacuous, dimensions a and b: by the oracle's own string and draw file, the tandem gap has reads drawn at a placement
    whose period-shifted twin (the same bases under the whole read) lies inside the read's window, so the drawn one won a tie
    of bit-equal products by coming first.  (p50: the period exceeds L = 36, and the tie is between copies 50 apart.)"""
    o = oracle_of(cid, tmp_path_factory)
    t = twins(o, 0, mc.period_of(cid))
    hist = {n: sum(1 for _, _, c in t if min(c, 3) == n) for n in range(4)}
    print(cid, "drawn reads by number of twins in their window (0, 1, 2, 3+):", hist)
    assert sum(hist[n] for n in (1, 2, 3)) >= 1, f"{cid}: no drawn read has a twin in its window"


def test_tandem_cases_reach_every_survivor_count(tmp_path_factory):
    """Dimension a as a whole: reads with 0, 1, 2 and at least 3 tied placements beyond the drawn one (the lane path defers at most
    two survivors per read and hands a read with more back to the wave path)."""
    seen = set()
    for cid in [f"a_{w}" for w in mc.A_TANDEMS]:
        seen |= {min(c, 3) for _, _, c in twins(oracle_of(cid, tmp_path_factory), 0, mc.period_of(cid))}
    assert seen == {0, 1, 2, 3}


def test_population_and_short_gap_cases_draw_reads_of_both_kinds(tmp_path_factory):
    """Not vacuous, dimensions c and d.  By the oracle's draw file no read with an N is drawn in any case here (seen on every case:
    the reads with N exercise the plain chain and the rejecting side of the wave path's accept copy); the accepting side of that
    copy is fed by the shorter reads, which the oracle does draw, beside the full-length reads of the lane path's copy in the
    same gap.  In the short gaps, drawn reads span the gap with more than 3 bases on either side (what sets ucoverf / umaxleftf /
    umaxrightf).  Every count case draws more than half of its reads; the one-read case and the all-N case draw none."""
    for cid in [f"c_{w}" for w in ec.N_SLOTS if w != "all"]:
        o = oracle_of(cid, tmp_path_factory)
        gap, (hl, reads) = o["case"].gaps[0], o["draw"][0]
        kinds = [mc.route(gap.unmapped[k], 36) for k in reads]
        print(cid, {k: kinds.count(k) for k in set(kinds)})
        assert set(kinds) == {"lane", "wave"}, (cid, set(kinds))
    for g0 in mc.D_GAPS:
        o = oracle_of(f"d_{g0}", tmp_path_factory)
        gap, (hl, reads) = o["case"].gaps[0], o["draw"][0]
        span = [k for k, (p, _) in reads.items() if -p > 3 and p + 36 - hl > 3]
        assert len(span) >= 10 and all(mc.route(gap.unmapped[k], 36) == "lane" for k in reads), (g0, len(span))
    for cid in ["c_t_63", "c_t_64", "c_t_65", "c_w256_255", "c_w256_256", "c_w256_257", "c_w512_511", "c_w512_512", "c_w512_513"]:
        o = oracle_of(cid, tmp_path_factory)
        assert len(o["draw"][0][1]) > len(o["case"].gaps[0].unmapped) // 2, cid
    for cid in ["c_all", "c_w256_1"]:
        o = oracle_of(cid, tmp_path_factory)
        assert len(o["draw"].get(0, (-1, {}))[1]) == 0 and max([c[3] for c in o["cands"].get(0, [])] + [0]) == 0, cid


def test_error_model_cases_place_reads(tmp_path_factory):
    """Not vacuous, dimension e: under every model from 0.5 % to 85 % the MLE pass of some candidate accepted reads (valid_count >
    0) and the finalize pass drew some.  The two degenerate models are different, and this test says so, so that a change shows:
    e_denorm's reads are evaluated (the products below 1e-290 are what the case is for) but none passes the model's cut-off, which
    is a percentile of the model pairs' own likelihoods and no self-consistent set of pairs puts it near 290; so, as under
    e_nonmono, the oracle accepts fewer than 3 reads in each probe of checkGapReads and never starts the candidate loop, and the
    case pins the passes of the probes through placeReads calls, flops and the all-N result only.  (The marker with reads placed:
    test_non_monotone_marker_injected_on_the_device_equals_the_emulation.)"""
    for cid in [f"e_{w}" for w in mc.E_RATES]:
        o = oracle_of(cid, tmp_path_factory)
        print(cid, "valid_count max", max(c[3] for c in o["cands"][0]), "drawn", len(o["draw"][0][1]))
        assert max(c[3] for c in o["cands"][0]) >= 3 and len(o["draw"][0][1]) >= 3, cid
    for cid in ("e_denorm", "e_nonmono"):
        o = oracle_of(cid, tmp_path_factory)
        assert not o["cands"] and o["place_calls"] > 0, cid


@pytest.mark.parametrize("cid", CPU_IDS)
def test_emulation_equals_oracle_exactly(cid, tmp_path_factory):
    """Dimensions a-e through the one-lane emulation (glibc, the reference's summation order): bytes, counters, planes and draw
    planes bit-identical to the oracle.  The emulation takes the lane path wherever its one weight row leaves room for the packed
    consensus (tools/mle_cases.emu_class), which is the case for every tandem case."""
    o = oracle_of(cid, tmp_path_factory)
    res, st = fill_with_draw(util.EMULIB, o)
    forms = forms_of(o, mc.classes_of(o["case"])[0], emu=True)
    print("candidates in the lane path:", sum(f["lane_path"] for f in forms.values()), "of", len(forms))
    if cid in mc.TANDEM_IDS:            # (the shortest candidates' pile-up fits the row, and then the packed consensus does not)
        assert 2 * sum(f["lane_path"] for f in forms.values()) > len(forms)
    compare(o, res, st, 0.0)
    print("reads compared with the draw file:", compare_draw(o, res))
    report_ratio(cid, o, st, forms, "emulation")


# ---------------------------------------------------------------------------------------------------------------- GPU
def _native():
    return "libfighip.so" in open("/proc/self/maps").read()


def _fill_logged(o, capfd, monkeypatch, seq=False):
    """-> (FillResult, stats, classes as dicts from the library's `[figsched] class:` lines, in the order of fig_pack.h's table)."""
    for k in ("FIG_ESTEP", "FIG_SH_CHUNKS", "FIG_SCHED"):
        monkeypatch.delenv(k, raising=False)
    if seq:
        monkeypatch.setenv("FIG_SCHED", "seq")
    monkeypatch.setenv("FIG_SCHED_LOG", "1")
    capfd.readouterr()
    res, st = fill_with_draw(None, o)
    err = capfd.readouterr().err
    assert _native()
    classes = [dict(capGl=int(m[1]), ncolE=int(m[2]), Wcap=int(m[3]), nt=int(m[4]), nteams=int(m[5]), lds_tab=int(m[6]), tiles=int(m[7])) for m in _CLASS_RE.findall(err)]
    tcols = [int(x) for x in re.findall(r"\[figsched\] class: .* tile_cols=(\d+) ", err)]
    assert classes and len(tcols) == len(classes), err[-2000:]
    return res, st, [dict(c, tile_cols=t) for c, t in zip(classes, tcols)]


def _check_on_device(cid, tmp_path_factory, capfd, monkeypatch, seq):
    o = oracle_of(cid, tmp_path_factory)
    res, st, classes = _fill_logged(o, capfd, monkeypatch, seq)
    want, _ = mc.classes_of(o["case"])
    assert classes == want, "the class table restated in tools/ differs from the library's log"
    forms = forms_of(o, classes)
    print({k: tuple(int(v) for v in f.values()) for k, f in forms.items()})
    compare(o, res, st, 1e-6)
    print("reads compared with the draw file:", compare_draw(o, res))
    report_ratio(cid, o, st, forms, "device seq" if seq else "device")
    return forms


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_device_matches_oracle(cid, tmp_path_factory, monkeypatch, capfd):
    """Every directed case on the device in the default schedule."""
    _check_on_device(cid, tmp_path_factory, capfd, monkeypatch, seq=False)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", SEQ_IDS)
def test_device_matches_oracle_in_the_sequential_schedule(cid, tmp_path_factory, monkeypatch, capfd):
    """The tandem and population cases under FIG_SCHED=seq: the same pass inside fig_fill_kernel."""
    _check_on_device(cid, tmp_path_factory, capfd, monkeypatch, seq=True)


@pytest.mark.gpu
def test_non_monotone_marker_injected_on_the_device_equals_the_emulation(tmp_path_factory, monkeypatch):
    """The marker with reads placed.  Both ways of the issue were done: e_nonmono reaches fig_model_fmm = 2.0 from a myout.sam, but
    under that model the oracle never starts its candidate loop (test_error_model_cases_place_reads); so here the model of a_p20
    gets one errorTypeProbs entry of 1.25 (outside [0, 1]: the marker) and goes to the device and to the emulation through
    fig_ctx_set_model.  No oracle knows this model; the two builds of the engine must agree: strings, lengths, gaptofill,
    candidate records, draw planes, placeReads calls and algorithmic flops bit for bit, likelihood and the two E-step planes at
    1e-6 (they pass through log / exp of the device's libm and of glibc; the MLE pass's own outputs are the integer ones).  With
    the marker nothing is pruned: mle_exec_flops >= mle_alg_flops on both."""
    import dataclasses
    from test_planes import _close
    for k in ("FIG_ESTEP", "FIG_SH_CHUNKS", "FIG_SCHED"):
        monkeypatch.delenv(k, raising=False)
    o = oracle_of("a_p20", tmp_path_factory)
    T = np.array(o["model"].T, dtype=np.float64)
    T[0 * 5 + 1] = 1.25
    m = dataclasses.replace(o["model"], T=T)
    assert mc.model_fmm(o["model"]) < 0.05 and mc.model_fmm(m) == 2.0
    o2 = dict(o, model=m, fmm=2.0)
    a, sa = fill_with_draw(util.EMULIB, o2)
    b, sb = fill_with_draw(None, o2)
    assert _native()
    assert a.strings == b.strings and list(a.filled_len) == list(b.filled_len) and list(a.gaptofill) == list(b.gaptofill)
    assert [[c[:3] for c in g] for g in a.cand] == [[c[:3] for c in g] for g in b.cand] and len(a.cand[0]) > 1
    assert max(c[2] for c in a.cand[0]) >= 3, "no read accepted under the injected model"
    for x, y in zip(a.draw, b.draw):
        assert np.array_equal(x, y)
    assert int((a.draw[0] != INT_MIN).sum()) >= 3
    assert sa["place_calls"] == sb["place_calls"] and sa["alg_flops"] == sb["alg_flops"]
    for ca, cb in zip(a.cand[0], b.cand[0]):
        assert abs(ca[3] - cb[3]) <= 1e-6 * max(1.0, abs(ca[3])) or ca[3] == cb[3], (ca, cb)
    for pa, pb in ((a.counts, b.counts), (a.read_maxlv, b.read_maxlv)):
        ok, at = _close(pa.reshape(-1), pb.reshape(-1), 1e-6)
        assert ok, (at, pa.reshape(-1)[at], pb.reshape(-1)[at])
    for what, st in (("emulation", sa), ("device", sb)):
        print(f"{what}: mle_exec_flops / mle_alg_flops = {st['mle_exec_flops'] / st['mle_alg_flops']:.4f}")
        assert st["mle_exec_flops"] >= st["mle_alg_flops"]


# (dispatch, lds, use_serial, nci_lds, use_kf) -> a case that reaches it.  dispatch: "plain" (fig_hot_mle<LDS> of an untiled class),
# "tiled-lds" (the tiled class's LDS form, one "weight row" behind the records), "tiled-slab" (the tiled class falling back to
# fig_hot_mle<false>).  These are all that can occur in the four forms:
#   * in LDS every combination of the other three occurs; the tiled class's LDS form has exactly the factor buffers, the words of
#     the packed consensus and 8 doubles behind its records (FIG_TILED_MLE_DOUBLES), so use_serial is on, the pile-up (at least
#     (5 * 1217 + 1) / 2 + 1 doubles) never fits, and use_kf follows the model alone;
#   * fig_hot_mle<false> has nci_lds and use_kf off by their `LDS &&`; use_serial off would need nteams * Wcap < 1664 doubles in a
#     class of more than 2400 columns, which has Wcap > 2400.
# Not reached: a class with neither its table in LDS nor tiles (a gap of about 10 kb at L = 36).  Its pass is the same
# fig_hot_mle<false> under the same three values as "tiled-slab"; only the first line of fig_mle_dispatch differs.
FORMS_EXPECTED = {
    ("plain", 1, 1, 1, 1): "f_1250", ("plain", 1, 1, 0, 1): "f_lds", ("plain", 1, 0, 1, 1): "d_20", ("plain", 1, 0, 0, 1): "f_1400_L200",
    ("plain", 1, 1, 1, 0): "f_1250_e85", ("plain", 1, 1, 0, 0): "f_lds_e85", ("plain", 1, 0, 1, 0): "f_short_e85", ("plain", 1, 0, 0, 0): "f_1400_L200_e85",
    ("tiled-lds", 1, 1, 0, 1): "f_tiled", ("tiled-slab", 0, 1, 0, 0): "f_slab",
}


def _dispatch(cl, f):
    return "plain" if not cl["tiles"] else ("tiled-lds" if f["lds"] else "tiled-slab")


def _reached(o, forms):
    classes, cls_of = mc.classes_of(o["case"])
    return {(_dispatch(classes[cls_of[g]], f),) + tuple(int(f[k]) for k in ("lds", "use_serial", "nci_lds", "use_kf")) for (g, G), f in forms.items()}


def test_form_cases_reach_every_memory_form_in_the_restated_class_table(tmp_path_factory):
    """FORMS_EXPECTED on the class table as tools/ restates it and the passes the oracle ran (the GPU test below repeats it on the
    library's own log)."""
    reached = {}
    for cid in sorted(set(FORMS_EXPECTED.values())):
        o = oracle_of(cid, tmp_path_factory)
        for key in _reached(o, forms_of(o, mc.classes_of(o["case"])[0])):
            reached.setdefault(key, set()).add(cid)
    assert set(reached) == set(FORMS_EXPECTED), reached
    for key, cid in FORMS_EXPECTED.items():
        assert cid in reached[key], (key, cid, reached[key])


@pytest.mark.gpu
def test_cases_reach_every_memory_form_on_the_device(tmp_path_factory, monkeypatch, capfd):
    """Dimension f: the four predicates of the pass on the classes the library logs and the candidates the oracle evaluated; the
    cases reach every combination that can occur (FORMS_EXPECTED), each in the case named there, and every fill matches the oracle."""
    reached = {}
    for cid in sorted(set(FORMS_EXPECTED.values())):
        o = oracle_of(cid, tmp_path_factory)
        forms = _check_on_device(cid, tmp_path_factory, capfd, monkeypatch, seq=False)      # (asserts that the logged classes are the restated ones)
        for key in _reached(o, forms):
            reached.setdefault(key, set()).add(cid)
    print(reached)
    assert set(reached) == set(FORMS_EXPECTED)
    for key, cid in FORMS_EXPECTED.items():
        assert cid in reached[key], (key, cid, reached[key])
