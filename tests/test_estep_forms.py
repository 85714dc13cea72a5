"""The shared-factor form of the unmapped E-step (fig_hot_estep_sh, figbird_amd/csrc/fig_engine_shared.h) at its own edges.

The emulation always runs the pair form, so only the GPU tests here execute the chunking, the split rounds, the operand-select
stream and fig_weights_n; the CPU tests pin the inputs (emulation == oracle, bit for bit) and the integer arithmetic that says
which fig_sh_unit<NS> instantiation each case reaches.  Cases: tools/estep_cases.py.

Per case one oracle run (Figbird.cpp-main mode, level-3 trace) and one fill through the C ABI with the candidate records and
both planes on: strings, filled_len and gaptofill exact; candidate records (G, EM iterations, valid_count) exact; likelihood,
countsGap and the per-read maxima at the parity contract's 1e-6 (0 with the emulation), 0 and +-inf exact; placeReads calls
and algorithmic flops equal to the oracle's STATS line (the shared form's phase B counts its flops itself).

Evidence that the form under test ran (the A/B rule): a second fill with FIG_ESTEP=pair.  A candidate that fig_sh_applies
puts in the pair form in both fills must be bit-identical in likelihood, countsGap and per-read maxima; one it puts in the
shared form must differ from the pair fill in at least one bit of countsGap (the two forms take their weights from
different log/exp routines: fig_weights_n against the library's log10 / exp).

What the truncation leaves of the strings: with few reads the oracle keeps an N core in every gap over 400 bp here, and the
string is all N for a405_1 .. a405_5, a500_1 .. a500_4 and b_all (every read irregular).  That is fine for the planes, which
are compared whatever the string holds; that reads were placed at all is checked on the candidate records and the planes
themselves (test_generator_leaves_every_gap_a_placed_read).  Only the 12-bp and the partial-mode gaps fill completely.  The
planes are compared whatever the string holds."""
import os
import re

import numpy as np
import pytest

import util
from figbird_amd import api
from tools import estep_cases as ec
from test_planes import compare_planes, fill_with_planes, model_of, parse_planes, prepare

CASES = ec.all_cases()
CPU_IDS = [c for c in CASES if not c.startswith("f_")]           # dimensions a-e (f needs the device's class geometry to mean anything)
AB_IDS = ["a405_65", "d256", "d512", "e_Lm2", "e_Lm1", "f_alone", "f_mate"]

_ORACLE = {}


def oracle_of(cid, tmp_path_factory):
    """The case, its written inputs, the host model and the oracle's records: computed once per case id and shared (read-only)."""
    if cid not in _ORACLE:
        base = tmp_path_factory.mktemp("estep_" + cid)
        root, case = prepare(CASES[cid](), base)
        tr = os.path.join(str(base), "o.trace")
        r = util.run_oracle_figbird(root, trace=tr, level=3)
        assert r.returncode == 0, r.stderr
        cands, _ = util.parse_trace(tr)
        stats = [ln.rstrip("\n").split("\t")[1:3] for ln in open(tr) if ln.startswith("STATS")]
        gapout = [ln.split("\t") for ln in util.read(os.path.join(root, "tmp", "gapout0.txt")).splitlines()]
        gtf = [int(x) for x in util.read(os.path.join(root, "tmp", "gaptofill0.txt")).split()]
        assert len(gapout) == len(case.gaps) == len(gtf) and len(stats) == 1
        _ORACLE[cid] = dict(case=case, root=root, model=model_of(root), cands=cands, planes=parse_planes(tr), gapout=gapout, gaptofill=gtf,
                            place_calls=int(stats[0][0]), flops=float(stats[0][1]))
    return _ORACLE[cid]


def compare_with_oracle(o, res, st, tol):
    assert [int(e[4]) for e in o["gapout"]] == list(res.filled_len)
    assert [e[5] if len(e) > 5 else "" for e in o["gapout"]] == res.strings
    assert o["gaptofill"] == list(res.gaptofill)
    assert set(o["cands"]) == set(o["planes"])
    for g, cands in o["cands"].items():
        got = res.cand[g]
        assert len(got) == len(cands), f"gap {g}: candidate count"
        for (G1, it1, lik1, v1), (G2, it2, v2, lik2) in zip(cands, got):
            assert (G1, it1, v1) == (G2, it2, v2), f"gap {g} G={G1}"
            print(f"gap {g} G={G1}: likelihood {lik1!r} (oracle) {lik2!r}")
            if np.isfinite(lik1):
                assert abs(lik1 - lik2) <= tol * max(1.0, abs(lik1)), f"gap {g} G={G1}: {lik1!r} vs {lik2!r}"
            else:
                assert lik1 == lik2 or (np.isnan(lik1) and np.isnan(lik2))
    compare_planes(res, o["planes"], tol)
    assert st["place_calls"] == o["place_calls"]
    assert st["alg_flops"] == o["flops"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_read_counts_reach_every_split_instantiation():
    """Dimension a's parameters, through the integer arithmetic of fig_hot_estep_sh:309-331 (tools/estep_cases.split_plan): the
    left-over items of the last full round run fig_sh_unit<32>, <16>, <8> and <4>, and the path without left-over items is
    taken too; <4> needs the 8-wave class.  The FIG_SH_CHUNKS repeats move the same read counts to other instantiations."""
    reached = {}
    for g0, nt in ec.A_GAPS.items():
        assert ec.nt_of_class(g0) == nt
        for n in ec.READ_COUNTS:
            plan = ec.split_plan(n, g0, 36, nt)
            assert sum(p[1] for p in plan) == (n + 31) // 32 and all(p[0] == (g0 + 35 + 63) // 64 for p in plan)
            for nT, nc, nfull, mleft, fsplit in plan:
                assert nfull * (nt // 64) + mleft == nT * nc and (mleft == 0) == (fsplit == 0) and mleft * fsplit <= nt // 64
                reached.setdefault((nt, 32 // fsplit if fsplit else 0), []).append((g0, n))
    units = {u for _, u in reached}
    assert units == {0, 4, 8, 16, 32}, reached.keys()
    assert {u for nt, u in reached if nt == 256} == {0, 8, 16, 32}       # 7 tiles x 1, 2, 3 chunks leave 3, 2, 1 items of 4 waves
    assert (512, 4) in reached and (256, 4) not in reached
    alt = {(n, ch): {32 // p[4] if p[4] else 0 for g0, nt in ec.A_GAPS.items() for p in ec.split_plan(n, g0, 36, nt, ch)} for n, ch in ec.CHUNK_REPEATS}
    assert alt[(129, 1)] == {32, 4} and alt[(129, 2)] == {16, 8, 32, 4} and alt[(129, 3)] == {8, 16}
    assert alt[(33, 1)] == {32, 4}


def test_predicate_restated_switches_where_the_issue_says():
    """tools/estep_cases.sh_applies against the boundaries named in fig_engine_shared.h's header and fig_pack.h's classes."""
    f = lambda G, L, nt, nteams=4, start=1500: ec.sh_applies(G, L, nt, nteams, start, 690)
    assert f(363, 150, 256) and not f(364, 150, 256)
    assert f(412, 101, 256) and not f(413, 101, 256) and f(924, 101, 512) and not f(925, 101, 512)
    assert f(420, 36, 256, start=35) and not f(420, 36, 256, start=34)
    assert f(600, 200, 512, nteams=8) and not f(600, 200, 512, nteams=2)
    assert not f(70, 31, 256)


@pytest.mark.parametrize("cid", list(CASES))
def test_generator_leaves_every_gap_a_placed_read(cid, tmp_path_factory):
    """A compare of empty output with empty output must not pass for a live one: in every case the oracle gives every gap a
    non-empty string, and the E-step of at least one candidate placed reads: a countsGap plane with weight in it and a finite,
    non-zero per-read maximum.  No case here has the empty result as its purpose, so there is no exception.  (valid_count, the
    MLE pass's count, is 0 in a500_1, a500_3 and b_all: the planes this file is about are live there all the same.)"""
    o = oracle_of(cid, tmp_path_factory)
    for e in o["gapout"]:
        assert int(e[4]) > 0 and len(e) > 5 and len(e[5]) == int(e[4]), e[:5]
    assert len(o["cands"]) == len(o["case"].gaps)
    for g, cands in o["cands"].items():
        assert len(cands) >= 1
        assert any(cnt is not None and np.isfinite(cnt).all() and (cnt > 0).any() and rmax is not None and (np.isfinite(rmax) & (rmax != 0)).any()
                   for _, cnt, rmax in o["planes"][g]), f"gap {g}: the E-step placed no read"


@pytest.mark.parametrize("cid", CPU_IDS)
def test_emulation_equals_oracle_exactly(cid, tmp_path_factory):
    """Dimensions a-e through the one-lane emulation (pair form, glibc): bytes, counters and planes bit-identical to the oracle.
    This pins the inputs themselves."""
    o = oracle_of(cid, tmp_path_factory)
    res, st = fill_with_planes(util.EMULIB, o["case"], o["model"], o["planes"])
    compare_with_oracle(o, res, st, 0.0)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _native():
    return "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_device_matches_oracle(cid, tmp_path_factory, monkeypatch):
    """Every directed case on the device in its default form."""
    for k in ("FIG_ESTEP", "FIG_SH_CHUNKS", "FIG_SCHED"):
        monkeypatch.delenv(k, raising=False)
    o = oracle_of(cid, tmp_path_factory)
    res, st = fill_with_planes(None, o["case"], o["model"], o["planes"])
    assert _native()
    compare_with_oracle(o, res, st, 1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunks", ec.CHUNK_REPEATS)
@pytest.mark.parametrize("g0", list(ec.A_GAPS))
def test_device_matches_oracle_with_fewer_chunks_per_super_chunk(g0, n, chunks, tmp_path_factory, monkeypatch):
    """FIG_SH_CHUNKS = 1, 2, 3 (read once in fig_ctx_create): the same reads dealt as other (chunk, tile) items."""
    monkeypatch.delenv("FIG_ESTEP", raising=False)
    monkeypatch.setenv("FIG_SH_CHUNKS", str(chunks))
    o = oracle_of(f"a{g0}_{n}", tmp_path_factory)
    res, st = fill_with_planes(None, o["case"], o["model"], o["planes"])
    compare_with_oracle(o, res, st, 1e-6)


_CLASS_RE = re.compile(r"\[figsched\] class: capG=(\d+) capGl=(\d+) ncolE=(\d+) Wcap=(\d+) nt=(\d+) nteams=(\d+) lds_tab=(\d+) tiles=(\d+)")


def _fill_logged(o, capfd, monkeypatch, pair):
    """-> (FillResult, stats, [(capGl, nt, nteams, lds_tab, tiles)] from the library's `[figsched] class:` lines)."""
    monkeypatch.setenv("FIG_SCHED_LOG", "1")
    if pair:
        monkeypatch.setenv("FIG_ESTEP", "pair")
    else:
        monkeypatch.delenv("FIG_ESTEP", raising=False)
    monkeypatch.delenv("FIG_SH_CHUNKS", raising=False)
    capfd.readouterr()
    res, st = fill_with_planes(None, o["case"], o["model"], o["planes"])
    err = capfd.readouterr().err
    classes = [(int(m[1]), int(m[4]), int(m[5]), int(m[6]), int(m[7])) for m in _CLASS_RE.findall(err)]
    assert classes, err[-2000:]
    return res, st, classes


def _class_of(classes, gmax):
    """The launch class of a gap whose longest candidate is gmax columns: classes partition (0, 448], (448, 1216], (1216, 1600], ...
    (fig_pack.h, defs[]); capGl is the class's own longest candidate rounded up to 8."""
    lo = max([0] + [c for c in ec.CLASS_CAPS if c < gmax])
    hi = min([c for c in ec.CLASS_CAPS if c >= gmax] + [1 << 30])
    mine = [c for c in classes if lo < c[0] <= ((hi + 7) & ~7) and c[0] >= gmax]
    assert len(mine) == 1, (classes, gmax)
    return mine[0]


def ab_rule(o, a, b, classes, gmax_of, only=None):
    """The A/B rule between the default fill `a` and the FIG_ESTEP=pair fill `b` -> {(gap, G): "shared" | "pair"}.
    Restates fig_sh_applies (fig_engine_shared.h:573-579) through tools/estep_cases.sh_applies."""
    case, forms = o["case"], {}
    for g, recs in o["planes"].items():
        _, nt, nteams, lds_tab, tiles = _class_of(classes, gmax_of(case.gaps[g]))
        assert lds_tab == 1 and tiles == 0 and nt == ec.nt_of_class(gmax_of(case.gaps[g]))
        for k, (G, cnt, rmax) in enumerate(recs):
            if only is not None and G not in only:
                continue
            shared = ec.sh_applies(G, case.read_len, nt, nteams, case.gaps[g].start, case.max_distance)
            ca, cb = a.counts[g, k, :G, :], b.counts[g, k, :G, :]
            ra, rb = a.read_maxlv[g, k], b.read_maxlv[g, k]
            same = ca.tobytes() == cb.tobytes()
            print(f"gap {g} G={G}: nt={nt} nteams={nteams} -> {'shared' if shared else 'pair'}; countsGap entries differing: {int((ca.view(np.int64) != cb.view(np.int64)).sum())} of {ca.size}")
            if shared:
                assert not same, f"gap {g} G={G}: the default fill equals the pair form bit for bit: the shared-factor form did not run"
            else:
                assert same, f"gap {g} G={G}: pair form in both fills, countsGap differs"
                assert ra.tobytes() == rb.tobytes(), f"gap {g} G={G}: pair form in both fills, per-read maxima differ"
                la, lb = a.cand[g][k][3], b.cand[g][k][3]
                assert np.float64(la).tobytes() == np.float64(lb).tobytes(), f"gap {g} G={G}: pair form in both fills, likelihood {la!r} vs {lb!r}"
            forms[(g, G)] = "shared" if shared else "pair"
    return forms


@pytest.mark.gpu
@pytest.mark.parametrize("cid", AB_IDS)
def test_default_fill_runs_the_form_the_predicate_names(cid, tmp_path_factory, monkeypatch, capfd):
    """The A/B rule on the single-candidate cases: 412 | 413 bp and 924 | 925 bp at L = 101 (shared | pair), a 65-read case of
    dimension a (shared), the contig-start guard (gap start L - 2: S.left is one below xoff and the E-step must fall back to the
    pair form; L - 1: shared), and the 600-bp gap at L = 200 alone (8 weight rows: shared) and beside a 1200-bp gap
    (tools/estep_cases.F_MATE = 1200: the class then has 2 weight rows, so both its gaps take the pair form).  Both fills
    match the oracle."""
    o = oracle_of(cid, tmp_path_factory)
    a, sa, cls_a = _fill_logged(o, capfd, monkeypatch, pair=False)
    b, sb, cls_b = _fill_logged(o, capfd, monkeypatch, pair=True)
    assert cls_a == cls_b
    compare_with_oracle(o, a, sa, 1e-6)
    compare_with_oracle(o, b, sb, 1e-6)
    forms = ab_rule(o, a, b, cls_a, lambda g: g.length)
    want = {"a405_65": {(0, 405): "shared"}, "d256": {(0, 412): "shared", (1, 413): "pair"}, "d512": {(0, 924): "shared", (1, 925): "pair"},
            "e_Lm2": {(0, 420): "pair"}, "e_Lm1": {(0, 420): "shared"}, "f_alone": {(0, 600): "shared"}, "f_mate": {(0, 600): "pair", (1, 1200): "pair"}}[cid]
    assert forms == want


@pytest.mark.gpu
def test_batch_mate_changes_the_form_but_not_the_result(tmp_path_factory, monkeypatch, capfd):
    """Dimension f: the class geometry follows the longest gap of the class, so the 600-bp gap's E-step form depends on its
    batch-mates.  Alone its class has at least 4 weight rows; beside a 1200-bp gap (F_MATE = 1200; 1200 + 200 = 1400 columns of
    weights per row) fewer than 4.  Strings and candidate records of the 600-bp gap are identical in the two fills."""
    oa, om = oracle_of("f_alone", tmp_path_factory), oracle_of("f_mate", tmp_path_factory)
    ra, _, ca = _fill_logged(oa, capfd, monkeypatch, pair=False)
    rm, _, cm = _fill_logged(om, capfd, monkeypatch, pair=False)
    na, nm = _class_of(ca, 600)[2], _class_of(cm, 600)[2]
    print("nteams alone", na, "with mate", nm)
    assert na >= 4 and nm < 4
    assert ra.strings[0] == rm.strings[0] and ra.filled_len[0] == rm.filled_len[0] and ra.gaptofill[0] == rm.gaptofill[0]
    assert [c[:3] for c in ra.cand[0]] == [c[:3] for c in rm.cand[0]]


@pytest.mark.gpu
def test_bench_x149_crosses_the_form_boundary_inside_one_sweep(tmp_path, monkeypatch, capfd):
    """bench_x149 (tools/make_bench_golden.py): G0 = 149 at L = 150, candidates 74 .. 372 in the 256-thread class; the sweep
    crosses G + L - 1 = 512 | 513.  Default fill against FIG_ESTEP=pair, per candidate: G >= 364 bit-identical (likelihood,
    countsGap, per-read maxima), every G <= 363 differs in countsGap.  Seen on an MI355X: all 290 candidates of the shared form
    differ and all 9 of the pair form are identical, although 290 candidates of the other form ran before them -- the candidates
    of a gap do not feed one another's E-steps, so the per-candidate claim stands and need not be restricted to
    single-candidate gaps.  (The comparison with the pinned oracle records is test_gpu_parity's.)"""
    import json
    from tools import make_bench_golden as mbg
    root = util.extract_golden("bench_x149", str(tmp_path))
    ref = json.load(open(os.path.join(root, "ref", "cands.json")))
    batch, _, _ = mbg.make("bench_x149")
    model = model_of(root)
    monkeypatch.setenv("FIG_SCHED_LOG", "1")
    fills = []
    for pair in (False, True):
        if pair:
            monkeypatch.setenv("FIG_ESTEP", "pair")
        else:
            monkeypatch.delenv("FIG_ESTEP", raising=False)
        capfd.readouterr()
        eng = api.Engine(0)
        eng.set_model(model)
        res = eng.fill(batch, debug_cand=512, plane_cols=373, plane_reads=int(batch.u_read_off[1]))
        eng.close()
        cls = [(int(m[1]), int(m[4]), int(m[5])) for m in _CLASS_RE.findall(capfd.readouterr().err)]
        fills.append((res, cls))
    (a, cls_a), (b, cls_b) = fills
    assert cls_a == cls_b == [(448, 256, 4)], cls_a
    assert [c[0] for c in a.cand[0]] == [c[0] for c in ref["cands"]] == [c[0] for c in b.cand[0]]
    assert a.strings == b.strings
    n_sh = n_pair = 0
    for k, (G, it, v, lik) in enumerate(a.cand[0]):
        shared = ec.sh_applies(G, 150, 256, 4, int(batch.gap_start[0]), int(model.max_distance))
        assert shared == (G <= 363)
        same = a.counts[0, k, :G].tobytes() == b.counts[0, k, :G].tobytes()
        if shared:
            assert not same, f"G={G}: the shared-factor form did not run"
            n_sh += 1
        else:
            assert same and a.read_maxlv[0, k].tobytes() == b.read_maxlv[0, k].tobytes(), f"G={G}"
            assert (it, v) == b.cand[0][k][1:3] and np.float64(lik).tobytes() == np.float64(b.cand[0][k][3]).tobytes(), f"G={G}"
            n_pair += 1
    assert (n_sh, n_pair) == (363 - 74 + 1, 372 - 364 + 1)
