"""Partial mode's fallback forms and its overlap detector (cases: tools/partial_cases.py; fixtures: tests/golden/p*.tar.gz, made
with the reference's own binaries).

In a partial-mode run placeReads has the fast form of fig_engine_partial.h and the generic loops of fig_engine_core.h (512
threads, one read per wave, fig_accumulate_chunk); fig_partial_fast refuses the fast form for a gap whose clipped reads hold an
N, for a gap fewer than L - 1 bases from its contig's start and for a class whose table is tiled.  After the MLE pass
fig_detect_overlap_par deals the read pairs over the threads, and falls back to lane 0's serial walk above 192 reads and in a
tiled class.  The emulation is one lane wide: the dealing, the atomics and the wave reductions of these forms run only on the
device, so the GPU tests here are the only comparison of them with anything.

CPU: the form each gap takes, from the restated predicates and class table; the branches of the detector the fixtures reach,
from the oracle's DET trace lines (300, 30 * len with two or more maximal pairs, -100 from a false overlap, 0 / 0); the guard
against likelihood ties; the emulation against the oracle on the three plane cases, bit for bit.
GPU: every case through the C ABI against the oracle (strings, filled_len, gaptofill, candidate records exact; likelihood
1e-6 relative; placeReads calls and algorithmic flops equal; countsGap and per-read maxima 1e-6 on pn, pstart_10, pwide), the
library's own class lines against the restated table, and pn + pmany + pwide as one batch under four scheduler settings,
bit-identical to the default fill.

The detector's result enters every candidate's likelihood as +300, +30 * len or -100, so a wrong branch fails the 1e-6 check."""
import os
import re

import numpy as np
import pytest

import util
from tools import partial_cases as pc
from test_planes import compare_planes, fill_with_planes, model_of, parse_planes, prepare
from figbird_amd import api, synth

CASES = list(pc.all_cases())
PLANE_CASES = ["pn", "pstart_10", "pwide"]
TOL = 1e-6

_ORACLE = {}


def oracle_of(cid, tmp_path_factory):
    """The case, its inputs, the host model and the oracle's records (Figbird.cpp-main mode: one process, the gaps in order):
    computed once per case id and shared, read-only.  Trace level 5 (CAND + DET), 7 (+ planes) for the plane cases."""
    if cid not in _ORACLE:
        base = tmp_path_factory.mktemp("pf_" + cid)
        root, case = prepare(pc.merged() if cid == "pmix" else cid, base)
        tr = os.path.join(str(base), "o.trace")
        planes_on = cid in PLANE_CASES
        r = util.run_oracle_figbird(root, trace=tr, level=7 if planes_on else 5)
        assert r.returncode == 0, r.stderr
        cands, _ = util.parse_trace(tr)
        stats = [ln.rstrip("\n").split("\t")[1:3] for ln in open(tr) if ln.startswith("STATS")]
        gapout = [ln.split("\t") for ln in util.read(os.path.join(root, "tmp", "gapout0.txt")).splitlines()]
        gtf = [int(x) for x in util.read(os.path.join(root, "tmp", "gaptofill0.txt")).split()]
        assert len(gapout) == len(case.gaps) == len(gtf) and len(stats) == 1
        _ORACLE[cid] = dict(case=case, root=root, model=model_of(root), cands=cands, planes=parse_planes(tr) if planes_on else None, det=pc.parse_det(tr),
                            liks=pc.parse_cands(tr), gapout=gapout, gaptofill=gtf, place_calls=int(stats[0][0]), flops=float(stats[0][1]))
    return _ORACLE[cid]


def fill(lib_path, o, planes=True):
    """-> (FillResult with candidate records [and both planes], fig_get_stats) of one fill in a fresh context."""
    if planes and o["planes"] is not None:
        return fill_with_planes(lib_path, o["case"], o["model"], o["planes"])
    eng = api.Engine(0, lib_path=lib_path)
    eng.set_model(o["model"])
    res = eng.fill(synth.case_to_batch(o["case"]), debug_cand=512)
    st = eng.stats()
    eng.close()
    return res, st


def compare_with_oracle(o, res, st, tol):
    """-> the largest relative likelihood error seen."""
    assert [int(e[4]) for e in o["gapout"]] == list(res.filled_len)
    assert [e[5] if len(e) > 5 else "" for e in o["gapout"]] == res.strings
    assert o["gaptofill"] == list(res.gaptofill)
    worst = 0.0
    assert len(o["cands"]) > 0
    for g, cands in o["cands"].items():
        got = res.cand[g]
        assert len(got) == len(cands), f"gap {g}: candidate count"
        for (G1, it1, lik1, v1), (G2, it2, v2, lik2) in zip(cands, got):
            assert (G1, it1, v1) == (G2, it2, v2), f"gap {g} G={G1}"
            if np.isfinite(lik1):
                err = abs(lik1 - lik2) / max(1.0, abs(lik1))
                worst = max(worst, err)
                assert err <= tol, f"gap {g} G={G1}: {lik1!r} vs {lik2!r}"
            else:
                assert lik1 == lik2 or (np.isnan(lik1) and np.isnan(lik2))
    if o["planes"] is not None and res.counts is not None:
        compare_planes(res, o["planes"], tol)
    assert st["place_calls"] == o["place_calls"]
    assert st["alg_flops"] == o["flops"]
    print(f"{o['case'].name}: largest likelihood error {worst:.3g} relative over {sum(len(c) for c in o['cands'].values())} candidates")
    return worst


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("cid", CASES)
def test_each_gap_takes_the_form_the_case_is_for(cid):
    """fig_partial_fast and the detector's fallback condition, restated (tools/partial_cases.py), on the fixture's own case."""
    case = pc.all_cases()[cid]()
    f = pc.forms(case)
    assert [(x[1], x[2]) for x in f] == pc.EXPECTED_FORMS[cid]
    if cid == "pn":                  # the clean gap shares its class with a gap that holds an N
        assert f[0][0] is f[1][0] and f[0][1] != f[1][1]
        assert [any("N" in r.seq for r in g.partial) for g in case.gaps] == [True, False, True]
    if cid == "p192":
        assert [len(g.partial) for g in case.gaps] == [192, 193]
    if cid == "pmany":               # 240 reads = 15 super-chunks of the fast E-step
        assert all(len(g.partial) == 15 * pc.FIG_PT_ROWS for g in case.gaps)
    if cid.startswith("pwide"):      # the 1217-1600 class with its table in LDS, and the last class, tiled
        assert (f[0][0]["capGl"], f[0][0]["lds_tab"], f[0][0]["tiles"]) == (1256, 1, 0)
        assert f[1][0] is f[2][0] and f[1][0]["lds_tab"] == 0 and f[1][0]["tiles"] >= 2
        assert [g.length for g in case.gaps] == [1250, 1700, 1800]
    if cid == "pwide_n":
        assert all(any("N" in r.seq for r in g.partial) for g in case.gaps)
    assert all(len(g.partial) < 3000 for g in case.gaps)


def test_predicates_restated_switch_where_the_device_code_says():
    cls = pc.class_table([150], 50)[0][0]
    assert (cls["capGl"], cls["ncolE"], cls["nt"], cls["nteams"], cls["lds_tab"], cls["tiles"]) == (152, 256, 256, 4, 1, 0)
    f = lambda start, n=False, c=cls, L=50: pc.partial_fast(c, L, start, 180, n)
    assert f(49) and not f(48) and not f(10) and not f(49, n=True) and f(5000)
    assert pc.detector_parallel(cls, 50, 192) and not pc.detector_parallel(cls, 50, 193)
    assert pc.detector_parallel(cls, 200, 88) and not pc.detector_parallel(cls, 200, 89)         # 89 * 208 > 256 * 72: the staging area
    # the tiled class: neither form, whatever the gap
    t, _ = pc.class_table([1800], 101)
    assert t[0]["lds_tab"] == 0 and t[0]["tiles"] >= 2 and not f(5000, c=t[0], L=101) and not pc.detector_parallel(t[0], 101, 10)
    # a 1700-bp gap alone at L = 101 is not tiled (why pwide carries an 1800-bp gap beside it); 1736 | 1737 columns is the edge
    assert pc.class_table([1700], 101)[0][0]["lds_tab"] == 1
    assert pc.class_table([1736], 101)[0][0]["lds_tab"] == 1 and pc.class_table([1737], 101)[0][0]["lds_tab"] == 0
    assert [pc.gmax_partial(g, 50) for g in (12, 20, 40, 50, 51, 100, 101)] == [150, 150, 150, 150, 255, 500, 101]


def test_partial_n_rate_leaves_the_other_streams_alone():
    """synth.make_case(partial_n_rate=...) writes N into clipped reads only, and at 0 draws nothing: every earlier seed still
    gives the case its fixture was made from."""
    kw = dict(contig_len=5000, read_len=50, insert_mean=180, insert_sd=10, coverage=30, err=0.005, n_model_pairs=50)
    a = synth.make_case("a", 5, "partial", [(1500, 30), (3000, 40)], **kw)
    b = synth.make_case("a", 5, "partial", [(1500, 30), (3000, 40)], partial_n_rate=0.0, **kw)
    c = synth.make_case("a", 5, "partial", [(1500, 30), (3000, 40)], partial_n_rate=0.05, partial_n_gaps=[1], **kw)
    assert a == b
    assert c.gaps[0].partial[0].seq.count("N") == 0 and sum(r.seq.count("N") for r in c.gaps[0].partial) == 0
    n1 = sum(r.seq.count("N") for r in c.gaps[1].partial)
    assert 0 < n1 < 0.2 * 50 * len(c.gaps[1].partial)
    assert c.myout == a.myout and c.scaffolds == a.scaffolds


def test_fixtures_reach_every_branch_of_the_detector(tmp_path_factory):
    """Over the fixtures, the oracle's detect_overlap_gapestimate returns, at least once each: 300; a 30 * len value with two or
    more pairs of maximal length (the parallel form's tie-break); 0 / -1 from a false overlap; 0 / 0.  Both detector forms see
    them: the serial one in pmany, the parallel one in the pstart cases."""
    seen, by_case = set(), {}
    for cid in CASES:
        by_case[cid] = pc.det_branches(oracle_of(cid, tmp_path_factory)["det"])
        seen |= by_case[cid]
    print({k: sorted(v) for k, v in by_case.items()})
    assert pc.REQUIRED_BRANCHES <= seen, sorted(pc.REQUIRED_BRANCHES - seen)
    assert pc.REQUIRED_BRANCHES <= by_case["pmany"]                                                             # serial form
    assert pc.REQUIRED_BRANCHES <= by_case["pstart_10"] | by_case["pstart_48"] | by_case["pstart_49"]          # parallel form
    for cid in CASES:                # one DET record per partial-mode placeReads call
        o = oracle_of(cid, tmp_path_factory)
        assert len(o["det"]) == o["place_calls"] > 0


@pytest.mark.parametrize("cid", CASES + ["pmix"])
def test_no_decision_sits_within_the_tolerance_of_flipping(cid, tmp_path_factory):
    """Device and glibc differ in the last ulp, so a fixture is only usable at 1e-6 if no best-candidate or diff1 <= 0.9 decision
    of the candidate loop is closer than that to flipping (tools/partial_cases.tie_margin; values equal bit for bit are fine)."""
    m = pc.tie_margin(oracle_of(cid, tmp_path_factory)["liks"])
    print(cid, "tie margin", m)
    assert m > pc.TIE_TOL


@pytest.mark.parametrize("cid", PLANE_CASES)
def test_emulation_equals_oracle_exactly(cid, tmp_path_factory):
    """Through the C ABI of the one-lane emulation (glibc): strings, counters, candidate records and both planes bit-identical to
    the oracle.  This pins the inputs and the records the GPU tests compare with."""
    o = oracle_of(cid, tmp_path_factory)
    res, st = fill(util.EMULIB, o)
    assert compare_with_oracle(o, res, st, 0.0) == 0.0


# ---------------------------------------------------------------------------------------------------------------- GPU
_CLASS_RE = re.compile(r"\[figsched\] class: capG=(\d+) capGl=(\d+) ncolE=(\d+) Wcap=(\d+) nt=(\d+) nteams=(\d+) lds_tab=(\d+) tiles=(\d+)")
_KNOBS = ("FIG_SCHED", "FIG_LANES", "FIG_MIN_CHUNK", "FIG_ITEMS_PER_WG", "FIG_ESTEP", "FIG_CLASS_LANES")


def _native():
    return "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASES)
def test_device_matches_oracle(cid, tmp_path_factory, monkeypatch, capfd):
    """Every directed case on the device, against the oracle; and the launch classes the library built are the ones the form
    assertions above were computed from."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FIG_SCHED_LOG", "1")
    o = oracle_of(cid, tmp_path_factory)
    capfd.readouterr()
    res, st = fill(None, o)
    err = capfd.readouterr().err
    assert _native()
    compare_with_oracle(o, res, st, TOL)
    logged = sorted(set((int(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[5]), int(m[6]), int(m[7])) for m in _CLASS_RE.findall(err)))
    want = sorted(set((c["capGl"], c["ncolE"], c["Wcap"], c["nt"], c["nteams"], c["lds_tab"], c["tiles"]) for c, _, _ in pc.forms(o["case"])))
    assert logged == want, err[-2000:]


_SETTINGS = {"seq": {"FIG_SCHED": "seq"}, "lanes_serial": {"FIG_LANES": "serial"}, "chunk1_ipw1": {"FIG_MIN_CHUNK": "1", "FIG_ITEMS_PER_WG": "1"},
             "chunk64": {"FIG_MIN_CHUNK": "64"}}


def assert_fills_bit_identical(a, b, n_gaps):
    assert a.strings == b.strings
    assert list(a.filled_len) == list(b.filled_len) and list(a.gaptofill) == list(b.gaptofill)
    assert list(a.n_place) == list(b.n_place)
    for g in range(n_gaps):
        assert len(a.cand[g]) == len(b.cand[g]), f"gap {g}"
        for x, y in zip(a.cand[g], b.cand[g]):
            assert tuple(x[:3]) == tuple(y[:3]), f"gap {g}"
            assert np.float64(x[3]).tobytes() == np.float64(y[3]).tobytes(), f"gap {g}: {x} vs {y}"


@pytest.mark.gpu
def test_same_gaps_other_neighbours_other_rounds(tmp_path_factory, monkeypatch):
    """pn + pmany + pwide as ONE batch (tools/partial_cases.merged: four launch classes, both placeReads forms and both detector
    forms side by side), filled by default and under FIG_SCHED=seq, FIG_LANES=serial, FIG_MIN_CHUNK=1 FIG_ITEMS_PER_WG=1 and
    FIG_MIN_CHUNK=64: the same device arithmetic in other rounds and beside other neighbours.  Strings, gaptofill, candidate
    records, likelihood bits, per-gap placeReads counts and algorithmic flops bit-identical to the default fill; placeReads
    calls and flops equal to the oracle's in every fill; the default fill within 1e-6 of the oracle."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    o = oracle_of("pmix", tmp_path_factory)
    n = len(o["case"].gaps)
    base, sb = fill(None, o)
    assert _native()
    compare_with_oracle(o, base, sb, TOL)
    for name, env in _SETTINGS.items():
        for k in _KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r, st = fill(None, o)
        assert_fills_bit_identical(base, r, n)
        assert st["place_calls"] == sb["place_calls"] == o["place_calls"], name
        assert st["alg_flops"] == sb["alg_flops"] == o["flops"], name
