"""Reuse of the last MLE search while the E-step consensus stands (fig_mle_reuse_*, figbird_amd/csrc/fig_engine_core.h).

Mode 0 of the MLE pass is a function of the soft consensus E.gs, the flanks, the model and the reads; within one candidate
evaluation only E.gs moves.  fig_place_reads keeps the string of its last executed pass and the pass's per-read outputs in the
scratch slab and, when the next call's string is the same, restores them instead of searching again.  FIG_MLE_REUSE=0 runs
every pass.  Nothing but mle_exec_flops (the FP64 multiplies the passes executed) may tell the two apart.

Cases: tools/mle_cases.py.  Per case one oracle run, shared with tests/test_mle_forms.py (same process, same cache), and fills
through the C ABI with candidate records, both numeric planes and the draw planes on.  On = off bit for bit: strings,
filled_len, gaptofill, every candidate record (estimate, iterations, valid count, likelihood bits), the planes, the draw
planes, placeReads calls, alg_flops and mle_alg_flops; both equal the oracle as tests/test_mle_forms.py compares with it.
Evidence that the path ran: mle_exec_flops strictly smaller with reuse on.

Why reuse fires in every case chosen: a candidate's EM loop ends through comp_count >= 5, five consecutive calls with an
unchanged hard consensus, and the candidates here reach that with the soft consensus unchanged as well (asserted through the
counter, not assumed).  What each case adds is asserted on the oracle's own records in
test_cases_cover_the_invalidations_they_are_named_for.

MEASURED, mle_exec_flops with reuse / without:
  emulation  d_12 8503828 / 30857540  d_30 9694792 / 31600408  b_L31 3623854 / 12831041  b_L65 7861059 / 27682962
             b_short 4023303 / 13697118  c_slot31 8014172 / 20208198  f_lds 208368 / 237744
  MI355X     d_12 17165920 / 59723856 (seq 17170276 / 59728212)  b_L31 1984620 / 8704831 (seq 1984806 / 8704800)
             c_slot31 4096448 / 10291828 (seq 4096232 / 10291504)  f_lds 220108 / 249484 (seq the same)
"""
import dataclasses

import numpy as np
import pytest

import util
from tools import mle_cases as mc
from test_mle_forms import INT_MIN, _native, compare, compare_draw, fill_with_draw, oracle_of
from test_planes import _close

# case -> what it is here for
REUSE_CASES = {
    "d_12": "G0 <= 30: the three flags are OR-only within a candidate; reads with N beside N-free ones",
    "d_30": "G0 <= 30 at the flags' upper edge",
    "b_L31": "L = 31 (no sweep: Lfull < 32), a 60-bp gap with many candidates next to a one-candidate gap of 420 bp",
    "b_L65": "L = 65, two words and a tail per read",
    "b_short": "reads shorter than L (wave-per-read path) among full-length ones",
    "c_slot31": "a read with an N base (plain chain) and three shorter reads",
    "f_lds": "a 405-bp gap: large_gap_flag, finalize_flag = 1 inside the loop, low-coverage regions, seed re-weighting",
}
DEVICE_CASES = ["d_12", "b_L31", "c_slot31", "f_lds"]      # the 72-, 480- and 324-column classes of 256 threads and the 405-bp gap's own


def fill(lib, o, monkeypatch, reuse, seq=False):
    for k in ("FIG_ESTEP", "FIG_SH_CHUNKS", "FIG_SCHED", "FIG_MLE_REUSE"):
        monkeypatch.delenv(k, raising=False)
    if not reuse:
        monkeypatch.setenv("FIG_MLE_REUSE", "0")
    if seq:
        monkeypatch.setenv("FIG_SCHED", "seq")
    return fill_with_draw(lib, o)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def assert_same_fill(a, b, lik_tol=0.0):
    """Two fills of one case: everything integer exact; likelihood and planes bit for bit (lik_tol 0) or at lik_tol."""
    assert a.strings == b.strings and list(a.filled_len) == list(b.filled_len) and list(a.gaptofill) == list(b.gaptofill)
    assert len(a.cand) == len(b.cand)
    for ga, gb in zip(a.cand, b.cand):
        assert [c[:3] for c in ga] == [c[:3] for c in gb]
        for ca, cb in zip(ga, gb):
            if lik_tol == 0.0:
                assert bits(ca[3]) == bits(cb[3]), (ca, cb)
            else:
                assert ca[3] == cb[3] or abs(ca[3] - cb[3]) <= lik_tol * max(1.0, abs(ca[3])), (ca, cb)
    for x, y in zip(a.draw, b.draw):
        assert np.array_equal(x, y)
    for pa, pb in ((a.counts, b.counts), (a.read_maxlv, b.read_maxlv)):
        if lik_tol == 0.0:
            assert np.array_equal(bits(pa), bits(pb))
        else:
            ok, at = _close(pa.reshape(-1), pb.reshape(-1), lik_tol)
            assert ok, (at, pa.reshape(-1)[at], pb.reshape(-1)[at])


def assert_same_counters(sa, sb):
    for k in ("place_calls", "alg_flops", "mle_alg_flops"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cases_cover_the_invalidations_they_are_named_for(tmp_path_factory):
    """On the oracle's own candidate records: candidates of more than 5 EM iterations (the consensus changed inside the loop, so
    the key must miss there) beside candidates at the minimum; gaps with several candidates (the key must not survive
    fig_initialize); a candidate at G == G0 (org is restored, fig_run_original may follow); gaps of at most 30 bp; reads with N
    and shorter reads; a gap over 400 bp (large_gap_flag: finalize_flag = 1 inside the loop)."""
    for cid in REUSE_CASES:
        o = oracle_of(cid, tmp_path_factory)
        assert o["cands"], cid
        g0 = o["case"].gaps[0].length
        iters = [c[1] for c in o["cands"][0]]
        print(cid, "G0", g0, "candidates", len(iters), "iterations", sorted(set(iters)))
        if cid != "f_lds":
            assert len(iters) > 1 and any(c[0] == g0 for c in o["cands"][0]), cid
            assert min(iters) == 5 or max(iters) > 5, cid
    assert any(max(c[1] for c in oracle_of(cid, tmp_path_factory)["cands"][0]) > 5 for cid in REUSE_CASES)
    assert oracle_of("d_12", tmp_path_factory)["case"].gaps[0].length <= 30 and oracle_of("d_30", tmp_path_factory)["case"].gaps[0].length <= 30
    routes = [mc.route(r, 36) for r in oracle_of("c_slot31", tmp_path_factory)["case"].gaps[0].unmapped]
    assert "chain" in routes and "wave" in routes and "lane" in routes
    assert "wave" in [mc.route(r, 36) for r in oracle_of("b_short", tmp_path_factory)["case"].gaps[0].unmapped]
    assert "chain" in [mc.route(r, 36) for r in oracle_of("d_12", tmp_path_factory)["case"].gaps[0].unmapped]
    f = oracle_of("f_lds", tmp_path_factory)
    assert f["case"].gaps[0].length > 400 and len(f["cands"][0]) == 1
    assert {g.length for g in oracle_of("b_L31", tmp_path_factory)["case"].gaps} == {60, mc.B_MATE}


@pytest.mark.parametrize("cid", list(REUSE_CASES))
def test_reuse_on_equals_off_equals_oracle(cid, tmp_path_factory, monkeypatch):
    """The one-lane emulation with reuse on and with FIG_MLE_REUSE=0: bit for bit the same fill and the same algorithmic
    counters, both equal to the oracle (tolerance 0), and fewer multiplies executed with reuse on."""
    o = oracle_of(cid, tmp_path_factory)
    on, son = fill(util.EMULIB, o, monkeypatch, True)
    off, soff = fill(util.EMULIB, o, monkeypatch, False)
    print(f"{cid}: mle_exec_flops {son['mle_exec_flops']:.0f} with reuse, {soff['mle_exec_flops']:.0f} without, mle_alg_flops {son['mle_alg_flops']:.0f}")
    assert_same_fill(on, off)
    assert_same_counters(son, soff)
    for res, st in ((on, son), (off, soff)):
        compare(o, res, st, 0.0)
        compare_draw(o, res)
    assert son["mle_exec_flops"] < soff["mle_exec_flops"], f"{cid}: no pass was reused"


def test_reuse_is_the_same_in_every_schedule_of_the_emulation(tmp_path_factory, monkeypatch):
    """FIG_SCHED=seq (whole gaps, fig_run_original and finalize straight after the loop in one workgroup) against the default
    schedule, reuse on: the same fill, and reuse fires there as well.  (The multiplies executed differ a little between the two
    schedules with or without reuse: tests/test_mle_forms.py, the last lines of its MEASURED block.)"""
    o = oracle_of("d_12", tmp_path_factory)
    a, sa = fill(util.EMULIB, o, monkeypatch, True)
    b, sb = fill(util.EMULIB, o, monkeypatch, True, seq=True)
    c, sc = fill(util.EMULIB, o, monkeypatch, False, seq=True)
    assert_same_fill(a, b)
    assert_same_fill(b, c)
    assert_same_counters(sa, sb)
    assert_same_counters(sb, sc)
    assert sb["mle_exec_flops"] < sc["mle_exec_flops"]


def marker_model(o):
    """The injected non-monotone model of tests/test_mle_forms.py: one errorTypeProbs entry of 1.25 in the model of a_p20."""
    T = np.array(o["model"].T, dtype=np.float64)
    T[0 * 5 + 1] = 1.25
    m = dataclasses.replace(o["model"], T=T)
    assert mc.model_fmm(o["model"]) < 0.05 and mc.model_fmm(m) == 2.0
    return dict(o, model=m, fmm=2.0)


def test_marker_model_runs_every_pass_in_full(tmp_path_factory, monkeypatch):
    """Under the non-monotone marker nothing is pruned and nothing is reused: on and off execute the same multiplies, at least
    the credited ones, and give the same fill."""
    o2 = marker_model(oracle_of("a_p20", tmp_path_factory))
    on, son = fill(util.EMULIB, o2, monkeypatch, True)
    off, soff = fill(util.EMULIB, o2, monkeypatch, False)
    assert len(on.cand[0]) > 1 and max(c[2] for c in on.cand[0]) >= 3, "no read accepted under the injected model"
    assert_same_fill(on, off)
    assert_same_counters(son, soff)
    assert son["mle_exec_flops"] == soff["mle_exec_flops"] >= son["mle_alg_flops"]


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("seq", [False, True], ids=["default", "seq"])
@pytest.mark.parametrize("cid", DEVICE_CASES)
def test_device_with_reuse_equals_the_emulation(cid, seq, tmp_path_factory, monkeypatch):
    """The device with reuse on against the emulation with reuse on and against the device with FIG_MLE_REUSE=0, in both
    scheduler forms: everything integer exact, likelihood and planes at the project's 1e-6 against the emulation and bit for
    bit between the two device fills; the oracle compare of tests/test_mle_forms.py on top; fewer multiplies with reuse on."""
    o = oracle_of(cid, tmp_path_factory)
    emu, semu = fill(util.EMULIB, o, monkeypatch, True, seq)
    dev, sdev = fill(None, o, monkeypatch, True, seq)
    doff, sdoff = fill(None, o, monkeypatch, False, seq)
    assert _native()
    print(f"{cid} seq={seq}: device mle_exec_flops {sdev['mle_exec_flops']:.0f} with reuse, {sdoff['mle_exec_flops']:.0f} without")
    assert_same_fill(emu, dev, 1e-6)
    assert_same_fill(dev, doff)
    compare(o, dev, sdev, 1e-6)
    compare_draw(o, dev)
    assert sdev["place_calls"] == semu["place_calls"] == sdoff["place_calls"] and sdev["alg_flops"] == semu["alg_flops"] == sdoff["alg_flops"]
    if seq:                             # (the default schedule's speculative evaluations are counted in mle_alg_flops as well)
        assert sdev["mle_alg_flops"] == semu["mle_alg_flops"] == sdoff["mle_alg_flops"]
    assert sdev["mle_exec_flops"] < sdoff["mle_exec_flops"], f"{cid}: no pass was reused on the device"


@pytest.mark.gpu
def test_marker_model_on_the_device_reuses_nothing(tmp_path_factory, monkeypatch):
    o2 = marker_model(oracle_of("a_p20", tmp_path_factory))
    on, son = fill(None, o2, monkeypatch, True, seq=True)
    off, soff = fill(None, o2, monkeypatch, False, seq=True)
    assert _native()
    assert_same_fill(on, off)
    assert_same_counters(son, soff)
    assert int((on.draw[0] != INT_MIN).sum()) >= 3
    assert son["mle_exec_flops"] == soff["mle_exec_flops"] >= son["mle_alg_flops"]
