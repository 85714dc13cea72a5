"""The per-read maxima of the shared-factor E-step (fig_hot_estep_sh, figbird_amd/csrc/fig_engine_shared.h): taken in phase A by a
transposing reduction per (tile, reads of the unit) and an atomic maximum per read, the offset found in phase B by comparing
with it, the flop credit of a read in closed form.  Cases: tools/estep_maxima_cases.py; machinery and contract: those of
tests/test_estep_forms.py (oracle run with level-3 trace; fill with candidate records and both planes; strings, filled_len,
gaptofill and candidate records exact; likelihood, countsGap and per-read maxima at 1e-6 with 0 and +-inf exact; placeReads
calls and algorithmic flops equal to the oracle's STATS line, which is what checks the closed-form credit; a second fill with
FIG_ESTEP=pair as evidence that the shared form ran).

The emulation runs the pair form, so the CPU tests pin the inputs (emulation == oracle bit for bit), the integer arithmetic
that says which fig_sh_unit<NS> a case reaches, and the windows (an empty one; ones that begin and end inside a tile).

Two cases are also compared with a fill of the library as it was before the maxima moved (tests/golden/estep_maxima_parent.json,
recorded once on an MI355X from the parent commit's library): the per-read maxima plane and mle_exec_flops, the count of
multiplies the MLE search executed after pruning, which moves when a read's hint_e does.  Both must be equal exactly.

Not covered: a constructed bit-for-bit tie of two placements' products (see profiles/estep_maxima/README.md)."""
import json
import os

import numpy as np
import pytest

import util
from figbird_amd import synth
from tools import estep_cases as ec
from tools import estep_maxima_cases as mc
from test_planes import fill_with_planes, model_of, parse_planes, prepare
from test_estep_forms import _fill_logged, ab_rule, compare_with_oracle

CASES = mc.all_cases()
PARENT_IDS = ["mixed", "n129"]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estep_maxima_parent.json")

_ORACLE = {}


def oracle_of(cid, tmp_path_factory):
    """The case, its written inputs, the host model and the oracle's records: computed once per case id and shared (read-only)."""
    if cid not in _ORACLE:
        base = tmp_path_factory.mktemp("emax_" + cid)
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


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cases_reach_the_shapes_they_are_named_for():
    """Through tools/estep_cases.split_plan: the read counts leave a partial last chunk and cross the super-chunk, the unit cases
    reach fig_sh_unit<16>, <8> (both workgroup sizes) and <4> (8 waves only: with 4 waves the split stops at 32 / 4 reads),
    w448 | w449 have a full last tile | a last tile with one live lane."""
    for n in mc.N_READS:
        plan = ec.split_plan(n, 405, mc.L, 256)
        assert len(plan) == (n + 127) // 128 and sum(p[1] for p in plan) == (n + 31) // 32
    assert len(ec.split_plan(129, 405, mc.L, 256)) == 2 and 127 % 32 != 0 and 33 % 32 == 1
    for cid, (g0, n, ns) in mc.UNITS.items():
        nt = ec.nt_of_class(g0)
        assert nt == int(cid[1:4])
        (nT, nc, nfull, mleft, fsplit), = ec.split_plan(n, g0, mc.L, nt)
        assert mleft > 0 and 32 // fsplit == ns, (cid, nT, nc, nfull, mleft, fsplit)
    assert all(32 // p[4] != 4 for n in range(1, 129) for p in ec.split_plan(n, 405, mc.L, 256) if p[4])
    assert (413 + mc.L - 1) % 64 == 0 and (414 + mc.L - 1) % 64 == 1
    for g0 in (405, 413, 414, 500):
        assert ec.sh_applies(g0, mc.L, ec.nt_of_class(g0), 4, 1500, 690)


@pytest.mark.parametrize("cid", list(CASES))
def test_one_candidate_per_gap_and_live_planes(cid, tmp_path_factory):
    """Every case has one candidate, G = G0 (so Wn and the tiles are what the case's name says), and the E-step placed reads."""
    o = oracle_of(cid, tmp_path_factory)
    g0 = o["case"].gaps[0].length
    (G, cnt, rmax), = o["planes"][0]
    assert G == g0 and cnt is not None and rmax is not None
    assert (cnt > 0).any() and (np.isfinite(rmax) & (rmax != 0)).any()


def test_windows_begin_and_end_inside_tiles_and_two_are_empty(tmp_path_factory):
    """Restated fig_window_u on the left-anchored reads: in `empty` exactly the two moved reads have hi < lo and the oracle's
    per-read maximum of exactly those is 0; in `w448` some window begins and ends strictly inside a tile of 64 placements."""
    o = oracle_of("empty", tmp_path_factory)
    _, pick = mc.case_empty()
    m = o["model"]
    batch = synth.case_to_batch(o["case"])
    (G, _, rmax), = o["planes"][0]
    win = mc.windows(batch, 0, int(m.Tmin), int(m.Tmax), G)
    assert sorted(s for s, lo, hi in win if hi < lo) == sorted(pick)
    assert all((rmax[s] == 0) == (hi < lo) for s, lo, hi in win), [(s, lo, hi, rmax[s]) for s, lo, hi in win]
    o = oracle_of("w448", tmp_path_factory)
    (G, _, _), = o["planes"][0]
    win = mc.windows(synth.case_to_batch(o["case"]), 0, int(o["model"].Tmin), int(o["model"].Tmax), G)
    inside = [(s, lo, hi) for s, lo, hi in win if hi >= lo and (lo + mc.L - 1) % 64 not in (0,) and (hi + mc.L - 1) % 64 != 63
              and lo > -(mc.L - 1) and hi < G - 1]
    assert inside, win


def test_mixed_case_holds_the_chunks_it_promises(tmp_path_factory):
    batch = synth.case_to_batch(oracle_of("mixed", tmp_path_factory)["case"])
    seqs = [bytes(batch.u_seq[int(batch.u_seq_off[s]):int(batch.u_seq_off[s + 1])]) for s in range(int(batch.u_read_off[1]))]
    irr = [b"N" in q or len(q) != mc.L for q in seqs]
    assert len(irr) == 70 and irr[mc.MIXED_N] and irr[mc.MIXED_SHORT] and len(seqs[mc.MIXED_SHORT]) == mc.L - 5
    assert sum(irr[:32]) == 2 and all(irr[32:64]) and not any(irr[64:])


@pytest.mark.parametrize("cid", list(CASES))
def test_emulation_equals_oracle_exactly(cid, tmp_path_factory):
    o = oracle_of(cid, tmp_path_factory)
    res, st = fill_with_planes(util.EMULIB, o["case"], o["model"], o["planes"])
    compare_with_oracle(o, res, st, 0.0)


# ---------------------------------------------------------------------------------------------------------------- GPU
def parent_record(res, st):
    return {"read_maxlv": [float(x).hex() for x in np.asarray(res.read_maxlv[0, 0]).reshape(-1)], "mle_exec_flops": float(st["mle_exec_flops"]).hex()}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_device_matches_oracle_in_the_shared_form(cid, tmp_path_factory, monkeypatch, capfd):
    """Default fill and FIG_ESTEP=pair fill against the oracle; the default fill's candidate took the shared form (its countsGap
    differs from the pair fill's in at least one bit).  For PARENT_IDS also: per-read maxima and mle_exec_flops equal to the
    parent library's, bit for bit."""
    o = oracle_of(cid, tmp_path_factory)
    a, sa, cls_a = _fill_logged(o, capfd, monkeypatch, pair=False)
    b, sb, cls_b = _fill_logged(o, capfd, monkeypatch, pair=True)
    assert "libfighip.so" in open("/proc/self/maps").read() and cls_a == cls_b
    compare_with_oracle(o, a, sa, 1e-6)
    compare_with_oracle(o, b, sb, 1e-6)
    g0 = o["case"].gaps[0].length
    assert ab_rule(o, a, b, cls_a, lambda g: g.length) == {(0, g0): "shared"}
    if cid in PARENT_IDS:
        want = json.load(open(FIXTURE))[cid]
        got = parent_record(a, sa)
        print("mle_exec_flops", float.fromhex(got["mle_exec_flops"]), "parent", float.fromhex(want["mle_exec_flops"]))
        assert got["mle_exec_flops"] == want["mle_exec_flops"]
        assert got["read_maxlv"] == want["read_maxlv"]
