"""The continuous form of the candidate-parallel scheduler against the two orders it must equal.

In the default order an eval workgroup that finishes the last item of a gap's chunk replays the gap inside the launch, publishes
the gap's next chunk (or its end item) for any workgroup of the launch, and the host's rounds only start the gaps and mop up
(fig_engine_sched.h: fig_item_continue; fig_abi.hip: fig_chunk_finished / fig_cont_publish / fig_cont_pop); it is the default in
unmapped mode and FIG_SCHED=continuous in partial mode, whose default stays the rounds.  FIG_SCHED=rounds is
the host-driven order (every chunk a round), FIG_SCHED=seq one workgroup per gap.  The arithmetic is the same kernels on the same
candidates in all three, so everything is compared for equality: strings, filled_len, gaptofill, candidate records with the
likelihood's bits, both numeric planes, per-gap placeReads counts, placeReads calls and algorithmic flops.

CPU: the one-lane emulation runs the continuous order through the same fig_item_* functions and the same chunk-size function
(tools/emu/fig_emu_abi.cpp); continuous == rounds == oracle, bit for bit, on an unmapped case whose gaps go through three or more
continuation generations and on a partial-mode case.
GPU: 1, 3 and 40 unmapped-mode gaps of 20-120 bp with at most 60 reads of 36-50 bp (100-150 candidates each: two or three chunks
of the 64 slots a gap has), and two partial-mode goldens: neg_overlap, whose gap 1 closes at its first candidate, and
partial_brackets.  The unmapped gaps of these sizes run their whole range (50 equal likelihoods in a row do not occur), so the
early stops come from a partial-mode case of 60 gaps of 70-99 bp at 3x coverage (`need`): every gap there stops after 36-90 of
its 350-500 candidates, most of them below the gap's original length, which sends the end item through run(originalGap).  With
FIG_ITEMS_PER_WG=1 FIG_MIN_CHUNK=1 the planner cuts chunks of a few dozen candidates, so these stops fall inside continued
chunks and the end items are continuations too.  What each case is there for is read from the results and asserted, so a
change of the generator cannot quietly empty the test.  No test here tries to make a workgroup wait, and nothing is repeated to
provoke anything."""
import os
import re

import numpy as np
import pytest

import util
from figbird_amd import api, synth
from tools import estep_cases as ec
from tools import partial_cases as pc
from test_planes import model_of, prepare

_KNOBS = ("FIG_SCHED", "FIG_LANES", "FIG_MIN_CHUNK", "FIG_ITEMS_PER_WG", "FIG_ESTEP", "FIG_SH_CHUNKS", "FIG_CONT_CAP", "FIG_CONT_LIVE", "FIG_CONT_PRIO",
          "FIG_EMU_CHUNK", "FIG_EMU_TILES")
MIN_CHUNK = 16                       # FIG_MIN_CHUNK's default (fig_abi_host.h)


def case_one():
    return synth.make_case("cont1", 11, "unmapped", [(3000, 20)], contig_len=7000, read_len=50, coverage=25, n_model_pairs=800, max_reads_per_gap=60)


def case_three():
    return synth.make_case("cont3", 12, "unmapped", [(2500, 20), (5000, 40), (7500, 120)], contig_len=10000, read_len=36, coverage=25, n_model_pairs=800,
                           max_reads_per_gap=48)


def case_forty():
    rng = np.random.default_rng(4040)
    lens = [int(x) for x in rng.integers(20, 121, size=40)]
    specs = [(2000 + 1800 * i, n) for i, n in enumerate(lens)]
    return synth.make_case("cont40", 13, "unmapped", specs, contig_len=2000 + 1800 * 40 + 2000, read_len=42, coverage=25, n_model_pairs=800, max_reads_per_gap=60)


def case_need():
    rng = np.random.default_rng(9090)
    lens = [int(x) for x in rng.integers(70, 100, size=60)]
    specs = [(2000 + 1500 * i, n) for i, n in enumerate(lens)]
    return synth.make_case("contneed", 21, "partial", specs, contig_len=2000 + 1500 * 60 + 2000, read_len=50, insert_mean=180, insert_sd=10, coverage=3, err=0.005,
                           n_model_pairs=600)


def candidate_range(case, G0):
    """findFrac (fig_gaprules.h: gap_alloc / gap_range, partial mode, float arithmetic as there) -> (first candidate length, number of candidates)."""
    assert case.mode == "partial"
    f = np.float32
    pl = case.partial_len
    f1, f2 = (f(.00001), f(3 * pl) / f(G0)) if G0 <= pl else (f(.00001), f(5.0)) if G0 <= 2 * pl else (f(1), f(1))
    lo, hi = int(f(G0) * f1), int(f(G0) * f2)
    return lo, max(1, hi - lo + 1)


CASES = {"one": case_one, "three": case_three, "forty": case_forty, "need": case_need}
_PREP = {}


def prepared(cid, tmp_path_factory):
    """The case, its written inputs and the host model: made once per case id and shared, read-only."""
    if cid not in _PREP:
        base = tmp_path_factory.mktemp("cont_" + cid)
        src = CASES[cid]() if cid in CASES else pc.all_cases()[cid]() if cid == "pn" else cid      # (else: the name of a fill golden)
        root, case = prepare(src, base)
        _PREP[cid] = dict(case=case, root=root, base=str(base), model=model_of(root), batch=synth.case_to_batch(case))
    return _PREP[cid]


def set_env(monkeypatch, **env):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def fill(lib_path, p, planes=None, eng=None):
    """One fill with the candidate records (and both planes, planes = (cols, reads)) -> (FillResult, fig_get_stats)."""
    own = eng is None
    if own:
        eng = api.Engine(0, lib_path=lib_path)
        eng.set_model(p["model"])
        eng.upload(p["batch"])
    cols, reads = planes if planes else (0, 0)
    res = eng.fill_resident(debug_cand=512, plane_cols=cols, plane_reads=reads)
    st = eng.stats()
    if own:
        eng.free_batch()
        eng.close()
    return res, st


def plane_shape(p, res):
    off = p["batch"].u_read_off if p["case"].mode == "unmapped" else p["batch"].p_read_off
    return max(c[0] for g in range(len(p["case"].gaps)) for c in res.cand[g]) + 1, int(np.diff(off).max()) + 1


def assert_same_fill(a, sa, b, sb, n_gaps, what):
    assert a.strings == b.strings, what
    assert list(a.filled_len) == list(b.filled_len) and list(a.gaptofill) == list(b.gaptofill), what
    assert list(a.n_place) == list(b.n_place), what
    for g in range(n_gaps):
        assert len(a.cand[g]) == len(b.cand[g]), f"{what}: gap {g}: candidate count"
        for x, y in zip(a.cand[g], b.cand[g]):
            assert tuple(x[:3]) == tuple(y[:3]), f"{what}: gap {g}"
            assert np.float64(x[3]).tobytes() == np.float64(y[3]).tobytes(), f"{what}: gap {g}: {x} vs {y}"
    if a.counts is not None or b.counts is not None:
        for g in range(n_gaps):
            for k, c in enumerate(a.cand[g]):
                assert a.counts[g, k, :c[0]].tobytes() == b.counts[g, k, :c[0]].tobytes(), f"{what}: gap {g} G={c[0]}: countsGap"
                assert a.read_maxlv[g, k].tobytes() == b.read_maxlv[g, k].tobytes(), f"{what}: gap {g} G={c[0]}: per-read maxima"
    assert sa["place_calls"] == sb["place_calls"], what
    assert sa["alg_flops"] == sb["alg_flops"], what


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("cid", ["three", "need"])
def test_chunk_of_a_continuation(cid, tmp_path_factory, monkeypatch):
    """fig_cont_chunk = min(max(FIG_MIN_CHUNK, the gap's last chunk), slots per gap, candidates left), counted exactly.  With
    FIG_EMU_CHUNK=c the emulation's first chunk of a gap is min(c, 64 slots, range) and fig_cont_chunk must keep that size, so a
    gap whose loop ended at candidate index e (the last one its bookkeeping consumed; every candidate here is recorded) was cut into
    ceil((e + 1) / min(c, 64)) chunks, all but the first continued: cont_chunks must equal the sum over the gaps.  A chunk
    function that returned anything else -- smaller, larger, or past the slots -- changes the count."""
    p = prepared(cid, tmp_path_factory)
    n = len(p["case"].gaps)
    for c in (3, 16, 64, 100):
        set_env(monkeypatch, FIG_SCHED="continuous", FIG_EMU_CHUNK=str(c))
        res, st = fill(util.EMULIB, p)
        consumed = [len(res.cand[g]) for g in range(n)]
        assert min(consumed) > 0
        want = sum(-(-e // min(c, 64)) - 1 for e in consumed)
        print(cid, "FIG_EMU_CHUNK", c, "cont_chunks", st["cont_chunks"], "expected", want)
        assert st["cont_chunks"] == want, c


@pytest.mark.parametrize("cid", ["three", "pn"])
def test_emulation_orders_agree_with_the_oracle(cid, tmp_path_factory, monkeypatch):
    """Continuous == rounds == seq == oracle through the one-lane emulation, bit for bit, planes included; the unmapped case's gaps
    run through three or more continuation generations each where they have the candidates for it."""
    p = prepared(cid, tmp_path_factory)
    n = len(p["case"].gaps)
    tr = os.path.join(p["base"], "o.trace")
    r = util.run_oracle_figbird(p["root"], trace=tr, level=3)
    assert r.returncode == 0, r.stderr
    cands, _ = util.parse_trace(tr)
    stats = [ln.rstrip("\n").split("\t")[1:3] for ln in open(tr) if ln.startswith("STATS")]
    gapout = [ln.split("\t") for ln in util.read(os.path.join(p["root"], "tmp", "gapout0.txt")).splitlines()]
    gtf = [int(x) for x in util.read(os.path.join(p["root"], "tmp", "gaptofill0.txt")).split()]
    from test_planes import compare_planes, parse_planes
    planes = parse_planes(tr)

    set_env(monkeypatch, FIG_SCHED="rounds")
    first, _ = fill(util.EMULIB, p)
    shape = plane_shape(p, first)
    fills = {}
    for name, env in {"continuous": {"FIG_SCHED": "continuous"}, "rounds": {"FIG_SCHED": "rounds"}, "seq": {"FIG_SCHED": "seq"}, "continuous_chunk16": {"FIG_SCHED": "continuous", "FIG_EMU_CHUNK": "16"},
                      "continuous_chunk3": {"FIG_SCHED": "continuous", "FIG_EMU_CHUNK": "3"}}.items():
        set_env(monkeypatch, **env)
        fills[name] = fill(util.EMULIB, p, shape)
    base, sb = fills["rounds"]
    assert sb["cont_chunks"] == 0 and fills["seq"][1]["cont_chunks"] == 0
    for name in ("continuous", "seq", "continuous_chunk16", "continuous_chunk3"):
        assert_same_fill(base, sb, *fills[name], n, name)
    # against the oracle, exactly
    res, st = fills["continuous"]
    assert [int(e[4]) for e in gapout] == list(res.filled_len) and [e[5] if len(e) > 5 else "" for e in gapout] == res.strings and gtf == list(res.gaptofill)
    for g, cs in cands.items():
        assert [(G, it, v) for G, it, _, v in cs] == [tuple(c[:3]) for c in res.cand[g]], f"gap {g}"
        for (_, _, lik, _), c in zip(cs, res.cand[g]):
            assert lik == c[3] or (np.isnan(lik) and np.isnan(c[3])), f"gap {g}"
    compare_planes(res, planes, 0.0)
    assert st["place_calls"] == int(stats[0][0]) and st["alg_flops"] == float(stats[0][1])
    # generations: a gap that consumed c candidates in chunks of exactly 16 (FIG_EMU_CHUNK) was continued at least ceil(c / 16) - 1 times
    gens = [max(0, -(-len(res.cand[g]) // MIN_CHUNK) - 1) for g in range(n)]
    print(cid, "candidates consumed per gap", [len(res.cand[g]) for g in range(n)], "cont_chunks", st["cont_chunks"], "chunk 16:", fills["continuous_chunk16"][1]["cont_chunks"],
          "chunk 3:", fills["continuous_chunk3"][1]["cont_chunks"])
    assert fills["continuous_chunk16"][1]["cont_chunks"] == sum(gens)       # (exact: test_chunk_of_a_continuation says why)
    if cid == "three":
        assert max(gens) >= 3, gens
    else:
        assert st["cont_chunks"] >= 1


# ---------------------------------------------------------------------------------------------------------------- GPU
def _native():
    return "libfighip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one", "three", "forty", "neg_overlap", "partial_brackets"])
def test_three_orders_agree_on_the_device(cid, tmp_path_factory, monkeypatch):
    """Default against FIG_SCHED=rounds against FIG_SCHED=seq, and the default's variants: an entry array of one entry (the gap
    is handed back to the host's rounds), continuations handed out oldest first, and every chunk continued however few
    workgroups are left (FIG_CONT_LIVE=0: with one gap, one workgroup then feeds on the gap's chain alone).  Two fills in a row on
    the resident batch are identical (stale entries or counters would show)."""
    p = prepared(cid, tmp_path_factory)
    n = len(p["case"].gaps)
    eng = api.Engine(0)
    eng.set_model(p["model"])
    set_env(monkeypatch)
    eng.upload(p["batch"])
    try:
        first, _ = fill(None, p, eng=eng)
        assert _native()
        shape = plane_shape(p, first) if cid != "forty" else None       # (40 gaps x 512 records x 5 x columns doubles: the planes stay with the small shapes)
        # the continuous form is the default in unmapped mode only (fig_knobs_from_env): the partial-mode cases ask for it
        on = {} if p["case"].mode == "unmapped" else {"FIG_SCHED": "continuous"}
        settings = {"default": on, "default_again": on, "rounds": {"FIG_SCHED": "rounds"}, "seq": {"FIG_SCHED": "seq"}, "cap1": dict(on, FIG_CONT_CAP="1"),
                    "fifo": dict(on, FIG_CONT_PRIO="0"), "live0": dict(on, FIG_CONT_LIVE="0")}
        if on:
            settings["mode_default"] = {}
        fills = {}
        for name, env in settings.items():
            set_env(monkeypatch, **env)
            fills[name] = fill(None, p, shape, eng=eng)
            st = fills[name][1]
            print(f"{cid} {name}: launches {st['n_launches']} cont_chunks {st['cont_chunks']} alg_flops {st['alg_flops']:.6g} spec_flops {st['spec_flops']:.6g} kernel {st['kernel_ms']:.1f} ms")
    finally:
        eng.free_batch()
        eng.close()
    base, sb = fills["rounds"]
    for name in settings:
        assert_same_fill(base, sb, *fills[name], n, f"{cid}: {name} against rounds")
    # evidence that each path ran
    assert sb["cont_chunks"] == 0 and fills["seq"][1]["cont_chunks"] == 0
    if "mode_default" in fills:
        assert fills["mode_default"][1]["cont_chunks"] == 0 and fills["mode_default"][1]["n_launches"] == sb["n_launches"]      # partial mode: the rounds
    consumed = [len(base.cand[g]) for g in range(n)]
    print(cid, "candidates consumed per gap", consumed)
    assert max(consumed) > 64                                         # some gap needs more than the 64 slots of its first chunk
    assert fills["live0"][1]["cont_chunks"] > 0 and fills["live0"][1]["n_launches"] < sb["n_launches"]
    assert fills["cap1"][1]["cont_chunks"] <= fills["cap1"][1]["n_launches"]       # one entry per eval launch at the most
    for name in ("default", "default_again", "fifo", "cap1"):
        assert fills[name][1]["n_launches"] < sb["n_launches"], name      # (at the least, the replay launches are gone)
    if cid == "forty":
        # Ten items per workgroup: chunks end while most of the launch is still at work.  (With 1 or 3 gaps every workgroup holds one
        # item of the gaps' first chunks, they end together, and the one that replays a gap finds the launch gone: by default
        # it publishes nothing and the host's next round takes the gap, which is what keeps a chain of chunks from running in one
        # workgroup -- 144 ms against 15 ms for the 1-gap case under FIG_CONT_LIVE=0.)
        for name in ("default", "default_again", "fifo"):
            assert fills[name][1]["cont_chunks"] > 0, name
    if cid == "neg_overlap":
        assert base.gaptofill[1] != 0 and consumed[1] == 0 and base.filled_len[1] == 0      # closes at its first candidate
    if cid == "forty":
        assert all(c > 64 for c in consumed)                          # every gap goes past the 64 slots of its first chunk


_CHUNK_RE = re.compile(r"\[figsched\] capG=\d+ round 1: active=(\d+) chunk=(\d+) items=(\d+)")


@pytest.mark.gpu
def test_early_stop_and_fallback_end_item_inside_the_launch(tmp_path_factory, monkeypatch, capfd):
    """The `need` case in the continuous form with small chunks (FIG_ITEMS_PER_WG=1 FIG_MIN_CHUNK=1; the first round's largest chunk
    is read from the library's round log, and a continued chunk is never larger: fig_cont_chunk keeps the gap's size).
    From the candidate records: every gap stops before the end of its range (candidate_range restates findFrac), at an index past
    the largest chunk for most of them -- the stop fell in a continued chunk, and what that chunk evaluated past it is discarded
    (executed flops above the useful ones, the useful ones equal in every order).  A gap that stopped below its original length
    needs run(originalGap) in its end item: exactly three placeReads calls beyond its candidates' (three EM iterations each).
    Under FIG_CONT_LIVE=0 the whole fill is, per launch class, the begin launch and ONE eval launch -- no end launch, no replay
    launch -- so those end items ran as continuations inside the launch."""
    p = prepared("need", tmp_path_factory)
    case, n = p["case"], len(p["case"].gaps)
    small = {"FIG_ITEMS_PER_WG": "1", "FIG_MIN_CHUNK": "1"}
    settings = {"rounds": dict(small, FIG_SCHED="rounds"), "seq": {"FIG_SCHED": "seq"}, "continuous": dict(small, FIG_SCHED="continuous"),
                "continuous_live0": dict(small, FIG_SCHED="continuous", FIG_CONT_LIVE="0")}
    eng = api.Engine(0)
    eng.set_model(p["model"])
    set_env(monkeypatch)
    eng.upload(p["batch"])
    fills, chunk = {}, {}
    try:
        for name, env in settings.items():
            set_env(monkeypatch, FIG_SCHED_LOG="1", **env)
            capfd.readouterr()
            fills[name] = fill(None, p, eng=eng)
            m = _CHUNK_RE.findall(capfd.readouterr().err)
            chunk[name] = max(int(x[1]) for x in m) if m else None
            st = fills[name][1]
            print(f"need {name}: launches {st['n_launches']} cont_chunks {st['cont_chunks']} first-round chunk {chunk[name]} alg_flops {st['alg_flops']:.6g} spec_flops {st['spec_flops']:.6g} kernel {st['kernel_ms']:.1f} ms")
    finally:
        eng.free_batch()
        eng.close()
    assert _native()
    base, sb = fills["rounds"]
    for name in settings:
        assert_same_fill(base, sb, *fills[name], n, f"need: {name} against rounds")
    res, st = fills["continuous_live0"]
    N = chunk["continuous_live0"]
    assert N is not None and 1 <= N < 64
    consumed = [len(res.cand[g]) for g in range(n)]
    ranges = [candidate_range(case, g.length) for g in case.gaps]
    assert all(res.cand[g][0][0] == ranges[g][0] for g in range(n))
    stopped = [g for g in range(n) if 0 < consumed[g] < ranges[g][1]]
    in_continued = [g for g in stopped if consumed[g] > N]
    below = [g for g in range(n) if consumed[g] > 0 and res.cand[g][-1][0] < case.gaps[g].length and res.gaptofill[g] == 0]
    extra = [int(res.n_place[g]) - sum(c[1] + 1 for c in res.cand[g]) for g in range(n)]
    print("need: consumed", consumed, "first-round chunk", N, "stopped", len(stopped), "in a continued chunk", len(in_continued), "below G0", len(below))
    assert len(stopped) == n and len(in_continued) >= n // 2
    assert len(below) >= n // 2 and any(g in in_continued for g in below)
    assert all(c[1] == 2 for g in range(n) for c in res.cand[g])      # three EM iterations per candidate: it + 1 placeReads calls
    assert all(extra[g] == (3 if g in below else 0) for g in range(n)), extra
    # inside the launch: per launch class (the gaps of 90 bp and more have candidates past 448 columns: two classes, restated by
    # tools/partial_cases.gmax_partial and tools/estep_cases.CLASS_CAPS) the begin launch and ONE eval launch, continued chunks,
    # no end launch
    classes = {min(c for c in ec.CLASS_CAPS if c >= pc.gmax_partial(g.length, case.read_len)) for g in case.gaps}
    assert len(classes) == 2
    assert st["n_launches"] == 2 * len(classes) and st["cont_chunks"] >= sum(-(-consumed[g] // N) - 1 for g in range(n))
    assert fills["continuous"][1]["cont_chunks"] > 0 and fills["continuous"][1]["n_launches"] < sb["n_launches"]
    assert sb["cont_chunks"] == 0
    for name in ("continuous", "continuous_live0"):
        assert fills[name][1]["spec_flops"] > fills[name][1]["alg_flops"] == sb["alg_flops"], name
