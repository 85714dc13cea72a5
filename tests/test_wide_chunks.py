"""Wide chunks of the continuous scheduler (FIG_WIDE, FIG_SLOTS_WIDE): a gap that keeps running gets wider chunks.

The rule is one function, fig_wide_chunk (fig_engine_sched.h), for the kernel's continuation (fig_item_continue), the host's
round planner (fig_plan_round, for a gap that comes back with j > 0) and the one-lane emulation.  A gap owns min(its candidates,
W) slots of its persistent slab instead of 64.  Which candidate is evaluated when changes, and nothing else: every order is
compared for equality with FIG_SCHED=rounds and FIG_SCHED=seq by test_continuous_sched.assert_same_fill (strings, lengths,
candidate records with the likelihood's bits, planes, per-gap placeReads counts, placeReads calls, algorithmic flops).

CPU: the rule and the planner as pure functions through the emulation's shims; the emulation under FIG_WIDE=grow with small
chunks and a small wide cap, where several doublings, the cap and slot indices past the first chunk's width all occur and the
number of continued chunks is predicted exactly; a stand-alone program built with -fsanitize=address,undefined that lays out
persistent slabs of random sizes (tools/probe/persist_layout_check.cpp).
GPU: the shapes of test_continuous_sched under every FIG_WIDE, again with small first chunks, twice on the resident batch, and
with a wide cap below the gaps' ranges.  Nothing here tries to make a workgroup wait, and nothing is repeated to provoke anything."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import util
from figbird_amd import api
from test_continuous_sched import _native, assert_same_fill, candidate_range, fill, plane_shape, prepared, set_env as _set_env

GROW, IDLE = 1, 2                    # FIG_WIDE_GROW, FIG_WIDE_IDLE (fig_engine_sched.h)
_WIDE_KNOBS = ("FIG_WIDE", "FIG_SLOTS_WIDE", "FIG_WIDE_MAX_ACTIVE", "FIG_SCHED_LOG")


def set_env(monkeypatch, **env):
    for k in _WIDE_KNOBS:
        monkeypatch.delenv(k, raising=False)
    _set_env(monkeypatch, **env)


# ---------------------------------------------------------------------------------------------------------------- the rule
def _lib():
    lib = ctypes.CDLL(util.EMULIB)
    lib.fig_emu_cont_chunk.restype = lib.fig_emu_wide_chunk.restype = lib.fig_emu_wide_rank.restype = ctypes.c_int
    lib.fig_emu_cont_chunk.argtypes = [ctypes.c_int] * 4
    lib.fig_emu_wide_chunk.argtypes = [ctypes.c_int] * 9
    lib.fig_emu_wide_rank.argtypes = [ctypes.c_int] * 7
    return lib


def test_chunk_rule_as_a_pure_function():
    """Over random (mode, minc, last, base, W, slots, left, consumed_all, spare): never above the gap's slots, W or what is left;
    with the widening off, or after a chunk that was not consumed to its end, exactly today's fig_cont_chunk within the base
    slots; never below that (no ratchet down); with growth alone at most twice the last chunk (or today's, where FIG_MIN_CHUNK
    asks for more); with idle alone at most the spare workgroups (or today's).  The rank is the number of chunks the rule cuts
    `left` into."""
    lib = _lib()
    rng = np.random.default_rng(20260102)
    seen = {"grown": 0, "idle": 0, "cap": 0, "same": 0}
    for it in range(6000):
        base = int(rng.choice([1, 3, 16, 64]))
        W = int(max(base, rng.choice([base, 24, 64, 128, 256, 512])))
        rangecap = int(rng.integers(1, 900))
        slots = max(1, min(rangecap, W))                       # what the packer gives the gap
        left = int(rng.integers(1, rangecap + 1))
        minc = int(rng.choice([1, 3, 16, 64, 100]))
        last = int(rng.integers(1, W + 1))
        mode = int(rng.integers(0, 4))
        consumed_all = int(rng.integers(0, 4) != 0)
        spare = int(rng.integers(0, 600))
        today = lib.fig_emu_cont_chunk(minc, last, min(slots, base), left)
        n = lib.fig_emu_wide_chunk(mode, minc, last, base, W, slots, left, consumed_all, spare)
        what = (mode, minc, last, base, W, slots, left, consumed_all, spare, today, n)
        assert 1 <= n <= min(slots, W, left), what
        assert n >= today, what
        if mode == 0 or not consumed_all:
            assert n == today, what
            continue
        bound = today
        if mode & GROW:
            bound = max(bound, 2 * last)
        if mode & IDLE:
            bound = max(bound, spare)
        assert n <= bound, what
        assert n == max(today, min(bound, slots, W, left)), what      # and it takes what the rule allows
        seen["grown"] += mode == GROW and n > today
        seen["idle"] += mode == IDLE and n > today
        seen["cap"] += n in (W, slots) and n < bound
        seen["same"] += n == today
        # the rank: chunks of the chain under the rule in force, nothing idle
        if it % 8:
            continue
        r, l, k = 0, left, n
        while l > 0:
            r += 1; l -= k
            k = lib.fig_emu_wide_chunk(mode, minc, k, base, W, slots, l, 1, 0) if l > 0 else 0
        assert lib.fig_emu_wide_rank(mode, minc, n, base, W, slots, left) == r, what
    print(seen)
    assert all(v > 100 for v in seen.values()), seen
    # the doubling the unmapped gaps of the bench set see: 64, 128, 256, 256, 97 for 801 candidates
    sizes, left, last = [64], 801 - 64, 64
    while left > 0:
        last = lib.fig_emu_wide_chunk(GROW, 16, last, 64, 256, 256, left, 1, 0)
        sizes.append(last); left -= last
    assert sizes == [64, 128, 256, 256, 97]
    assert lib.fig_emu_wide_rank(GROW, 16, 128, 64, 256, 256, 801 - 64) == 4 and lib.fig_emu_wide_rank(0, 16, 64, 64, 256, 256, 801 - 64) == 12


def _plan(lib, ids, ctl, capacity, nsplit, slots_cap, wide_mode, wide_cap, minc, ipw, n_active_max, shim="fig_emu_plan_round_wide", max_active=96):
    ids_a = np.asarray(ids, dtype=np.int32); ctl_a = np.asarray(ctl, dtype=np.int32).reshape(-1)
    cap_ints = 4 * (len(ids) * (max(slots_cap, wide_cap) + 1) + 1)
    items = np.zeros(cap_ints, dtype=np.int32); entries = np.zeros(cap_ints, dtype=np.int32)
    nam, n_items, n_ent, chunk = (ctypes.c_int(v) for v in (n_active_max, 0, 0, 0))
    i32p, ip = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)
    head = [ids_a.ctypes.data_as(i32p), len(ids), ctl_a.ctypes.data_as(i32p), capacity, nsplit, slots_cap]
    tail = [minc, ipw, ctypes.byref(nam), items.ctypes.data_as(i32p), ctypes.byref(n_items), entries.ctypes.data_as(i32p), ctypes.byref(n_ent), cap_ints, ctypes.byref(chunk)]
    fn = getattr(lib, shim)
    fn.restype = ctypes.c_int
    wide = [wide_mode, wide_cap, max_active] if shim.endswith("_wide") else []
    fn.argtypes = [i32p, ctypes.c_int, i32p] + [ctypes.c_int] * (3 + len(wide)) + [ctypes.c_int, ctypes.c_double, ip, i32p, ip, i32p, ip, ctypes.c_int, ip]
    n_active = fn(*(head + wide + tail))
    assert n_active >= 0
    its = items[:4 * n_items.value].reshape(-1, 4).tolist(); ent = entries[:4 * n_ent.value].reshape(-1, 4).tolist()
    # items and entries agree whatever the chunk sizes: per entry, n items of the gap, candidates j .. j+n-1 into slots 0 .. n-1
    pos = 0
    for g, n, _, _ in ent:
        mine = its[pos:pos + n]; pos += n
        assert sorted((i[1], i[2]) for i in mine) == [(ctl[g][1] + k, k) for k in range(n)] and all(i[0] == g for i in mine)
    assert pos == len(its) and chunk.value == max([e[1] for e in ent], default=0)
    return n_active, nam.value, its, ent, chunk.value


def test_planner_with_a_wide_cap():
    """fig_plan_round with the wide cap as an argument of its own.  Identical to the planner without it when the wide cap equals
    slots_cap, when FIG_WIDE is 0, and for every gap with j == 0 (a gap's first chunk is never widened); a gap with j > 0 grows
    to twice its last chunk (FigGapCtl::last) within the wide cap and what it has left; idle widening happens only in a round
    that admits every active gap and holds fewer items than the lane's share of workgroups, and hands out no more than that.
    Growth is off for a lane whose active set has been above FIG_WIDE_MAX_ACTIVE (here: 0, and a lane of 120 gaps under the
    default 96); idle widening is not gated."""
    lib = ctypes.CDLL(util.EMULIB)
    rng = np.random.default_rng(7)
    widened_grow = widened_idle = full_rounds = 0
    for _ in range(400):
        ng = int(rng.integers(1, 30))
        ctl = []
        for g in range(ng):
            rangec = int(rng.integers(1, 900)); st = int(rng.choice([0, 1, 1, 1, 2]))
            j = int(rng.integers(0, rangec + 1)) if rng.integers(0, 3) else 0
            ctl.append([st, j, rangec, int(rng.choice([0, 16, 64, 128])) if j else 0])
        ids = [int(x) for x in rng.permutation(ng)]
        capacity, nsplit, minc, ipw = int(rng.choice([4, 64, 512, 2048])), int(rng.choice([1, 2])), int(rng.choice([1, 16])), float(rng.choice([1.0, 12.0]))
        slots_cap, W = 64, int(rng.choice([128, 256]))
        old = _plan(lib, ids, ctl, capacity, nsplit, slots_cap, 0, 0, minc, ipw, 0, shim="fig_emu_plan_round")
        for mode, cap in ((0, W), (GROW, slots_cap), (IDLE, slots_cap), (GROW | IDLE, slots_cap)):
            assert _plan(lib, ids, ctl, capacity, nsplit, slots_cap, mode, cap, minc, ipw, 0) == old, (mode, cap)
        assert _plan(lib, ids, ctl, capacity, nsplit, slots_cap, GROW, W, minc, ipw, 0, max_active=0) == old
        assert _plan(lib, ids, ctl, capacity, nsplit, slots_cap, GROW | IDLE, W, minc, ipw, 0, max_active=0) == _plan(lib, ids, ctl, capacity, nsplit, slots_cap, IDLE, W, minc, ipw, 0)
        base_n = {e[0]: e[1] for e in old[3]}
        for mode in (GROW, IDLE, GROW | IDLE):
            new = _plan(lib, ids, ctl, capacity, nsplit, slots_cap, mode, W, minc, ipw, 0)
            assert new[0] == old[0]
            grown = {}
            for g, n, _, _ in new[3]:
                st, j, rangec, last = ctl[g]
                assert n <= min(W, rangec - j), (g, n, ctl[g])
                if j == 0 or g not in base_n:
                    continue
                want = base_n[g]
                if (mode & GROW) and want > 0:
                    want = max(want, min(2 * last, W, rangec - j))
                grown[g] = want
                assert n >= base_n[g] and (n == want or (mode & IDLE and n > want)), (mode, g, n, want, ctl[g])
                widened_grow += mode == GROW and n > base_n[g]
            for g, n, _, _ in new[3]:
                if ctl[g][1] == 0 and g in base_n:
                    assert n == base_n[g], "a first chunk was widened"
            extra = sum(n - grown.get(g, n) for g, n, _, _ in new[3])
            if extra:
                total = sum(e[1] for e in new[3])
                assert mode & IDLE and len(new[3]) == new[0] and total <= capacity // nsplit, (mode, extra, total, capacity, nsplit)
                widened_idle += 1
            full_rounds += len(new[3]) < new[0]
    print("widened by growth", widened_grow, "by idle workgroups", widened_idle, "rounds that left gaps waiting", full_rounds)
    # a lane of 120 active gaps, every one with 64 of 300 candidates behind it: grown at FIG_WIDE_MAX_ACTIVE=120, not at the default 96
    ctl = [[1, 64, 300, 64] for _ in range(120)]
    args = (lib, list(range(120)), ctl, 100000, 1, 64)
    plain = _plan(*args, 0, 0, 16, 12.0, 0, shim="fig_emu_plan_round")
    assert _plan(*args, GROW, 256, 16, 12.0, 0) == plain and all(e[1] == 64 for e in plain[3])
    assert all(e[1] == 128 for e in _plan(*args, GROW, 256, 16, 12.0, 0, max_active=120)[3])
    assert widened_grow > 50 and widened_idle > 20 and full_rounds > 20


# ---------------------------------------------------------------------------------------------------------------- emulation
def grow_schedule(consumed, c, W):
    """Chunks of a gap of the emulation under FIG_EMU_CHUNK=c, FIG_WIDE=grow, FIG_SLOTS_WIDE=W (W below every range here) that
    consumed `consumed` candidates: c, then twice the last one within W, until the stop is covered."""
    sizes, n = [], min(c, 64)
    while sum(sizes) < consumed:
        sizes.append(n)
        n = max(n, min(2 * n, max(W, min(c, 64))))
    return sizes


@pytest.mark.parametrize("cid", ["three", "need"])
def test_emulation_grows_chunks_and_fills_the_same(cid, tmp_path_factory, monkeypatch):
    """`three` (unmapped, every gap runs its whole range) and `need` (partial, every gap stops early) under FIG_WIDE=grow with
    FIG_EMU_CHUNK 3 and 16 and FIG_SLOTS_WIDE=24 (the emulation's base width is the chunk, so the cap may lie below 64):
    3 -> 6 -> 12 -> 24 -> 24 ... and 16 -> 24 -> 24 ...  Equal to the rounds form and to seq; `three` equal to the oracle;
    cont_chunks exactly the count the growth schedule predicts from the candidates each gap consumed; for `need` the stops
    fall inside grown chunks."""
    p = prepared(cid, tmp_path_factory)
    n = len(p["case"].gaps)
    W = 24
    set_env(monkeypatch, FIG_SCHED="rounds")
    shape = None                     # (the planes are compared on the device, where a fill takes milliseconds)
    base = fill(util.EMULIB, p, shape)
    set_env(monkeypatch, FIG_SCHED="seq")
    seq = fill(util.EMULIB, p, shape)
    assert_same_fill(*base, *seq, n, "seq")
    consumed = [len(base[0].cand[g]) for g in range(n)]
    for c in (3, 16):
        set_env(monkeypatch, FIG_SCHED="continuous", FIG_EMU_CHUNK=str(c), FIG_WIDE="grow", FIG_SLOTS_WIDE=str(W))
        got = fill(util.EMULIB, p, shape)
        assert_same_fill(*base, *got, n, f"{cid}: grow, chunk {c}")
        sched = [grow_schedule(e, c, W) for e in consumed]
        want = sum(len(s) - 1 for s in sched)
        set_env(monkeypatch, FIG_SCHED="continuous", FIG_EMU_CHUNK=str(c))
        fixed = fill(util.EMULIB, p)[1]["cont_chunks"]
        print(cid, "chunk", c, "cont_chunks", got[1]["cont_chunks"], "predicted", want, "fixed sizes", fixed, "largest chunk", max(max(s) for s in sched))
        assert got[1]["cont_chunks"] == want
        assert fixed == sum(-(-e // c) - 1 for e in consumed) > want      # (FIG_WIDE not set under FIG_EMU_CHUNK: fixed sizes)
        assert max(max(s) for s in sched) == W > c and any(s.count(W) >= 2 for s in sched)      # doublings up to the cap, which binds: slot indices past the first chunk's width
        if cid == "need":
            ranges = [candidate_range(p["case"], g.length)[1] for g in p["case"].gaps]
            assert all(0 < e < r for e, r in zip(consumed, ranges))      # every gap stops early ...
            assert all(len(s) >= 2 and s[-1] > c and sum(s) >= e for s, e in zip(sched, consumed))      # ... inside a grown chunk ...
            assert sum(sum(s) > e for s, e in zip(sched, consumed)) >= n // 2                          # ... most of them with candidates of it discarded
    if cid == "three":
        tr = os.path.join(p["base"], "wide.trace")
        r = util.run_oracle_figbird(p["root"], trace=tr, level=1)
        assert r.returncode == 0, r.stderr
        cands, _ = util.parse_trace(tr)
        gapout = [ln.split("\t") for ln in util.read(os.path.join(p["root"], "tmp", "gapout0.txt")).splitlines()]
        res = got[0]
        assert [int(e[4]) for e in gapout] == list(res.filled_len) and [e[5] if len(e) > 5 else "" for e in gapout] == res.strings
        for g, cs in cands.items():
            assert [(G, it, v) for G, it, _, v in cs] == [tuple(x[:3]) for x in res.cand[g]], f"gap {g}"
            assert all(lik == x[3] or (np.isnan(lik) and np.isnan(x[3])) for (_, _, lik, _), x in zip(cs, res.cand[g])), f"gap {g}"


def test_defaults_grow_in_unmapped_mode_and_nothing_in_partial_mode(tmp_path_factory, monkeypatch):
    """Unmapped (`three`): the default is FIG_WIDE=grow, FIG_WIDE=0 cuts more chunks, the rounds form never widens, and growth is
    off with FIG_WIDE_MAX_ACTIVE=0.  Partial (`need`, FIG_SCHED=continuous): the default is FIG_WIDE=0; grow must be asked for."""
    for cid, on in (("three", {}), ("need", {"FIG_SCHED": "continuous"})):
        p = prepared(cid, tmp_path_factory)
        n = len(p["case"].gaps)
        out = {}
        for name, env in {"default": on, "off": dict(on, FIG_WIDE="0"), "grow": dict(on, FIG_WIDE="grow"), "gated": dict(on, FIG_WIDE="grow", FIG_WIDE_MAX_ACTIVE="0"),
                          "rounds_both": {"FIG_SCHED": "rounds", "FIG_WIDE": "both"}}.items():
            set_env(monkeypatch, **env)
            out[name] = fill(util.EMULIB, p)
        for name in out:
            assert_same_fill(*out["off"], *out[name], n, name)
        cc = {k: v[1]["cont_chunks"] for k, v in out.items()}
        print(cid, cc)
        assert cc["rounds_both"] == 0 and 0 < cc["grow"] < cc["off"] == cc["gated"]
        assert cc["default"] == (cc["grow"] if cid == "three" else cc["off"])


# ---------------------------------------------------------------------------------------------------------------- layout
def test_persistent_slab_layout_under_the_sanitizers(tmp_path):
    """tools/probe/persist_layout_check.cpp, a program of its own built with -fsanitize=address,undefined: for random (capGg, nU,
    nP, range, slots up to W) every array and every slot of fig_persist_layout is written in full inside an allocation of exactly
    the returned size, nothing overlaps and the last slot ends at the size; the packer's per-gap offsets and slot counts
    (fig_pack_persist) the same way."""
    exe = str(tmp_path / "persist_layout_check")
    src = os.path.join(util.ROOT, "tools", "probe", "persist_layout_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "persist layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------- GPU
_ROUND_RE = re.compile(r"\[figsched\] capG=(\d+) round (\d+): active=\d+ chunk=(\d+) items=(\d+) blocks=(\d+)")
_SLAB_RE = re.compile(r"\[figsched\] persistent slab: (\d+) B with (\d+) base slots per gap, (\d+) B with min\(candidates, (\d+)\) slots per gap")
_NARROW_RE = re.compile(r"\[figsched\] widened chunks narrowed to the live workgroups: (\d+)")
MODES = ("0", "grow", "idle", "both")
HAND_BACK = "100000"                 # FIG_CONT_LIVE so high that no chunk is ever continued in the launch: every gap goes back to the host's planner


class Run:
    """One upload, then one fill per setting: fills, per launch class (its capG) the largest chunk of round 1, 2, ... and the items
    and workgroups of round 1 (the log line of round r + 1 reports round r), the narrowed-chunk count, the upload's slab line."""

    def __init__(self, p, monkeypatch, capfd, upload_env, settings):
        self.fills, self.chunks, self.items1, self.blocks, self.narrowed, lines = {}, {}, {}, {}, {}, []
        eng = api.Engine(0)
        eng.set_model(p["model"])
        set_env(monkeypatch, FIG_SCHED_LOG="1", **upload_env)
        capfd.readouterr()
        eng.upload(p["batch"])
        self.slab = _SLAB_RE.search(capfd.readouterr().err)
        try:
            for name, env in settings.items():
                set_env(monkeypatch, FIG_SCHED_LOG="1", **env)
                capfd.readouterr()
                self.fills[name] = fill(None, p, eng=eng)
                err = capfd.readouterr().err
                self.chunks[name] = {}
                for capg, r, ch, items, blocks in _ROUND_RE.findall(err):
                    if int(r) > 0:
                        self.chunks[name].setdefault(int(capg), []).append(int(ch))
                    if int(r) == 1:
                        self.items1[int(capg)], self.blocks[int(capg)] = int(items), int(blocks)
                m = _NARROW_RE.search(err)
                self.narrowed[name] = int(m.group(1)) if m else None
                st = self.fills[name][1]
                lines.append(f"{name}: launches {st['n_launches']} cont_chunks {st['cont_chunks']} round chunks {self.chunks[name]} narrowed {self.narrowed[name]} spec_flops {st['spec_flops']:.6g} kernel {st['kernel_ms']:.1f} ms")
        finally:
            eng.free_batch()
            eng.close()
        print("\n".join(lines))
        assert _native()
        self.cc = {k: v[1]["cont_chunks"] for k, v in self.fills.items()}

    def every(self, name):
        return [c for v in self.chunks[name].values() for c in v]

    def later(self, name):
        return [c for v in self.chunks[name].values() for c in v[1:]]


def _settings(on, extra):
    s = {"rounds": dict(extra, FIG_SCHED="rounds"), "seq": {"FIG_SCHED": "seq"}}
    for m in MODES:
        s["wide_" + m] = dict(on, FIG_WIDE=m, **extra)
        s["wide_" + m + "_live0"] = dict(on, FIG_WIDE=m, FIG_CONT_LIVE="0", **extra)       # every chunk continued inside the launch
    s["wide_grow_again"] = s["wide_grow"]
    s["back_0"] = dict(on, FIG_WIDE="0", FIG_CONT_LIVE=HAND_BACK, **extra)                 # every chunk planned by the host
    s["back_grow"] = dict(on, FIG_WIDE="grow", FIG_CONT_LIVE=HAND_BACK, **extra)
    s["back_grow_gated"] = dict(on, FIG_WIDE="grow", FIG_WIDE_MAX_ACTIVE="0", FIG_CONT_LIVE=HAND_BACK, **extra)
    return s


def _upload_env(p):
    # wide slots are packed only where the fill would widen: partial mode has to ask at upload
    return {} if p["case"].mode == "unmapped" else {"FIG_SCHED": "continuous", "FIG_WIDE": "grow"}


# (case, small first chunks) where some gap consumes more than twice the largest first chunk, so that one doubling saves it a
# chunk; asserted as a precondition below.  `three` and the default `forty` / `need` have first chunks of 50-64 for 73-120 candidates.
GROW_SHOWS = {("one", False), ("one", True), ("forty", True), ("need", True)}
# where workgroups are spare while chunks end: 40 gaps x ~13 candidates on 512 workgroups
IDLE_SHOWS = {("forty", True)}


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True], ids=["default_chunks", "small_first_chunks"])
@pytest.mark.parametrize("cid", ["one", "three", "forty", "need"])
def test_every_wide_mode_fills_the_same_on_the_device(cid, small, tmp_path_factory, monkeypatch, capfd):
    """1, 3 and 40 unmapped gaps and `need` (partial, FIG_SCHED=continuous) under FIG_WIDE=0, grow, idle and both against rounds
    and seq; again with FIG_ITEMS_PER_WG=1 FIG_MIN_CHUNK=1, where first chunks are small and growth crosses the 64 base slots;
    grow twice in a row.  Evidence that each path ran, asserted:
      * in-kernel growth: with every chunk continued inside the launch (FIG_CONT_LIVE=0) a grown gap needs fewer chunks, so
        cont_chunks falls strictly (GROW_SHOWS, precondition asserted);
      * the host planner's growth: with no chunk continued in the launch (FIG_CONT_LIVE=100000, cont_chunks == 0) every later chunk
        is the planner's, and the round log shows one wider than any round of FIG_WIDE=0 has (for the one-gap case: 81 > 64);
        with FIG_WIDE_MAX_ACTIVE=0 the rounds are those of FIG_WIDE=0 again;
      * idle-driven widening: cont_chunks falls strictly where workgroups are spare (IDLE_SHOWS);
      * no round of FIG_WIDE=0 or of the rounds form holds a chunk above the 64 base slots, and first chunks are the same everywhere."""
    p = prepared(cid, tmp_path_factory)
    n = len(p["case"].gaps)
    on = {} if p["case"].mode == "unmapped" else {"FIG_SCHED": "continuous"}
    extra = {"FIG_ITEMS_PER_WG": "1", "FIG_MIN_CHUNK": "1"} if small else {}
    R = Run(p, monkeypatch, capfd, _upload_env(p), _settings(on, extra))
    base, sb = R.fills["rounds"]
    for name in R.fills:
        assert_same_fill(base, sb, *R.fills[name], n, f"{cid}: {name} against rounds")
    assert R.slab is not None and int(R.slab.group(2)) == 64 and int(R.slab.group(4)) == 256 and int(R.slab.group(3)) > int(R.slab.group(1))
    consumed = [len(base.cand[g]) for g in range(n)]
    cc = R.cc
    print(cid, "consumed", consumed, "slab", R.slab.groups(), cc)
    assert sb["cont_chunks"] == 0 and R.fills["seq"][1]["cont_chunks"] == 0
    assert max(R.every("wide_0") + R.every("wide_0_live0") + R.every("rounds") + R.every("back_0")) <= 64
    assert all(max(R.every(k)) <= 256 for k in R.chunks if k != "seq")
    firsts = {capg: v[0] for capg, v in R.chunks["wide_0_live0"].items()}
    assert all({capg: v[0] for capg, v in R.chunks[k].items()} == firsts for k in R.chunks if k not in ("seq", "rounds")), R.chunks      # a gap's first chunk is never widened
    first = max(firsts.values())
    assert max(consumed) > first and cc["wide_0_live0"] > 0
    assert cc["wide_idle_live0"] <= cc["wide_0_live0"] and cc["wide_grow_live0"] <= cc["wide_0_live0"]
    assert cc["back_0"] == cc["back_grow"] == cc["back_grow_gated"] == 0 and R.chunks["back_grow_gated"] == R.chunks["back_0"]
    if (cid, small) in GROW_SHOWS:
        assert max(consumed) > 2 * first, (consumed, first)
        assert 0 < cc["wide_grow_live0"] < cc["wide_0_live0"] and 0 < cc["wide_both_live0"] < cc["wide_0_live0"], cc
        assert max(R.later("back_grow")) > max(R.every("back_0")), (R.chunks["back_grow"], R.chunks["back_0"])
        if cid == "one":
            assert max(R.later("back_grow")) > 64
    if (cid, small) in IDLE_SHOWS:
        assert 0 < cc["wide_idle_live0"] < cc["wide_0_live0"], cc
    if cid == "need":
        for name in ("wide_grow", "wide_grow_live0"):
            st = R.fills[name][1]
            assert st["spec_flops"] > st["alg_flops"] == sb["alg_flops"], name


@pytest.mark.gpu
def test_a_widened_chunk_is_narrowed_to_the_live_workgroups(tmp_path_factory, monkeypatch, capfd):
    """fig_cont_publish, the device-only path: `need` under FIG_WIDE=grow.  A first fill gives, per launch class, the first chunk F
    and the launch's workgroups B (more planned items than workgroups: the launch is full while the first gaps' chunks end).  A
    gap that goes on gets 2F candidates; with FIG_CONT_LIVE = 100 B / 1.5 F per cent the launch 'can take' 1.5 F of them -- at
    least F, what the gap would have had without the widening, so the chunk is published with 1.5 F candidates.  The library counts
    these (FIG_SCHED_LOG); the fill is the same."""
    p = prepared("need", tmp_path_factory)
    n = len(p["case"].gaps)
    on = {"FIG_SCHED": "continuous", "FIG_WIDE": "grow"}
    probe = Run(p, monkeypatch, capfd, _upload_env(p), {"rounds": {"FIG_SCHED": "rounds"}, "grow": on})
    consumed = [len(probe.fills["rounds"][0].cand[g]) for g in range(n)]
    capg = min(probe.blocks, key=lambda c: probe.blocks[c])
    F, B = probe.chunks["grow"][capg][0], probe.blocks[capg]
    print("class", capg, "first chunk", F, "workgroups", B, "items", probe.items1[capg], "consumed", consumed)
    assert probe.items1[capg] > B and 2 * F <= 256 and max(consumed) > F and probe.narrowed["grow"] is not None
    live = 100 * B // (3 * F // 2)
    R = Run(p, monkeypatch, capfd, _upload_env(p), {"rounds": {"FIG_SCHED": "rounds"}, "narrow": dict(on, FIG_CONT_LIVE=str(live)), "off": dict(on, FIG_WIDE="0", FIG_CONT_LIVE=str(live))})
    for name in R.fills:
        assert_same_fill(*R.fills["rounds"], *R.fills[name], n, name)
    print("FIG_CONT_LIVE", live, "narrowed", R.narrowed, R.cc)
    assert R.narrowed["narrow"] > 0 and R.cc["narrow"] > 0 and R.narrowed["off"] is None


@pytest.mark.gpu
def test_a_wide_cap_below_the_range_binds(tmp_path_factory, monkeypatch, capfd):
    """`one` (145 candidates) uploaded with FIG_SLOTS_WIDE=80: the gap owns 80 slots, and the chunk after the first 64 -- twice
    that by the rule -- is exactly 80, planned by the host (FIG_CONT_LIVE=100000: 64, 80, 1 in the round log) or continued in the
    launch (FIG_CONT_LIVE=0: 64, 80, 1 -- two continued chunks, as many as FIG_WIDE=0's 64, 64, 17).  The fills are the same."""
    p = prepared("one", tmp_path_factory)
    R = Run(p, monkeypatch, capfd, {"FIG_SLOTS_WIDE": "80"}, _settings({}, {}))
    base, sb = R.fills["rounds"]
    for name in R.fills:
        assert_same_fill(base, sb, *R.fills[name], 1, f"one, 80 slots: {name} against rounds")
    consumed = len(base.cand[0])
    assert R.slab is not None and int(R.slab.group(4)) == 80 and int(R.slab.group(3)) > int(R.slab.group(1))
    assert consumed > 64 + 80
    assert R.every("back_grow") == [64, 80, consumed - 144], R.chunks["back_grow"]
    assert max(c for k in R.chunks for c in R.every(k)) == 80
    assert R.cc["wide_grow_live0"] == 2 and R.cc["wide_0_live0"] == -(-consumed // 64) - 1
