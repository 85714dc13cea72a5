"""The C-ABI shared library and the host-side mirror (no GPU compute)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import util
from figbird_amd import api, build as fbuild, synth


def _declared_functions():
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    names = re.findall(r"^\s*(?:int|void|int64_t|const char \*)\s*\*?\s*(fig_[a-z_]+)\s*\(", hdr, flags=re.M)
    return sorted(set(names))


def test_header_declares_the_documented_surface():
    assert _declared_functions() == sorted(api.EXPORTS)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(fbuild.LIB), "libfighip.so must be built in-tree (python -m figbird_amd.build)"
    lib = ctypes.CDLL(fbuild.LIB)
    for fn in _declared_functions():
        assert hasattr(lib, fn), fn
    assert lib.fig_version() == 1


def test_no_gpu_means_a_loud_failure_not_a_fallback():
    """Without a HIP device fig_ctx_create must fail (FIG_ENODEV); with one it must succeed.  Never silent CPU."""
    lib = api.load_library()
    ctx = ctypes.c_void_p()
    rc = lib.fig_ctx_create(0, ctypes.byref(ctx))
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    if have:
        assert rc == 0
        lib.fig_ctx_destroy(ctx)
    else:
        assert rc == -2 and not ctx.value
        with pytest.raises(RuntimeError):
            api.Engine(0)


def test_struct_layouts_match_the_header():
    # sizes as the C compiler lays them out (x86-64 SysV): checked against a tiny C program
    import subprocess, tempfile
    src = '#include <stdio.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(fig_model),sizeof(fig_gap_batch),sizeof(fig_gap_results),sizeof(fig_stats));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert [int(x) for x in out] == [ctypes.sizeof(api.FigModel), ctypes.sizeof(api.FigGapBatch), ctypes.sizeof(api.FigGapResults), ctypes.sizeof(api.FigStats)]


def test_host_model_equals_oracle_model(tmp_path):
    """A0 built by the shipped host code (libfighost.so) vs the oracle's MODEL trace line."""
    root = util.extract_golden("unmapped_mid_err", str(tmp_path))
    tr = str(tmp_path / "t.trace")
    assert util.run_oracle_fillgaps(root, trace=tr).returncode == 0
    _, om = util.parse_trace(tr)
    m = api.model_from_files(os.path.join(root, "scf.fa"), os.path.join(root, "tmp") + "/", os.path.join(root, "tmp", "myout.sam"),
                             partial_flag=0, unmapped_flag=1, script_itr=1, max_distance=690, read_length=50, neg_overlap=30, partial_len=50)
    assert (m.cutoff, m.Tmin, m.Tmax) == om[:3]
    assert m.stats == om[3:]
    assert len(m.e) == 50 and np.all(m.e > 0) and np.all(m.e < 1)
    assert abs(m.T.reshape(5, 5).sum(axis=1) - 1).max() < 1e-12


def test_set_inputmean_changes_the_model_as_in_the_reference(tmp_path):
    """set_inputmean = 1 (Figbird.cpp:6971-6973, used at :913): pairs on a contig no longer than the insert size stay out of the
    insert-size histogram.  The `inputmean` fixture (reference outputs made with the flag on) has such a contig: the host
    model equals the oracle's with the flag on, and differs from the model built with the flag off."""
    root = util.extract_golden("inputmean", str(tmp_path))
    a = util.meta(root)["fillgaps_argv"]
    assert a[13] == "1"
    tr = str(tmp_path / "t.trace")
    assert util.run_oracle_fillgaps(root, trace=tr).returncode == 0
    _, om = util.parse_trace(tr)
    kw = dict(partial_flag=0, unmapped_flag=1, script_itr=1, max_distance=int(a[1]), read_length=int(a[2]), neg_overlap=int(a[10]), partial_len=int(a[11]))
    on = api.model_from_files(os.path.join(root, "scf.fa"), os.path.join(root, "tmp") + "/", os.path.join(root, "tmp", "myout.sam"), setinputmean=1, isz=int(a[14]), **kw)
    off = api.model_from_files(os.path.join(root, "scf.fa"), os.path.join(root, "tmp") + "/", os.path.join(root, "tmp", "myout.sam"), setinputmean=0, isz=int(a[14]), **kw)
    assert (on.cutoff, on.Tmin, on.Tmax) == om[:3] and on.stats == om[3:]
    assert on.stats != off.stats and (on.Tmin, on.Tmax) != (off.Tmin, off.Tmax)


def test_case_to_batch_applies_parse_unmapped_orientation():
    c = synth.make_case("t", 5, "unmapped", [(3000, 30)], coverage=6, n_model_pairs=50)
    b = synth.case_to_batch(c)
    g = c.gaps[0]
    assert b.n_gaps == 1 and int(b.u_read_off[1]) == len(g.unmapped)
    for k, r in enumerate(g.unmapped):
        s = b.u_seq[b.u_seq_off[k]:b.u_seq_off[k + 1]].tobytes().decode()
        if r.anchor_reverse:
            assert s == r.mate_seq_fastq and b.u_is_reverse[k] == 0
        else:
            assert s == synth.revcomp(r.mate_seq_fastq) and b.u_is_reverse[k] == 1


def test_emulation_library_through_the_python_api(tmp_path):
    """api.Engine drives the same ctypes structs whichever library sits behind the ABI."""
    name = "partial_small"
    root = util.extract_golden(name, str(tmp_path))
    m = util.meta(root)
    a = m["fillgaps_argv"]
    model = api.model_from_files(os.path.join(root, "scf.fa"), os.path.join(root, "tmp") + "/", os.path.join(root, "tmp", "myout.sam"),
                                 partial_flag=int(a[4]), unmapped_flag=int(a[5]), script_itr=int(a[3]), max_distance=int(a[1]),
                                 read_length=int(a[2]), neg_overlap=int(a[10]), partial_len=int(a[11]))
    case = synth.make_case(name, 2, "partial", [(3000, 30), (6000, 120), (9000, 10)], insert_mean=180, insert_sd=10, coverage=30, n_model_pairs=800)
    eng = api.Engine(0, lib_path=util.EMULIB)
    eng.set_model(model)
    res = eng.fill(synth.case_to_batch(case))
    eng.close()
    exp = [ln.split("\t") for ln in util.read(os.path.join(root, "ref", "gapout.txt")).splitlines()]
    assert [int(e[4]) for e in exp] == list(res.filled_len)
    assert [e[5] if len(e) > 5 else "" for e in exp] == res.strings


def test_model_build_threads_agree(tmp_path, monkeypatch):
    """N2: the two passes over myout.sam split over host threads (mmap, ranges cut on pair / qname-group boundaries) give
    exactly the single-thread model: every accumulated quantity is an integer histogram."""
    import time
    c = synth.make_case("mt", 77, "unmapped", [(3000, 30)], coverage=2, n_model_pairs=9000, err=0.01, model_indel_rate=0.08, contig_len=14000)
    # multi-alignment groups: a few pairs repeated back to back under the same qnames (what `bowtie2 -k` writes)
    out = []
    for k in range(0, len(c.myout), 2):
        out += c.myout[k:k + 2]
        if (k // 2) % 97 == 0:
            out += c.myout[k:k + 2] * (1 + (k // 2) % 3)
    c.myout = out
    p = synth.write_case(c, str(tmp_path))
    models, times = [], []
    for th in ("1", "2", "5", "16"):
        monkeypatch.setenv("FIGFILL_THREADS", th)
        t0 = time.time()
        m = api.model_from_files(p["scf"], p["tmp"], p["myout"], partial_flag=0, unmapped_flag=1, script_itr=1, max_distance=c.max_distance,
                                 read_length=c.read_len, neg_overlap=30, partial_len=c.partial_len)
        times.append(time.time() - t0)
        models.append(m)
    a = models[0]
    for b in models[1:]:
        assert (a.Tmin, a.Tmax, a.cutoff, a.stats) == (b.Tmin, b.Tmax, b.cutoff, b.stats)
        for x, y in ((a.e, b.e), (a.ins, b.ins), (a.dele, b.dele), (a.T, b.T), (a.insd, b.insd)):
            assert np.array_equal(x, y)
    assert a.ins.max() > a.ins.min()            # the indel reads really fed inPosDist


@pytest.mark.parametrize("lens,threads", [([20, 500, 25, 600, 18, 33, 700], 5), ([500, 20, 600, 700, 30, 800, 900, 450, 25, 1000, 40, 1100], 3)])
def test_gap_deal_matches_live_reference(lens, threads, tmp_path):
    """FillGaps.cpp:456-649 deals the gaps to $num_threads worker processes (short gaps in turn, long ones by remaining
    capacity); `figfill` reproduces it (fig_host.cpp: thread_allocation) for gaploads.txt, the order of draw.txt and the
    process-level overlap_threshold, and so does the oracle.  Read-less gaps keep this quick.  The reference's FillGaps.out
    output on these cases is recorded in tests/golden/gap_deal.json (tools/make_deal_golden.py).  (The committed `threads3`
    fixture pins the short-gap branch with reads.)"""
    from figbird_amd import synth
    from tools.make_deal_golden import FILES, deal_case
    with open(os.path.join(util.GOLDEN, "gap_deal.json")) as f:
        ref = next(g for g in json.load(f).values() if g["lens"] == lens and g["threads"] == threads)["files"]
    case = deal_case(lens)
    for tag, exe in (("host", [util.EMU]), ("oracle", [util.ORACLE, "fillgaps"])):
        p = synth.write_case(case, str(tmp_path / tag))
        cwd = tmp_path / ("cwd_" + tag); cwd.mkdir()
        r = util.run(exe + synth.fillgaps_argv(case, p, n_threads=threads), str(cwd), timeout=600)
        assert r.returncode == 0, r.stderr
        assert {fn: util.read(p["tmp"] + fn) for fn in FILES} == ref, tag


def _run_handle(root):
    import ctypes as C
    from figbird_amd import api
    h = api.load_host_library()
    argv = util.meta(root)["fillgaps_argv"]
    hh = h.fighost_run_open((C.c_char_p * 15)(*[a.encode() for a in argv]), C.create_string_buffer(256), 256)
    assert hh
    return h, hh


def _reach_and_presets(root, lib_path):
    """(reach bits measured by the library, presets carried along the reference's worker processes) of a golden's run."""
    import ctypes as C
    from figbird_amd import api
    cwd = os.getcwd(); os.chdir(root)
    try:
        h, hh = _run_handle(root)
        n = int(h.fighost_run_ngaps(hh))
        ids = np.arange(n, dtype=np.int64)
        cm = api.FigModel(); h.fighost_run_model(hh, C.byref(cm))
        cb = api.FigGapBatch(); su = C.c_int64(); sp = C.c_int64()
        assert h.fighost_run_shard(hh, api._p(ids, api.c_i64_p), n, C.byref(cb), C.byref(su), C.byref(sp)) == 0
        eng = api.Engine(0, lib_path=lib_path)
        eng.set_model_struct(cm)
        eng.upload_struct(cb)
        reach = eng.probe_reach().copy()
        eng.free_batch(); eng.close()
        preset = np.zeros(n, dtype=np.uint8)
        h.fighost_run_ot_presets(hh, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
        h.fighost_run_close(hh)
    finally:
        os.chdir(cwd)
    return reach.tolist(), preset.tolist()


OT_EXPECT = {   # golden -> (reach, presets): tools/make_golden.py explains the two fixtures
    # gap 0 closes by a negative overlap at its first candidate, gap 1 sits 8 bp from the contig end: neither gets to :6317,
    # so gap 1 still sees overlap_threshold = 0 (a carry predicted from contig geometry alone handed it 5)
    "ot_carry": ([0, 0], [0, 0]),
    # $num_threads = 3: processes {0, 3}, {1}, {2}: gap 3 follows gap 0 in ITS process, although gaps 1 and 2 got there
    "ot_carry_t3": ([0, 1, 1, 0], [0, 0, 0, 0]),
    "threads3": ([1] * 8, [0, 0, 0, 1, 1, 1, 1, 1]),
    "neg_overlap": ([1, 0], [0, 1]),
}


@pytest.mark.parametrize("name", sorted(OT_EXPECT))
def test_overlap_threshold_carry_is_measured(name, tmp_path):
    """Figbird.cpp:103, :6298-6317: the library measures which gaps get to `overlap_threshold=5` (fig_batch_probe_reach; here the
    one-lane emulation of the same device code), the host carries the bits along the reference's worker processes."""
    root = util.extract_golden(name, str(tmp_path))
    assert _reach_and_presets(root, util.EMULIB) == OT_EXPECT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(OT_EXPECT))
def test_overlap_threshold_carry_is_measured_on_the_device(name, tmp_path):
    """The same through libfighip.so: fig_probe_kernel on the MI355X."""
    root = util.extract_golden(name, str(tmp_path))
    assert _reach_and_presets(root, None) == OT_EXPECT[name]
    assert "libfighip.so" in open("/proc/self/maps").read()


def test_library_measures_the_carry_itself_without_a_preset(tmp_path):
    """gap_ot_preset = NULL: one worker process in batch order, carry measured by the library at upload -- same strings as with
    the explicit carry, and (on `ot_carry`) the preset differs from what contig geometry alone would have predicted."""
    from tools import make_golden
    case = make_golden.make("ot_carry")
    root = util.extract_golden("ot_carry", str(tmp_path))
    cwd = os.getcwd(); os.chdir(root)
    try:
        model = api.model_from_files("scf.fa", "tmp/", "tmp/myout.sam", partial_flag=1, unmapped_flag=0, script_itr=1, max_distance=case.max_distance,
                                     read_length=case.read_len, neg_overlap=case.neg_overlap, partial_len=case.partial_len)
    finally:
        os.chdir(cwd)
    exp = [ln.split("\t") for ln in util.read(os.path.join(root, "ref", "gapout.txt")).splitlines()]
    outs = []
    for preset in (None, np.zeros(2, dtype=np.uint8)):
        b = synth.case_to_batch(case); b.gap_ot_preset = preset
        eng = api.Engine(0, lib_path=util.EMULIB); eng.set_model(model)
        res = eng.fill(b); eng.close()
        outs.append((res.filled_len.tolist(), res.gaptofill.tolist(), res.strings))
    assert outs[0] == outs[1]
    assert outs[0][0] == [int(e[4]) for e in exp] and outs[0][2] == [e[5] if len(e) > 5 else "" for e in exp]


def _plan_round(lib, ids, ctl, capacity, nsplit, slots_cap, minc, ipw, n_active_max):
    ids_a = np.asarray(ids, dtype=np.int32); ctl_a = np.asarray(ctl, dtype=np.int32).reshape(-1)
    cap_ints = 4 * (len(ids) * (slots_cap + 1) + 1)
    items = np.zeros(cap_ints, dtype=np.int32); entries = np.zeros(cap_ints, dtype=np.int32)
    nam, n_items, n_ent, chunk = (ctypes.c_int(v) for v in (n_active_max, 0, 0, 0))
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.fig_emu_plan_round.restype = ctypes.c_int
    lib.fig_emu_plan_round.argtypes = [i32p, ctypes.c_int, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                       ctypes.POINTER(ctypes.c_int), i32p, ctypes.POINTER(ctypes.c_int), i32p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    n_active = lib.fig_emu_plan_round(ids_a.ctypes.data_as(i32p), len(ids), ctl_a.ctypes.data_as(i32p), capacity, nsplit, slots_cap, minc, ipw, ctypes.byref(nam),
                                      items.ctypes.data_as(i32p), ctypes.byref(n_items), entries.ctypes.data_as(i32p), ctypes.byref(n_ent), cap_ints, ctypes.byref(chunk))
    assert n_active >= 0
    return n_active, nam.value, items[:4 * n_items.value].reshape(-1, 4).tolist(), entries[:4 * n_ent.value].reshape(-1, 4).tolist(), chunk.value


def _check_round(lib, ids, ctl, capacity, nsplit, slots_cap, minc, ipw, n_active_max):
    """One planned round against what the scheduler promises; every expected value comes from the inputs."""
    n_active, nam, items, entries, chunk = _plan_round(lib, ids, ctl, capacity, nsplit, slots_cap, minc, ipw, n_active_max)
    active = [g for g in ids if ctl[g][0] == 1]                               # in cost order
    assert n_active == len(active)
    assert nam == max(n_active_max, len(active))                              # only grows
    if not active:
        assert items == [] and entries == []
        return entries
    target = ipw * min(8.0, max(1.0, nam / 96.0)) * capacity / max(1, nsplit)
    assert [e[0] for e in entries] == active[:len(entries)] and len(entries) >= 1      # a prefix of the cost order
    total, pos = 0, 0
    for g, n, _, _ in entries:
        assert total < 1.25 * target                                          # admitted while the round was not full
        j, rng = ctl[g][1], ctl[g][2]
        assert min(minc, slots_cap, rng - j) <= n <= min(slots_cap, rng - j)
        if rng == j:
            assert n == 0                                                     # replayed with nothing to evaluate
        assert items[pos:pos + n] == [[g, j + k, k, 0] for k in range(n - 1, -1, -1)]      # contiguous, slots descending to 0
        total += n; pos += n
    assert pos == len(items)                                                  # no item without an entry
    if len(entries) < len(active):
        assert total >= 1.25 * target                                         # the rest waits only because the round is full
    assert chunk == max(e[1] for e in entries)
    return entries


def test_round_planner_of_the_candidate_parallel_scheduler():
    """fig_plan_round (fig_abi_host.h) is what libfighip's class lanes and the emulation both run; here it is driven on
    hand-made gapctl snapshots through the emulation library's test-only shim."""
    lib = ctypes.CDLL(util.EMULIB)
    # gapctl rows {status, next j, range, -}: finished, active, loop done, active with nothing left, active near its end
    ctl = [[0, 0, 0, 0], [1, 0, 40, 0], [2, 7, 7, 0], [1, 9, 9, 0], [1, 30, 33, 0], [1, 2, 200, 0]]
    ent = _check_round(lib, [5, 1, 4, 3, 2, 0], ctl, capacity=4, nsplit=1, slots_cap=32, minc=16, ipw=12.0, n_active_max=0)
    assert [e[:2] for e in ent] == [[5, 32], [1, 16], [4, 3], [3, 0]]          # share 48/241: every want below minc except the first
    # nothing active: no round, and the lane's largest active set is kept
    assert _plan_round(lib, [2, 0], ctl, 4, 1, 32, 16, 12.0, 5)[:2] == (0, 5)
    # admission cut-off: 300 active gaps on two lanes of 8 workgroups; the round is full long before the last gap
    big = [[1, g % 7, 40 + g % 5, 0] for g in range(300)]
    ent = _check_round(lib, list(range(299, -1, -1)), big, capacity=8, nsplit=2, slots_cap=32, minc=16, ipw=12.0, n_active_max=0)
    assert 1 < len(ent) < 300
    # a chunk above the slot cap is clamped to it (the emulation's FIG_EMU_CHUNK form: exactly min(n, nslots, range - j))
    ent = _check_round(lib, [1, 4, 5], ctl, capacity=1000, nsplit=1, slots_cap=3, minc=3, ipw=12.0, n_active_max=0)
    assert [e[1] for e in ent] == [3, 3, 3]
    ent = _check_round(lib, [1, 4, 5], ctl, capacity=1000, nsplit=1, slots_cap=32, minc=64, ipw=12.0, n_active_max=0)
    assert [e[1] for e in ent] == [32, 3, 32]
    # random snapshots, the lane's history carried from round to round
    rng = np.random.default_rng(5)
    nam = 0
    for _ in range(50):
        n = int(rng.integers(1, 400))
        snap = [[int(rng.integers(0, 3)), 0, 0, 0] for _ in range(n)]
        for row in snap:
            row[2] = int(rng.integers(1, 120)); row[1] = int(rng.integers(0, row[2] + 1))
        ids = [int(g) for g in rng.permutation(n)[:int(rng.integers(1, n + 1))]]
        args = dict(capacity=int(rng.integers(1, 64)), nsplit=int(rng.integers(1, 3)), slots_cap=int(rng.integers(1, 65)), minc=int(rng.integers(1, 40)), ipw=float(rng.choice([6.0, 12.0])))
        _check_round(lib, ids, snap, n_active_max=nam, **args)
        nam = max(nam, sum(1 for g in ids if snap[g][0] == 1))
