"""Per-base read support (fig_gap_support, include/figbird_hip.h): for every byte of a gap string the five read counts of the
countsGap column it was called from, and per gap the path finalize took (FIG_SUP_*).

The reference of every exact comparison here is a pile-up in Python: the reads draw.txt lists (on the device: the reads the
draw planes report), each at its drawn offset o, base j of the read on column o + j for 0 <= o + j < draw length, bases outside
ACGT on row 4.  The call rule is computeSequence(check=1)'s: the first strict maximum over (A, C, G, T, other); N when that
maximum is 0 or the "other" row holds it."""
import ctypes as C
import os
import re
import socket
import subprocess
import tempfile

import numpy as np
import pytest

import util
from figbird_amd import api

ALL_FILL = util.GOLDEN_CASES + util.BENCH_GOLDENS
GPU_GOLDENS = util.GOLDEN_CASES + ["bench_b25", "bench_b160"]
CODE = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate(b"ACGT"):
    CODE[_c] = _k
INT_MIN = np.iinfo(np.int32).min


# ------------------------------------------------------------------------------------- the Python reference
def pile_up(reads, n):
    """reads: (offset, uint8 ASCII array) pairs -> int32 [n, 5]"""
    cnt = np.zeros((max(n, 0), 5), dtype=np.int32)
    for o, seq in reads:
        x = o + np.arange(len(seq), dtype=np.int64)
        ok = (x >= 0) & (x < n)
        np.add.at(cnt, (x[ok], CODE[seq[ok]]), 1)
    return cnt


def call(cnt):
    """[n, 5] counts -> uint8 ASCII [n]: first strict maximum, N when it is 0 or on row 4"""
    k = np.argmax(cnt, axis=1)                      # the first of equal maxima, as `v > mx` leaves it
    k = np.where(cnt[np.arange(len(cnt)), k] > 0, k, 4)
    return np.frombuffer(b"ACGTN", dtype=np.uint8)[k]


_HDR = re.compile(r"^ *=+\+Gap = (\d+) starting,length = (-?\d+)=+$")
_READ = re.compile(r"^ *([A-Za-z]+)\[(\d+) (-?\d+) isz = -?\d+ [IEP]\]$")


def parse_draw(path):
    """draw.txt -> {gap: (header length, [(offset, read)])}"""
    out, cur = {}, None
    for ln in open(path):
        ln = ln.rstrip("\n")
        m = _HDR.match(ln)
        if m:
            cur = int(m.group(1))
            assert cur not in out, "one header per gap (the two modes never run together)"
            out[cur] = (int(m.group(2)), [])
            continue
        m = _READ.match(ln)
        if m:
            out[cur][1].append((int(m.group(3)), np.frombuffer(m.group(1).encode(), dtype=np.uint8)))
    return out


def _gapout(root):
    return [ln.split("\t") for ln in util.read(os.path.join(root, "ref", "gapout.txt")).splitlines()]


# ------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", ALL_FILL)
def test_reference_pile_up_reproduces_every_called_base(name, tmp_path):
    """Pins the reference the GPU tests use: wherever draw.txt's header length equals the gapout length, every called (non-N)
    base of the reference's gapout.txt is the call of the pile-up of the reads draw.txt lists.  (An N of the reference over a
    supported column is recheck_sequence / findRegion masking and is not a mismatch.)"""
    root = util.extract_golden(name, str(tmp_path))
    draw = parse_draw(os.path.join(root, "ref", "draw.txt"))
    for e in _gapout(root):
        g, n = int(e[0]), int(e[4])
        s = np.frombuffer((e[5] if len(e) > 5 else "").encode(), dtype=np.uint8)
        assert len(s) == max(n, 0)
        if g not in draw or draw[g][0] != n:
            continue
        c = call(pile_up(draw[g][1], n))
        called = s != ord("N")
        assert np.array_equal(s[called], c[called]), f"{name} gap {g}"


def _open_run(root):
    host = api.load_host_library()
    argv = util.meta(root)["fillgaps_argv"]
    err = C.create_string_buffer(512)
    cwd = os.getcwd(); os.chdir(root)
    try:
        h = host.fighost_run_open((C.c_char_p * 15)(*[a.encode() for a in argv]), err, 512)
    finally:
        os.chdir(cwd)
    assert h, err.value.decode()
    return host, h


def test_support_writer_format(tmp_path):
    """fighost_run_write_support on hand-made arrays: `g contig start G0 n origin S D`, S the support of the called base (0
    under an N), D the depth; both empty for n = 0."""
    root = util.extract_golden("partial_small", str(tmp_path))
    exp = _gapout(root)
    assert len(exp) == 3
    host, h = _open_run(root)
    fl = np.array([4, 0, 2], dtype=np.int32)
    off = np.array([0, 4, 4, 6], dtype=np.int64)
    raw = np.frombuffer(b"ACNTGT", dtype=np.uint8).copy()
    sup = np.array([[7, 1, 0, 0, 0], [0, 12, 0, 2, 1], [3, 3, 0, 0, 0], [0, 0, 0, 1, 0],
                    [0, 0, 15, 0, 0], [1, 0, 0, 2, 4]], dtype=np.int32)
    org = np.array([api.SUP_FINAL | api.SUP_TIEBREAK, api.SUP_NONE, api.SUP_ORIGINAL], dtype=np.int32)
    err = C.create_string_buffer(512)
    cwd = os.getcwd(); os.chdir(root)
    try:
        rc = host.fighost_run_write_support(h, api._p(fl, api.c_i32_p), api._p(off, api.c_i64_p), C.cast(raw.ctypes.data, C.c_char_p),
                                            api._p(sup, api.c_i32_p), api._p(org, api.c_i32_p), err, 512)
    finally:
        os.chdir(cwd)
        host.fighost_run_close(h)
    assert rc == 0, err.value.decode()
    head = ["\t".join(e[:4]) for e in exp]
    want = (f"{head[0]}\t4\t5\t7,12,0,1\t8,15,6,1\n"
            f"{head[1]}\t0\t0\t\t\n"
            f"{head[2]}\t2\t2\t15,2\t15,7\n")
    assert util.read(os.path.join(root, "tmp", "gapsupport.txt")) == want


def test_support_abi_surface():
    """The new call and struct are declared and bound; fig_gap_results did not grow (a caller compiled against the previous
    header keeps working); the emulation library, which implements the ABI without the new call, still loads -- and asking
    it for the plane is an error, not a silent nothing."""
    hdr = util.read(os.path.join(util.ROOT, "include", "figbird_hip.h"))
    assert re.search(r"^int fig_fill_resident_ex\(fig_ctx \*ctx, fig_gap_results \*out, const fig_gap_support \*sup\);", hdr, flags=re.M)
    assert "fig_fill_resident_ex" in api.EXPORTS
    assert re.search(r"#define FIG_ABI_VERSION 1\b", hdr)
    src = ('#include <stdio.h>\n#include "figbird_hip.h"\nint main(){printf("%zu %zu %d %d %d %d\\n",sizeof(fig_gap_support),sizeof(fig_gap_results),'
           'FIG_SUP_NONE,FIG_SUP_FINAL,FIG_SUP_ORIGINAL,FIG_SUP_TIEBREAK);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out[0] == C.sizeof(api.FigGapSupport) == 16
    assert out[1] == C.sizeof(api.FigGapResults) == 128            # 128: the size before fig_gap_support existed
    assert out[2:] == [api.SUP_NONE, api.SUP_FINAL, api.SUP_ORIGINAL, api.SUP_TIEBREAK] == [0, 1, 2, 4]
    emu = api.load_library(util.EMULIB)
    assert not hasattr(emu, "fig_fill_resident_ex") and emu.fig_version() == 1
    eng = api.Engine(0, lib_path=util.EMULIB)
    try:
        eng.n_gaps = 0
        with pytest.raises(RuntimeError, match="fig_fill_resident_ex"):
            eng.fill_resident(support=True)
    finally:
        eng.close()


def test_figfill_on_a_library_without_the_call_fails_loudly(tmp_path):
    """FIGFILL_SUPPORT=1 with the emulation behind figfill: an error that names the missing call, and no gapsupport.txt."""
    root = util.extract_golden("partial_small", str(tmp_path))
    r = util.run([util.EMU] + util.meta(root)["fillgaps_argv"], root, {"FIGFILL_SUPPORT": "1"})
    assert r.returncode != 0 and "fig_fill_resident_ex" in r.stderr
    assert not os.path.exists(os.path.join(root, "tmp", "gapsupport.txt"))


# ------------------------------------------------------------------------------------- GPU
class Fill:
    """One fill with its inputs, as plain numpy arrays."""

    def gap_reads(self, g):
        """-> (draw length, [(offset, read)] of the drawn reads) or (None, [])"""
        lu, lp = int(self.draw_len[2 * g]), int(self.draw_len[2 * g + 1])
        assert lu < 0 or lp < 0
        if lu >= 0:
            ks = range(int(self.u_off[g]), int(self.u_off[g + 1]))
            return lu, [(int(self.draw_pos[k]), self.u_seq[self.u_seq_off[k]:self.u_seq_off[k + 1]]) for k in ks if self.draw_pos[k] != INT_MIN]
        if lp >= 0:
            nu = int(self.u_off[-1])
            ks = range(int(self.p_off[g]), int(self.p_off[g + 1]))
            return lp, [(int(self.draw_pos[nu + k]), self.p_seq[self.p_seq_off[k]:self.p_seq_off[k + 1]]) for k in ks if self.draw_pos[nu + k] != INT_MIN]
        return None, []

    def plane(self, g):
        return self.support[int(self.str_off[g]):int(self.str_off[g + 1])]

    def string(self, g):
        return self.raw[int(self.str_off[g]):int(self.str_off[g + 1])]


def _take(F, res, n):
    F.n = n
    F.filled_len = np.array(res.filled_len[:n]); F.gaptofill = np.array(res.gaptofill[:n])
    F.str_off = np.array(res.str_off[:n + 1]); F.raw = np.array(res.raw[:int(res.str_off[n])])
    F.draw_pos, F.draw_isz, F.draw_len = (np.array(a) for a in res.draw)
    F.support = None if res.support is None else np.array(res.support)
    F.origin = None if res.support_origin is None else np.array(res.support_origin)
    return F


def run_golden(root, support=True):
    """The golden `root` through libfighip.so as figfill fills it (run handle, overlap_threshold carry, resident fill), with
    the draw planes and, when asked, the support plane."""
    host, h = _open_run(root)
    try:
        n = int(host.fighost_run_ngaps(h))
        ids = np.arange(max(n, 1), dtype=np.int64)
        cm = api.FigModel(); host.fighost_run_model(h, C.byref(cm))
        cb = api.FigGapBatch(); su = C.c_int64(); sp = C.c_int64()
        assert host.fighost_run_shard(h, api._p(ids, api.c_i64_p), n, C.byref(cb), C.byref(su), C.byref(sp)) == 0
        F = Fill()
        F.G0 = np.ctypeslib.as_array(cb.gap_len, shape=(n,)).copy()
        F.u_off = np.ctypeslib.as_array(cb.u_read_off, shape=(n + 1,)).copy()
        F.p_off = np.ctypeslib.as_array(cb.p_read_off, shape=(n + 1,)).copy()
        F.u_seq_off = np.ctypeslib.as_array(cb.u_seq_off, shape=(int(su.value) + 1,)).copy() if su.value else np.zeros(1, dtype=np.int64)
        F.p_seq_off = np.ctypeslib.as_array(cb.p_seq_off, shape=(int(sp.value) + 1,)).copy() if sp.value else np.zeros(1, dtype=np.int64)
        F.u_seq = np.frombuffer(cb.u_seq or b"", dtype=np.uint8)           # (ASCII bases: no NUL inside)
        F.p_seq = np.frombuffer(cb.p_seq or b"", dtype=np.uint8)
        assert len(F.u_seq) == int(F.u_seq_off[-1]) and len(F.p_seq) == int(F.p_seq_off[-1])
        F.unmapped = bool(cm.unmapped_flag)
        eng = api.Engine(0)
        try:
            eng.set_model_struct(cm)
            eng.upload_struct(cb)
            reach = np.zeros(max(n, 1), dtype=np.uint8); reach[:n] = eng.probe_reach()
            preset = np.zeros(max(n, 1), dtype=np.uint8)
            host.fighost_run_ot_presets(h, api._p(reach, api.c_u8_p), api._p(preset, api.c_u8_p))
            eng.set_ot_preset(preset[:n])
            res = eng.fill_struct(cb, int(su.value), int(sp.value), draw=True, resident=True, support=support)
        finally:
            eng.close()
        assert "libfighip.so" in open("/proc/self/maps").read()
        return _take(F, res, n)
    finally:
        host.fighost_run_close(h)


@pytest.fixture(scope="module")
def fills(tmp_path_factory):
    """name -> Fill of that golden with the support and draw planes on; computed once per module, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_golden(util.extract_golden(name, str(tmp_path_factory.mktemp(name))))
        return cache[name]
    return get


def check_call_rule(F):
    assert F.support.shape == (int(F.str_off[F.n]), 5) and F.support.dtype == np.int32 and (F.support >= 0).all()
    for g in range(F.n):
        s, p = F.string(g), F.plane(g)
        assert len(s) == max(int(F.filled_len[g]), 0)
        c = call(p)
        called = s != ord("N")
        assert np.array_equal(s[called], c[called]), f"gap {g}: a called base is not the call of its column"
        assert (p[np.arange(len(s)), CODE[s]][called] >= 1).all(), f"gap {g}: a called base without support"
        assert (F.origin[g] == api.SUP_NONE) == (not p.any()), f"gap {g}: origin {F.origin[g]} against its plane"
        assert 0 <= F.origin[g] <= 7 and (F.origin[g] & 3) != 3


def check_evidence(F, g):
    """Gap g against the pile-up of its drawn reads, where the plane is defined as that pile-up: origin FINAL and as many
    columns as the draw header says.  -> "final" (compared exactly), "tiebreak" (compared column by column), None (not such a gap)"""
    org = int(F.origin[g])
    n, reads = F.gap_reads(g)
    if not (org & api.SUP_FINAL) or org & api.SUP_ORIGINAL or n is None or n != int(F.filled_len[g]):
        return None
    ref, p = pile_up(reads, n), F.plane(g)
    if not org & api.SUP_TIEBREAK:
        assert np.array_equal(p, ref), f"gap {g}: plane differs from the pile-up of {len(reads)} drawn reads"
        return "final"
    d = p[:, :4] - ref[:, :4]
    same = (d == 0).all(axis=1)
    plus10 = ((d == 10).sum(axis=1) == 1) & ((d != 0).sum(axis=1) == 1)
    zeroed = (p[:, :4] == 0).all(axis=1)
    assert np.array_equal(p[:, 4], ref[:, 4]), f"gap {g}: the tie-break never touches row 4"
    bad = ~(same | plus10 | zeroed)
    assert not bad.any(), f"gap {g}: columns {np.flatnonzero(bad)[:8]} are neither the pile-up, nor it +10 on one base, nor zeroed"
    return "tiebreak"


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_GOLDENS)
def test_call_rule_and_exact_evidence(name, fills, tmp_path):
    """Every gap of the golden: the emitted string is its plane's call or N, a called base has support, origin NONE means an
    all-zero plane and nothing else does; and where the plane is defined as the pile-up of the drawn reads it equals it --
    exactly, or (partial-mode tie-break) column by column up to +10 on one base or zeroed A..T.  The strings are the
    reference's, so the plane is evidence for the bytes figfill writes."""
    F = fills(name)
    root = util.extract_golden(name, str(tmp_path))
    exp = _gapout(root)
    assert [int(e[4]) for e in exp] == list(F.filled_len)
    assert [e[5] if len(e) > 5 else "" for e in exp] == [F.string(g).tobytes().decode() for g in range(F.n)]
    check_call_rule(F)
    for g in range(F.n):
        check_evidence(F, g)


@pytest.mark.gpu
def test_expected_origins(fills):
    """Origins that follow from the code and the goldens; they keep the comparisons above from being vacuous."""
    F = fills("bench_b160")
    n, reads = F.gap_reads(0)
    assert F.unmapped and int(F.origin[0]) == api.SUP_FINAL and n == int(F.filled_len[0]) == 305 != int(F.G0[0]) == 160 and len(reads) == 657
    assert check_evidence(F, 0) == "final"                                  # an unmapped-mode gap compared exactly
    assert int(fills("partial_brackets").origin[1]) & api.SUP_FINAL
    for name, gaps in [("cap_3001", [0]), ("edge_no_reads", [0]), ("neg_overlap", [1]), ("ot_carry", [0]), ("repeat_flanks", [0, 2])]:
        F = fills(name)
        for g in gaps:
            assert F.gap_reads(g)[0] is None and int(F.origin[g]) == api.SUP_NONE and not F.plane(g).any(), (name, g)
    for name in GPU_GOLDENS:                                                # no draw header, no evidence
        F = fills(name)
        for g in range(F.n):
            if F.gap_reads(g)[0] is None:
                assert int(F.origin[g]) == api.SUP_NONE, (name, g)
    for name, gaps in [("threads3", [1, 2, 3]), ("partial_L150", [1]), ("partial_L199", [0])]:
        F = fills(name)
        for g in gaps:
            assert F.gap_reads(g)[0] != int(F.filled_len[g]) and not int(F.origin[g]) & api.SUP_FINAL, (name, g)
    tags = [check_evidence(fills(name), g) for name in GPU_GOLDENS if not fills(name).unmapped for g in range(fills(name).n)]
    assert "tiebreak" in tags                                               # a partial-mode gap compared column by column


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unmapped_small", "partial_brackets"])
def test_off_means_off(name, fills, tmp_path):
    """Asking for the plane changes nothing else: lengths, gaptofill, strings and the draw planes are those of a fill without it."""
    on = fills(name)
    off = run_golden(util.extract_golden(name, str(tmp_path)), support=False)
    assert off.support is None and off.origin is None
    for f in ("filled_len", "gaptofill", "str_off", "raw", "draw_pos", "draw_isz", "draw_len"):
        assert np.array_equal(getattr(on, f), getattr(off, f)), f


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["threads3", "unmapped_small"])
def test_scheduler_modes_give_the_same_plane(name, tmp_path, monkeypatch):
    """fig_gap_end runs in fig_begin_kernel / fig_end_kernel under the candidate-parallel scheduler and in fig_fill_kernel under
    FIG_SCHED=seq: the same plane and origins, bit for bit."""
    monkeypatch.delenv("FIG_SCHED", raising=False)
    par = run_golden(util.extract_golden(name, str(tmp_path / "par")))
    monkeypatch.setenv("FIG_SCHED", "seq")
    seq = run_golden(util.extract_golden(name, str(tmp_path / "seq")))
    assert par.origin.any()
    assert np.array_equal(par.raw, seq.raw) and np.array_equal(par.str_off, seq.str_off)
    assert np.array_equal(par.support, seq.support) and np.array_equal(par.origin, seq.origin)


@pytest.mark.gpu
def test_both_engine_instantiations():
    """Gaps of 1599 and 1601 bp, either side of the boundary between the LDS-table and the global-table instantiation of the
    engine (fig_pack.h class table), made as tests/test_gpu_parity.py makes them: call rule and exact evidence on both."""
    from figbird_amd import synth
    from test_gpu_parity import _bench_engine
    spec = synth.BenchSpec(mode="unmapped", reads_per_gap_mean=500.0)
    eng, _ = _bench_engine(spec)
    batch, _ = synth.make_bench_batch(2027, 2, spec, gap_lengths=np.array([1599, 1601]))
    try:
        res = eng.fill(batch, support=True, draw=True)
    finally:
        eng.close()
    F = Fill()
    F.G0 = np.asarray(batch.gap_len); F.unmapped = True
    F.u_off, F.p_off = np.asarray(batch.u_read_off), np.asarray(batch.p_read_off)
    F.u_seq_off, F.p_seq_off, F.u_seq, F.p_seq = batch.u_seq_off, batch.p_seq_off, batch.u_seq, batch.p_seq
    _take(F, res, batch.n_gaps)
    assert list(F.G0) == [1599, 1601]
    check_call_rule(F)
    print("origins", list(F.origin), "filled", list(F.filled_len), "draw", [F.gap_reads(g)[0] for g in range(2)])
    for g in range(2):                      # the batch is seeded: both gaps end FINAL at their drawn length, so both are compared
        assert int(F.origin[g]) == api.SUP_FINAL and F.gap_reads(g)[0] == int(F.filled_len[g]), f"gap {g}: nothing to compare"
        assert check_evidence(F, g) == "final"


@pytest.mark.gpu
def test_gapsupport_file_is_the_same_from_every_host_path(tmp_path, monkeypatch):
    """threads3 with FIGFILL_SUPPORT=1: figfill on one GPU, figfill with FIGFILL_DEVICES=0,0 (two shards merged by the C++ host)
    and two-rank figfill_mp (shards gathered, rank 0 writes) leave the same gapsupport.txt, and in each run the reference's
    files stay byte-identical; without the variable no such file appears."""
    import torch.multiprocessing as mp
    from test_multi_rank import _mp_worker
    roots = [util.extract_golden("threads3", str(tmp_path / f"r{k}")) for k in range(4)]
    argv = util.meta(roots[0])["fillgaps_argv"]
    r = util.run([util.FIGFILL] + argv, roots[3])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(os.path.join(roots[3], "tmp", "gapsupport.txt"))
    r = util.run([util.FIGFILL] + argv, roots[0], {"FIGFILL_SUPPORT": "1"})
    assert r.returncode == 0, r.stderr
    r = util.run([util.FIGFILL] + argv, roots[1], {"FIGFILL_SUPPORT": "1", "FIGFILL_DEVICES": "0,0"})
    assert r.returncode == 0, r.stderr
    monkeypatch.setenv("FIGFILL_SUPPORT", "1")                              # the spawned ranks inherit it
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_mp_worker, args=(k, 2, port, roots[2], "threads3", q, None)) for k in range(2)]
    for p in ps:
        p.start()
    outs = [q.get(timeout=600) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(rc == 0 for _, rc in outs)
    files = [util.read(os.path.join(root, "tmp", "gapsupport.txt")) for root in roots[:3]]
    assert files[0] == files[1] == files[2]
    lines = files[0].splitlines()
    exp = _gapout(roots[0])
    assert len(lines) == len(exp) == 8
    for ln, e in zip(lines, exp):
        f = ln.split("\t")
        assert len(f) == 8 and f[:5] == e[:5]
        n = int(f[4])
        assert all(len(x.split(",")) == n if n else x == "" for x in f[6:8])
    assert any(int(ln.split("\t")[5]) != 0 for ln in lines)
    for root in roots:
        for fn in util.ref_files(root):
            assert util.read(os.path.join(root, "tmp", fn)) == util.read(os.path.join(root, "ref", fn)), (root, fn)
