#!/usr/bin/env python3
"""Directed cases for partial mode's fallback forms and its overlap detector, next to tools/estep_cases.py.

In a partial-mode run placeReads has two forms: the fast one (fig_partial_estep / fig_partial_mle, fig_engine_partial.h) and
the generic loops of fig_engine_core.h; fig_partial_fast picks between them per call.  After the MLE pass
fig_detect_overlap_par replaces lane 0's serial walk (fig_detect_overlap) unless the reads do not fit its staging area.  The
cases here reach every refusal of the fast form and every fallback of the detector:

  pn                 N in the clipped reads of gaps 0 and 2 (FigDevGap::pad bit 0), a clean gap beside them in the same class
  pstart_{10,48,49}  a gap 10 / L - 2 / L - 1 bases from the contig start (S.left < xoff = L - 1), L = 50
  p192               192 and 193 clipped reads: the parallel detector's last size and the serial detector's first
  pmany              240 reads per gap: serial detector; 15 super-chunks of FIG_PT_ROWS in the fast E-step
  pwide              1250 bp (the 1217-1600-column class), 1700 and 1800 bp (the last class, LDS-tiled at this length)
  pwide_n            pwide with N in the clipped reads: both refusals at once

pwide's 1800-bp gap: at L = 101 a class whose longest gap is 1700 bp still fits its table into LDS untiled (the class table
below: up to 1736 columns), so the 1700-bp gap alone would not reach the tiled form; a class's geometry follows its longest
gap, and beside an 1800-bp gap both run tiled.

The predicates of fig_partial_fast and of the detector's fallback, and the launch-class table of fig_pack.h they depend on,
are restated here in integers, so that a test can say which form a gap takes without running it (tests/test_partial_forms.py;
the GPU test compares the restated classes with the library's own `[figsched] class:` lines).

The oracle's trace levels 5..8 add one DET line per partial-mode placeReads call: what detect_overlap_gapestimate returned.
`det_branches` names the branches seen, `tie_margin` is the guard against likelihood ties: a fixture is only usable for a
1e-6 comparison of a device with glibc if no decision of the candidate loop sits within that distance of flipping.

  python3 tools/partial_cases.py            # per case and gap: class, form, detector form; branches reached; tie margin
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from figbird_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle", "figbird_oracle")

# ---- constants of the device code ----------------------------------------------------------------------------------------------
CLASS_DEFS = ((448, 256), (1216, 512), (1600, 512), (1 << 30, 512))     # fig_pack.h, ClsDef defs[]: longest candidate (columns), threads
LDS_MAX = 160 * 1024 - 1024          # fig_pack.h
FIG_MAX_READLEN = 200                # fig_types.h
FIG_PLB_BYTES = 8 * 64 * 4           # fig_engine.h
STATE_BYTES = 4152                   # sizeof(FigState); the library prints it on its `[figsched] class:` lines
FIG_PT_ROWS = 16                     # fig_engine_partial.h: reads per super-chunk of the fast E-step
DET_PAR_MAX_READS = 192              # fig_detect_overlap_par: prc > 192 -> serial
TIE_TOL = 1e-6                       # the parity contract's relative tolerance on a likelihood


# ---- the integer arithmetic of the host packer and the device predicates, restated ---------------------------------------------
def gmax_partial(G0, partial_len):
    """Longest candidate (columns) of a partial-mode gap: gap_alloc / gmax of fig_gaprules.h and fig_pack.h:200-206 (float32)."""
    factor = 3 * partial_len
    if G0 <= (2 * partial_len) // 2:
        f2, alloc = np.float32(factor) / np.float32(G0), factor * 3
    elif G0 <= 2 * partial_len:
        f2, alloc = np.float32(5.0), G0 * 5
    else:
        f2, alloc = np.float32(1.0), G0 * 3
    alloc = max(alloc, G0)
    return min(max(G0, int(np.float32(G0) * f2)), alloc)


def class_table(gmaxes, L, state_bytes=STATE_BYTES):
    """fig_pack.h:218-284 for a batch whose gaps reach `gmaxes` columns at read length L -> ([class dict], class index per gap).
    A class dict holds what the library logs: capGl, ncolE, Wcap, nt, nteams, lds_tab, tiles."""
    classes, cls_of, prev = [], [None] * len(gmaxes), 0
    for cap, nt in CLASS_DEFS:
        ids = [g for g, gm in enumerate(gmaxes) if prev < gm <= cap]
        prev = cap
        if not ids:
            continue
        capGl = (max([8] + [gmaxes[g] for g in ids]) + 7) & ~7
        ncolE = (capGl + 2 * (L - 1) + 7) & ~7
        Wcap = (capGl + L + 7) & ~7
        fixed = state_bytes + capGl + FIG_MAX_READLEN + 64 + FIG_PLB_BYTES
        c = dict(capGl=capGl, ncolE=ncolE, Wcap=Wcap, nt=nt, nteams=nt // 64, lds_tab=0, tiles=0)
        t = nt // 64
        while t >= 1:
            if fixed + 8 * (9 * ncolE + t * Wcap) <= LDS_MAX:
                c.update(lds_tab=1, nteams=t)
                break
            t >>= 1
        if not c["lds_tab"]:
            c.update(nt=512, nteams=8)
            found = False
            for t in (4, 2, 1):
                for ntl in range(2, 9):
                    step = ((ncolE + ntl - 1) // ntl + 7) & ~7
                    tcols = (step + L + 8 + 7) & ~7
                    if fixed + 8 * (9 * tcols + t * Wcap) <= LDS_MAX:
                        c.update(tiles=ntl, nteams=t)
                        found = True
                        break
                if found:
                    break
        for g in ids:
            cls_of[g] = len(classes)
        classes.append(c)
    return classes, cls_of


def partial_fast(cls, L, gap_start, D, has_n):
    """fig_partial_fast (fig_engine_partial.h:212-224) on the device.  S.left is min(D, gap start) (fig_engine.h), xoff = L - 1.
    The device's extra clause on the wave count always holds by the class table (4 or 8 waves)."""
    if not cls["lds_tab"] or cls["tiles"] > 0:
        return False
    if has_n:
        return False
    if min(D, gap_start) < L - 1:
        return False
    nw = cls["nt"] // 64
    assert nw >= 4 and nw % 4 == 0
    rstride = ((L + 1 + 7) & ~7) + 32
    if cls["nteams"] * cls["Wcap"] < rstride:
        return False
    return (L - 1 + 63) >> 6 <= 4


def detector_parallel(cls, L, prc):
    """Does fig_detect_overlap_par (fig_engine_partial.h:544-553) run its own form, or fall back to lane 0's serial walk?"""
    rl = (L + 15) & ~15
    return bool(cls["lds_tab"]) and cls["tiles"] == 0 and prc <= DET_PAR_MAX_READS and prc * rl <= cls["ncolE"] * 72


def forms(case):
    """Per gap of a partial-mode case: (class dict, "fast" | "generic", "par" | "serial")."""
    L = case.read_len
    classes, cls_of = class_table([gmax_partial(g.length, case.partial_len) for g in case.gaps], L)
    out = []
    for g, ci in zip(case.gaps, cls_of):
        c = classes[ci]
        n = min(len(g.partial), 3001)
        has_n = any(set(r.seq) - set("ACGT") for r in g.partial[:3001])
        out.append((c, "fast" if partial_fast(c, L, g.start, case.max_distance, has_n) else "generic", "par" if detector_parallel(c, L, n) else "serial"))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------
PSTART_L = 50
SEEDS = {"pn": 7105, "pstart_10": 7210, "pstart_48": 7248, "pstart_49": 7249, "p192": 7192, "pmany": 7240, "pwide": 7300, "pwide_n": 7300}

# what each gap must take: (E-step / MLE form, detector form) -- asserted by tests/test_partial_forms.py
EXPECTED_FORMS = {
    "pn": [("generic", "par"), ("fast", "par"), ("generic", "par")],
    "pstart_10": [("generic", "par"), ("fast", "par")],
    "pstart_48": [("generic", "par"), ("fast", "par")],
    "pstart_49": [("fast", "par"), ("fast", "par")],
    "p192": [("fast", "par"), ("fast", "serial")],
    "pmany": [("fast", "serial"), ("fast", "serial")],
    "pwide": [("fast", "par"), ("generic", "serial"), ("generic", "serial")],
    "pwide_n": [("generic", "par"), ("generic", "serial"), ("generic", "serial")],
}


def _cut(case, counts):
    for g, n in zip(case.gaps, counts):
        assert len(g.partial) >= n, (case.name, len(g.partial), n)
        g.partial = g.partial[:n]
    return case


def case_pn(seed=None):
    return synth.make_case("pn", seed or SEEDS["pn"], "partial", [(1500, 25), (3000, 60), (4500, 130)], contig_len=6500, read_len=101, insert_mean=180, insert_sd=10,
                           coverage=20, err=0.005, n_model_pairs=600, partial_n_rate=0.01, partial_n_gaps=[0, 2])


def case_pstart(start, seed=None):
    L = PSTART_L
    return synth.make_case(f"pstart_{start}", seed or SEEDS[f"pstart_{start}"], "partial", [(start, 20), (2500, 40)], contig_len=4500, read_len=L, insert_mean=180,
                           insert_sd=10, coverage=30, err=0.005, n_model_pairs=600)


def case_p192(seed=None):
    c = synth.make_case("p192", seed or SEEDS["p192"], "partial", [(1500, 12), (3000, 12)], contig_len=4500, read_len=50, insert_mean=180, insert_sd=10, coverage=180,
                        err=0.005, n_model_pairs=600)
    return _cut(c, [192, 193])


def case_pmany(seed=None):
    return synth.make_case("pmany", seed or SEEDS["pmany"], "partial", [(1500, 30), (3000, 80)], contig_len=4500, read_len=76, insert_mean=180, insert_sd=10,
                           coverage=200, err=0.005, n_model_pairs=600)


def case_pwide(with_n=False, seed=None):
    name = "pwide_n" if with_n else "pwide"
    return synth.make_case(name, seed or SEEDS[name], "partial", [(1500, 1250), (4500, 1700), (8000, 1800)], contig_len=11500, read_len=101, insert_mean=180,
                           insert_sd=10, coverage=20, err=0.005, n_model_pairs=600, partial_n_rate=0.01 if with_n else 0.0)


def all_cases():
    """{id: builder(seed=None)} of every directed case, in the order of the issue's table."""
    out = {"pn": case_pn}
    for s in (10, PSTART_L - 2, PSTART_L - 1):
        out[f"pstart_{s}"] = (lambda seed=None, s=s: case_pstart(s, seed))
    out["p192"] = case_p192
    out["pmany"] = case_pmany
    out["pwide"] = lambda seed=None: case_pwide(False, seed)
    out["pwide_n"] = lambda seed=None: case_pwide(True, seed)
    return out


def merged(name="pmix", ids=("pn", "pmany", "pwide")):
    """Several cases as ONE case (one batch, one model): every case's scaffold becomes a contig of its own, the gaps keep their
    reads and are numbered in the order of `ids`.  Read length, partial_len and the model pairs are those of the first case,
    which must have the longest reads (pmany's 76-base reads then run beside 101-base ones, in classes whose geometry follows
    L = 101).  All cases must share max_distance."""
    cs = [all_cases()[i]() for i in ids]
    a = cs[0]
    assert all(c.mode == "partial" and c.max_distance == a.max_distance and c.read_len <= a.read_len and len(c.scaffolds) == 1 for c in cs)
    gaps = []
    for ci, c in enumerate(cs):
        for g in c.gaps:
            g.contig = ci
            gaps.append(g)
    return synth.Case(name=name, mode="partial", read_len=a.read_len, insert_mean=a.insert_mean, insert_sd=a.insert_sd, max_distance=a.max_distance,
                      partial_len=a.partial_len, neg_overlap=a.neg_overlap, script_itr=a.script_itr, scaffolds=[c.scaffolds[0] for c in cs],
                      truth=[c.truth[0] for c in cs], gaps=gaps, myout=a.myout, n_pairs=a.n_pairs)


# ---- the oracle's trace --------------------------------------------------------------------------------------------------------
def parse_det(path):
    """DET lines -> [(gap, G, ret0, ret1, psr0, psr1, n_maximal_pairs, false_overlap_flag, partial_read_count)]."""
    return [tuple(int(x) for x in ln.split("\t")[1:10]) for ln in open(path) if ln.startswith("DET\t")]


def det_branches(det):
    """The branches of detect_overlap_gapestimate the DET records show -> set of
    "300" | "30len" | "30len_tie" (two or more pairs of maximal length) | "30len_false" (accepted despite a false overlap) |
    "m100_false" (0 / -1 from a false overlap) | "m100_short" (0 / -1: no pair long enough) | "0_0"."""
    out = set()
    for _, _, r0, r1, _, _, nmax, fo, _ in det:
        if r0 == 300:
            out.add("300")
        elif 1 <= r0 < FIG_MAX_READLEN:
            out.add("30len")
            if nmax >= 2:
                out.add("30len_tie")
            if fo == -1:
                out.add("30len_false")
        elif r1 == -1:
            out.add("m100_false" if fo == -1 else "m100_short")
        elif r0 == 0 and r1 == 0:
            out.add("0_0")
    return out


REQUIRED_BRANCHES = {"300", "30len_tie", "m100_false", "0_0"}


def parse_cands(path):
    cands = {}
    for ln in open(path):
        f = ln.rstrip("\n").split("\t")
        if f[0] == "CAND":
            cands.setdefault(int(f[1]), []).append(float.fromhex(f[4]))
    return cands


def tie_margin(cands):
    """The candidate loop's decisions on likelihoods (Figbird.cpp:6390-6482): `likelihood > maxLikelihood`,
    `likelihood > secondMaxLikelihood` and `|prevlikelihood - likelihood| <= 0.9`.  A device value may sit 1e-6 relative from
    the oracle's, so a decision between two DISTINCT values a, b can flip when its margin is <= 1e-6 (|a| + |b|).  Returns the
    smallest margin / (|a| + |b|) over all decisions (inf when there are none); values equal bit for bit are no decision."""
    worst = float("inf")
    for liks in cands.values():
        best = second = None
        prev = 0.0
        for v in liks:
            if not np.isfinite(v):
                prev = v
                continue
            for ref in (best, second):
                if ref is not None and ref != v:
                    worst = min(worst, abs(v - ref) / (abs(v) + abs(ref)))
            if best is None or v > best:
                best, second = v, best
            elif second is None or v > second:
                second = v
            if np.isfinite(prev) and abs(prev) + abs(v) > 0:
                worst = min(worst, abs(abs(prev - v) - 0.9) / (abs(prev) + abs(v)))
            prev = v
    return worst


def oracle_trace(case, base, level=5):
    """Write the case under `base`, run the oracle in FillGaps mode with the given trace level -> (paths, trace file)."""
    p = synth.write_case(case, os.path.join(base, case.name))
    tr = os.path.join(base, case.name + ".trace")
    env = dict(os.environ, FIG_ORACLE_TRACE=tr, FIG_ORACLE_TRACE_LEVEL=str(level))
    r = subprocess.run([ORACLE, "fillgaps"] + synth.fillgaps_argv(case, p), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return p, tr


if __name__ == "__main__":
    import time
    seen = set()
    with tempfile.TemporaryDirectory() as d:
        for cid, mk in all_cases().items():
            if len(sys.argv) > 1 and cid not in sys.argv[1:]:
                continue
            c = mk()
            t = time.time()
            _, tr = oracle_trace(c, d)
            dt = time.time() - t
            det = parse_det(tr)
            br = det_branches(det)
            seen |= br
            info = [f"G0={g.length} start={g.start} reads={len(g.partial)} capGl={f[0]['capGl']} nt={f[0]['nt']} nteams={f[0]['nteams']} lds_tab={f[0]['lds_tab']} tiles={f[0]['tiles']} {f[1]}/{f[2]}"
                    for g, f in zip(c.gaps, forms(c))]
            print(f"{cid} L={c.read_len} oracle {dt:.1f}s  branches {sorted(br)}  tie margin {tie_margin(parse_cands(tr)):.3g}")
            for ln in info:
                print("   ", ln)
    print("branches over all cases:", sorted(seen), "missing:", sorted(REQUIRED_BRANCHES - seen))
