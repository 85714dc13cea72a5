#!/usr/bin/env python3
"""Golden fixtures at the BENCH's own regime (this container only; needs oracle/_ref built from /root/reference).

bench.py's step is dominated by <= 400-bp gaps of the jump library (L = 150, insert N(3500, 350), D = 4025, 0.5 %
substitutions) at hundreds to thousands of reads per gap: 140-400 candidate lengths x 8-16 EM iterations each through
the candidate-parallel scheduler and its early-stop replay (Figbird.cpp:6298-6482).  One such gap costs the reference
10^3 CPU-seconds, so the comparison is made once, here, and committed:

  ref/gapout0.txt, gaptofill0.txt, draw0.txt      <- oracle/_ref/Figbird.out (-O2), Figbird.cpp main
  ref/gapout.txt, filledContigs.fa, Ncount.txt, draw.txt
                                                  <- oracle/_ref/FillGaps.out, which compiles and runs Figbird.cpp as shipped (-O0)
  ref/cands.json   per-candidate records (gapEstimate, EM iterations, likelihood as hex float, valid_count)   } from the oracle's
  ref/planes.npz   planes (i) countsGap and (ii) per-read E-step maxima after the last E-step of a spread of } level-4 trace, kept
                   candidates (float64)                                                                      } only after the oracle's
                                                                                                               text outputs equalled
                                                                                                               the reference's bytes
Fixtures are data only (inputs + expected outputs).

  python3 tools/make_bench_golden.py prepare          # writes /tmp/figbench_gold/<case>/{ref2,orc,fg} + jobs.txt
  (run the jobs, e.g. `xargs -P 6 -a /tmp/figbench_gold/jobs.txt -d '\n' -n 1 sh -c`)
  python3 tools/make_bench_golden.py collect [case..] # checks oracle == reference, writes tests/golden/<case>.tar.gz
"""
import json, os, shutil, subprocess, sys, tarfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from figbird_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
ORACLE = os.path.join(ROOT, "oracle", "figbird_oracle")
OUT = os.path.join(ROOT, "tests", "golden")
WORK = "/tmp/figbench_gold"
MODEL_SEED = 7

# name: gap length G0, reads in the gap (before the generator's edge filter), batch seed
CASES = {
    "bench_b25": dict(g0=25, reads=600, seed=9001),           # <= 30 bracket
    "bench_b100": dict(g0=100, reads=800, seed=9002),         # 31-133 bracket
    "bench_b160": dict(g0=160, reads=800, seed=9003),         # 134-400 bracket (candidates 80..400)
    "bench_cap40": dict(g0=40, reads=2990, seed=9004),        # <= 400 bp at the 3000-read cap
    "bench_c1100": dict(g0=1100, reads=700, seed=9005),       # one candidate; 1398 table columns: the one-weight-row LDS class
    "bench_t1800": dict(g0=1800, reads=900, seed=9006),       # one candidate; 2098 columns: the LDS-tiled class
    # candidates 74..372 in the 256-thread class (longest probe 447 columns): the sweep crosses G + L - 1 = 512 | 513, where
    # fig_sh_applies (fig_engine_shared.h) hands the E-step from the shared-factor form to the pair form inside ONE gap.  Few
    # reads and a 900-bp insert keep the 299 candidates affordable for the CPU (tests/test_estep_forms.py).
    "bench_x149": dict(g0=149, reads=40, seed=9007, insert=(900.0, 90.0), planes=(362, 363, 364, 365)),
}
N_PLANE_CANDS = 10


def spec_of(c):
    spec = synth.BenchSpec(mode="unmapped", reads_per_gap_mean=float(c["reads"]))
    if "insert" in c:
        spec.insert_mean, spec.insert_sd = c["insert"]
    return spec


def make(name):
    """(batch, model case, spec) of a fixture, exactly as generated (tests rebuild the in-memory batch from this)."""
    c = CASES[name]
    spec = spec_of(c)
    mc = synth.bench_model_case(MODEL_SEED, spec)
    batch, _ = synth.make_bench_batch(c["seed"], 1, spec, gap_lengths=np.array([c["g0"]]))
    return batch, mc, spec


def argv_of(name, mc, spec, paths, figbird):
    sim = str(CASES[name].get("set_inputmean", 0))
    if figbird:      # Figbird.cpp:6957-6973
        return [paths["scf"], str(spec.max_distance), str(spec.read_len), "1", "0", "1", "0", "1", paths["myout"], paths["tmp"], paths["gaps"],
                "30", str(mc.partial_len), "400", sim, str(int(spec.insert_mean))]
    return [paths["scf"], str(spec.max_distance), str(spec.read_len), "1", "0", "1", "1", paths["myout"], paths["tmp"], paths["gaps"],
            "30", str(mc.partial_len), "10", sim, str(int(spec.insert_mean))]


def prepare():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK)
    jobs = []
    for name, c in CASES.items():
        batch, mc, spec = make(name)
        nreads = int(batch.u_read_off[1])
        assert nreads <= 3000, (name, nreads)
        cost = nreads * (c["g0"] + 150) * (300 if c["g0"] <= 400 else 1)
        for sub in ("ref2", "orc", "fg"):
            root = os.path.join(WORK, name, sub)
            p = synth.write_batch_subset(batch, [0], mc, root, spec)
            if sub == "ref2":
                synth.write_gaploads(p, [0])
                cmd = f"cd {root} && {REF}/Figbird.out " + " ".join(argv_of(name, mc, spec, p, True)) + " > log.txt 2>&1; echo $? > rc"
                jobs.append((cost, cmd))
            elif sub == "orc":
                synth.write_gaploads(p, [0])
                cmd = (f"cd {root} && FIG_ORACLE_TRACE={root}/o.trace FIG_ORACLE_TRACE_LEVEL=4 {ORACLE} figbird " +
                       " ".join(argv_of(name, mc, spec, p, True)) + " > log.txt 2>&1; echo $? > rc")
                jobs.append((cost, cmd))
            else:
                cwd = os.path.join(root, "cwd"); os.makedirs(cwd)
                os.symlink("/root/reference/Figbird.cpp", os.path.join(cwd, "Figbird.cpp"))
                cmd = f"cd {cwd} && {REF}/FillGaps.out " + " ".join(argv_of(name, mc, spec, p, False)) + " > ../log.txt 2>&1; echo $? > ../rc"
                jobs.append((cost * 4.2, cmd))
        print(name, "reads", nreads, flush=True)
    jobs.sort(key=lambda t: -t[0])
    with open(os.path.join(WORK, "jobs.txt"), "w") as f:
        for _, cmd in jobs:
            f.write(cmd + "\n")
    print(len(jobs), "jobs in", os.path.join(WORK, "jobs.txt"))


def parse_level4(path):
    """-> cands [(G, iters, lik_hex, valid)], planes {G: (counts[G,5], rmax[R])} (last E/R before each CAND)."""
    cands, planes, e, r = [], {}, None, None
    for ln in open(path):
        f = ln.rstrip("\n").split("\t")
        if f[0] == "E":
            e = (int(f[2]), f[4:])
        elif f[0] == "R":
            r = (int(f[2]), f[4:])
        elif f[0] == "CAND":
            G = int(f[2])
            cands.append((G, int(f[3]), f[4], int(f[5])))
            if e and e[0] == G and r and r[0] == G:
                planes[G] = (e[1], r[1])
            e = r = None
    return cands, planes


def collect(name):
    base = os.path.join(WORK, name)
    for sub in ("ref2", "orc", "fg"):
        rc = open(os.path.join(base, sub, "rc")).read().strip()
        assert rc == "0", (name, sub, rc)
    rd = lambda *p: open(os.path.join(base, *p), "rb").read()
    # the restatement is pinned at this regime before its planes are kept
    for fn in ("gapout0.txt", "gaptofill0.txt", "draw0.txt"):
        assert rd("ref2", "tmp", fn) == rd("orc", "tmp", fn), f"{name}: oracle != reference on {fn}"
    # the as-shipped -O0 worker process agrees with the -O2 build (one worker: merged files = its files)
    assert rd("fg", "tmp", "gapout.txt") == rd("ref2", "tmp", "gapout0.txt"), name
    assert rd("fg", "tmp", "draw.txt") == rd("ref2", "tmp", "draw0.txt"), name
    cands, planes = parse_level4(os.path.join(base, "orc", "o.trace"))
    stats = [ln for ln in open(os.path.join(base, "orc", "o.trace")) if ln.startswith("STATS")]
    Gs = [c[0] for c in cands if c[0] in planes]
    best = max(cands, key=lambda c: float.fromhex(c[2]))[0] if cands else None
    pick = sorted(set([Gs[int(round(i * (len(Gs) - 1) / max(1, N_PLANE_CANDS - 1)))] for i in range(min(N_PLANE_CANDS, len(Gs)))] + ([best] if best in planes else []) +
                      [G for G in CASES[name].get("planes", ()) if G in planes]))
    arrs = {}
    for G in pick:
        e, r = planes[G]
        arrs[f"counts_{G}"] = np.array([float.fromhex(x) for x in e]).reshape(-1, 5)
        arrs[f"rmax_{G}"] = np.array([float.fromhex(x) for x in r])
    root = os.path.join(base, "pack", name)
    shutil.rmtree(os.path.join(base, "pack"), ignore_errors=True)
    shutil.copytree(os.path.join(base, "ref2"), root, ignore=shutil.ignore_patterns("log.txt", "rc", "gapout0.txt", "gaptofill0.txt", "draw0.txt", "gaploads.txt"))
    refdir = os.path.join(root, "ref"); os.makedirs(refdir)
    for fn in ("gapout0.txt", "gaptofill0.txt", "draw0.txt"):
        shutil.copy(os.path.join(base, "ref2", "tmp", fn), refdir)
    for fn in ("gapout.txt", "filledContigs.fa", "Ncount.txt", "draw.txt"):
        shutil.copy(os.path.join(base, "fg", "tmp", fn), refdir)
    np.savez_compressed(os.path.join(refdir, "planes.npz"), **arrs)
    with open(os.path.join(refdir, "cands.json"), "w") as f:
        json.dump({"cands": cands, "plane_cands": pick, "stats": stats[0].split("\t")[1:] if stats else None}, f)
    batch, mc, spec = make(name)
    p = {"scf": "scf.fa", "myout": "tmp/myout.sam", "tmp": "tmp/", "gaps": "gaps/"}
    meta = {"name": name, "figbird_argv": argv_of(name, mc, spec, p, True), "fillgaps_argv": argv_of(name, mc, spec, p, False),
            "mode": "unmapped", "n_gaps": 1, "g0": CASES[name]["g0"], "n_reads": int(batch.u_read_off[1]), "n_cands": len(cands),
            "set_inputmean": CASES[name].get("set_inputmean", 0)}
    with open(os.path.join(root, "meta.json"), "w") as f:
        json.dump(meta, f)
    tgz = os.path.join(OUT, name + ".tar.gz")
    with tarfile.open(tgz, "w:gz") as t:
        t.add(root, arcname=name)
    return tgz, len(cands), pick


if __name__ == "__main__":
    if sys.argv[1] == "prepare":
        prepare()
    else:
        for name in (sys.argv[2:] or list(CASES)):
            print(collect(name), flush=True)
