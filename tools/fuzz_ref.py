#!/usr/bin/env python3
"""Dev tool: fuzz the oracle restatement against oracle/_ref over many seeded cases."""
import os, sys, tempfile, shutil, random
from concurrent.futures import ProcessPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from figbird_amd import synth
from tools.compare_ref import compare

def mk(seed):
    rnd = random.Random(seed)
    mode = rnd.choice(["unmapped", "partial", "partial"])
    L = rnd.choice([36, 50, 76, 101])
    err = rnd.choice([0.0, 0.005, 0.02])
    if mode == "partial":
        gaps = []
        pos = 1500
        for _ in range(rnd.randint(2, 5)):
            g = rnd.choice([1, 3, 8, 15, 25, L - 5, L, L + 10, 2 * L, 2 * L + 30, 5 * L])
            gaps.append((pos, g)); pos += g + rnd.randint(800, 1500)
        neg = {}
        if rnd.random() < 0.4:
            gi = rnd.randrange(len(gaps)); neg[gi] = (rnd.choice([5, 10, 20]), rnd.choice([6, 10, 14, 20]))
        return synth.make_case(f"fz{seed}", seed, "partial", gaps, contig_len=pos + 1500, read_len=L,
                               insert_mean=rnd.choice([180, 220]), insert_sd=10, coverage=rnd.choice([3, 10, 30]),
                               err=err, n_model_pairs=1500, neg_overlap_gaps=neg, neg_overlap=rnd.choice([30, 0]),
                               script_itr=rnd.choice([1, 2]))
    else:
        gaps = []
        pos = 1500
        for _ in range(rnd.randint(1, 3)):
            g = rnd.choice([5, 12, 20, 29, 30, 45, 420, 600, 900])
            gaps.append((pos, g)); pos += g + rnd.randint(900, 1500)
        return synth.make_case(f"fz{seed}", seed, "unmapped", gaps, contig_len=pos + 1500, read_len=L,
                               insert_mean=rnd.choice([400, 600]), insert_sd=rnd.choice([20, 40]),
                               coverage=rnd.choice([4, 12, 25]), err=err, n_model_pairs=1500,
                               partial_reads_in_unmapped=rnd.random() < 0.7, read_n_rate=rnd.choice([0, 0, 0.01]),
                               script_itr=rnd.choice([1, 2]))

def mk_mid(seed):
    """Unmapped cases of the 134-400 bracket (candidate range [0.5 G0, 2.5 G0], Figbird.cpp:6894-6901; large_gap_flag off, up
    to ~400 candidate lengths per gap), which mk() leaves out for its CPU cost: one gap, few reads."""
    rnd = random.Random(seed)
    L = rnd.choice([36, 50])
    g = rnd.choice([134, 150, 180, 230, 300, 400])
    return synth.make_case(f"fzm{seed}", seed, "unmapped", [(1500, g)], contig_len=1500 + g + 1500, read_len=L,
                           insert_mean=rnd.choice([400, 600]), insert_sd=rnd.choice([20, 40]), coverage=rnd.choice([3, 5]),
                           err=rnd.choice([0.0, 0.01]), n_model_pairs=1200, partial_reads_in_unmapped=rnd.random() < 0.7,
                           read_n_rate=rnd.choice([0, 0.01]), script_itr=1)


# ---- read length as a dimension (tests/test_read_lengths.py, tests/test_gpu_parity.py) -------------------------------------
# L picks device code: the partial E-step's tile count (<LDS,2> up to L = 129, <LDS,4> for 130-200), its row strides (L % 8,
# L % 16), the shared-factor chain's tail (L % 4), the pair form below L = 32, and the buffers sized for FIG_MAX_READLEN = 200.
READLEN_SWEEP = [31, 32, 35, 63, 64, 75, 127, 128, 129, 130, 143, 144, 151, 199, 200]
REF_MAX_HANG = 104          # oracle/README.md, "Read-length domain": partial_left[100] / partial_right[100], Figbird.cpp:1625


def mk_readlen(mode, L, seed=None):
    """One small case per (mode, L): two gaps, low coverage (seconds for the CPU oracle and the one-lane emulation), reads placed
    in both gaps.  partial: a gap of L + 10 bp (candidate lengths 0 .. 5 (L + 10), Figbird.cpp:6886: both sides of the E-step's
    G = 128 TS switch, for TS = 2 and TS = 4 alike) and one of 600 bp (one candidate length, left and right tile groups apart).
    unmapped: 600 bp (one candidate length) next to 12 bp (up to 3 L candidate lengths, which the CPU can afford up to L = 75)
    or 450 bp, with the frag library's clipped reads alongside: every candidate runs the chain whose tail L % 4 selects."""
    seed = 900 + L if seed is None else seed
    if mode == "partial":
        gaps, pos = [], 1500
        for g in (L + 10, 600):
            gaps.append((pos, g)); pos += g + 1200
        return synth.make_case(f"rl_p{L}", seed, "partial", gaps, contig_len=pos + 300, read_len=L, insert_mean=max(180, 2 * L + 40),
                               insert_sd=10, coverage=4, err=0.005, n_model_pairs=400)
    gaps, pos = [], 1500
    for g in ((12, 600) if L <= 75 else (450, 600)):
        gaps.append((pos, g)); pos += g + 1300
    return synth.make_case(f"rl_u{L}", seed, "unmapped", gaps, contig_len=pos + 200, read_len=L, insert_mean=600, insert_sd=30,
                           coverage=8, err=0.005, n_model_pairs=400, partial_reads_in_unmapped=True)


def max_hang(case):
    """The most bases any clipped (partial) read of the case hangs into its gap, capped by the gap's longest candidate length:
    what the reference indexes partial_left / partial_right with (Figbird.cpp:1974-2009, :2053-2084)."""
    worst = 0
    for g in case.gaps:
        gmax = max(g.length, int(2.5 * g.length)) if g.length <= 400 else g.length
        if case.mode == "unmapped" and g.length < 30:
            gmax = max(gmax, 70)
        for r in g.partial:
            hang = len(r.seq) - r.clipped_index - 1 if r.match in (1, 4) else r.clipped_index
            worst = max(worst, min(hang, gmax))
    return worst


def ref_defined(case):
    """Is the reference's own behaviour defined on this case (oracle/README.md, "Read-length domain")?"""
    return max_hang(case) <= REF_MAX_HANG and case.read_len < 200      # char[MAX_READLENGTH = 200] holds 199 bases, Figbird.cpp:2544


def clip_hang(case, limit=REF_MAX_HANG):
    """Drop the clipped reads that hang more than `limit` bases into their gap: what is left is inside the reference's domain."""
    for g in case.gaps:
        g.partial = [r for r in g.partial if (len(r.seq) - r.clipped_index - 1 if r.match in (1, 4) else r.clipped_index) <= limit]
    return case


def one(seed):
    base = tempfile.mkdtemp(prefix=f"figfz{seed}_")
    try:
        c = mk(seed)
        ok = compare(c, base, verbose=False)
        return seed, ok, c.mode, [g.length for g in c.gaps]
    except Exception as e:
        return seed, False, "EXC " + repr(e), []
    finally:
        shutil.rmtree(base, ignore_errors=True)

if __name__ == "__main__":
    a, b = int(sys.argv[1]), int(sys.argv[2])
    bad = []
    with ProcessPoolExecutor(max_workers=int(os.environ.get("FIG_WORKERS", "8"))) as ex:
        for seed, ok, mode, gl in ex.map(one, range(a, b)):
            print(seed, "OK" if ok else "MISMATCH", mode, gl, flush=True)
            if not ok: bad.append(seed)
    print("bad seeds:", bad)
