#!/usr/bin/env python3
"""Generate tests/golden/gap_deal.json (needs oracle/_ref/FillGaps.out and the reference's Figbird.cpp, which FillGaps.out
compiles at run time: pass its path as argv[1]).

The read-less cases of tests/test_abi_and_host.py::test_gap_deal_matches_live_reference, run through the REFERENCE's
FillGaps.out ($num_threads worker processes): the fixture holds the four files that test compares (gaploads.txt, draw.txt,
gapout.txt, filledContigs.fa) as text, keyed like the test's parameter ids.  The inputs are not stored: synth.make_case
regenerates them from the seed.  FillGaps.cpp builds its file names in 100-byte buffers, so the reference runs in a short
scratch directory with relative paths.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from figbird_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gap_deal.json")
FILES = ("gaploads.txt", "draw.txt", "gapout.txt", "filledContigs.fa")
# (parameter id of the test, gap lengths, $num_threads)
CASES = [("lens0-5", [20, 500, 25, 600, 18, 33, 700], 5),
         ("lens1-3", [500, 20, 600, 700, 30, 800, 900, 450, 25, 1000, 40, 1100], 3)]


def deal_case(lens):
    specs, pos = [], 300
    for n in lens:
        specs.append((pos, n)); pos += n + 400
    return synth.make_case("deal", 5, "unmapped", specs, contig_len=pos + 400, coverage=0.0, n_model_pairs=300)


def relative_paths(paths, cwd):
    return {k: (os.path.relpath(v, cwd) + ("/" if v.endswith("/") else "")) if isinstance(v, str) and v.startswith(cwd) else v
            for k, v in paths.items()}


def main(figbird_cpp):
    exe = os.path.join(ROOT, "oracle", "_ref", "FillGaps.out")
    out = {}
    for cid, lens, threads in CASES:
        case = deal_case(lens)
        with tempfile.TemporaryDirectory(prefix="deal") as d:
            p = synth.write_case(case, os.path.join(d, "c"))
            os.symlink(os.path.abspath(figbird_cpp), os.path.join(d, "Figbird.cpp"))
            r = subprocess.run([exe] + synth.fillgaps_argv(case, relative_paths(p, d), n_threads=threads), cwd=d,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{cid}: FillGaps.out exited {r.returncode}: {r.stderr}")
            out[cid] = {"lens": lens, "threads": threads, "files": {fn: open(p["tmp"] + fn).read() for fn in FILES}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
