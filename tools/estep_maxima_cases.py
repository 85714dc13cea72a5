#!/usr/bin/env python3
"""Directed cases for the per-read maxima of the shared-factor E-step (figbird_amd/csrc/fig_engine_shared.h): the maximum is
taken in phase A, per (tile of 64 placements, reads of the unit), by a transposing reduction over the wave and an atomic
maximum on the read's maxlv word; phase B finds the offset by comparing its products with that maximum; the flop credit of
a regular read is a closed form of its window.  Cases are built like those of tools/estep_cases.py (synth.make_case plus an
edit) and use its restated integer arithmetic (split_plan, sh_applies, nt_of_class).

All gaps are at L = 36 and longer than 400 bp, where the few reads leave one candidate per gap (G = G0), so that a case's
Wn = G0 + L - 1, its tiles and its split round are known from its parameters:

  n<N>          405 bp, 256 threads, 7 tiles: N = 1, 31, 32, 33, 127, 129 reads (a partial last chunk; 129 crosses the super-chunk)
  w448 | w449   413 | 414 bp: Wn = 7 x 64 (a full last tile) | 7 x 64 + 1 (a last tile with one live lane), 40 reads
  u256_<NS>     405 bp with 40 | 70 reads: the left-over items run fig_sh_unit<16> | <8> (4 waves cannot reach <4>)
  u512_<NS>     500 bp, 512 threads, 9 tiles with 70 | 40 | 20 reads: <16> | <8> | <4>
  empty         405 bp, 40 reads, reads 5 and 33 anchored 800 bp further out: their insert-size window is empty
  mixed         405 bp, 70 reads: chunk 0 holds an N-base read (slot 3) and a short read (slot 9, L - 5 bases) among regular
                reads, chunk 1 has reads 32..63 all with an N base (no regular read), chunk 2 is regular

  python3 tools/estep_maxima_cases.py     # list the cases with their windows' relation to the tiles
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import estep_cases as ec  # noqa: E402

L = 36
N_READS = (1, 31, 32, 33, 127, 129)
UNITS = {"u256_16": (405, 40, 16), "u256_8": (405, 70, 8), "u512_16": (500, 70, 16), "u512_8": (500, 40, 8), "u512_4": (500, 20, 4)}
EMPTY_SLOTS = (5, 33)
MIXED_N, MIXED_SHORT, MIXED_CHUNK = 3, 9, list(range(32, 64))


def _gap(name, seed, g0, n):
    return ec._one_gap(name, seed, g0, L, n)


def far_anchor(case, gi, slots, by=800):
    """The anchors of the mates `slots` moved `by` bp away from the gap: no placement keeps the insert size inside [Tmin, Tmax]."""
    g = case.gaps[gi]
    for s in slots:
        r = g.unmapped[s]
        assert r.anchor_pos1 - 1 < g.start and r.anchor_pos1 > by, (s, r.anchor_pos1)
        r.anchor_pos1 -= by
    return case


def shorten(case, gi, slot, by=5):
    r = case.gaps[gi].unmapped[slot]
    r.mate_seq_fastq = r.mate_seq_fastq[:len(r.mate_seq_fastq) - by]
    return case


def case_empty():
    c = _gap("empty", 5405, 405, 40)
    left = [s for s, r in enumerate(c.gaps[0].unmapped) if r.anchor_pos1 - 1 < c.gaps[0].start and r.anchor_pos1 > 800]
    assert len(left) >= 2
    # the listed slots when they are left-anchored, else the nearest left-anchored ones
    pick = [min(left, key=lambda s: abs(s - want)) for want in EMPTY_SLOTS]
    assert len(set(pick)) == 2
    return far_anchor(c, 0, pick), pick


def case_mixed():
    c = _gap("mixed", 6405, 405, 70)
    ec.write_n(c, 0, [MIXED_N] + MIXED_CHUNK)
    return shorten(c, 0, MIXED_SHORT)


def all_cases():
    out = {}
    for n in N_READS:
        out[f"n{n}"] = (lambda n=n: _gap(f"n{n}", 7000 + n, 405, n))
    out["w448"] = lambda: _gap("w448", 7413, 413, 40)
    out["w449"] = lambda: _gap("w449", 7414, 414, 40)
    for cid, (g0, n, _) in UNITS.items():
        out[cid] = (lambda cid=cid, g0=g0, n=n: _gap(cid, 8000 + g0 + n, g0, n))
    out["empty"] = lambda: case_empty()[0]
    out["mixed"] = case_mixed
    return out


def windows(batch, gi, Tmin, Tmax, G):
    """fig_window_u (fig_engine_hot.h) for the left-anchored reads of gap gi at candidate length G = G0: [(slot, lo, hi)];
    right-anchored reads are left out (their window moves with the candidate's offset)."""
    a, b = int(batch.u_read_off[gi]), int(batch.u_read_off[gi + 1])
    gs = int(batch.gap_start[gi])
    out = []
    for s in range(a, b):
        pos1, ln = int(batch.u_anchor_pos[s]), int(batch.u_seq_off[s + 1] - batch.u_seq_off[s])
        if pos1 < gs:
            tis0 = gs - pos1 + ln
            out.append((s - a, max(-(ln - 1), Tmin - tis0), min(G - 1, Tmax - tis0)))
    return out


if __name__ == "__main__":
    for cid, mk in all_cases().items():
        c = mk()
        g = c.gaps[0]
        nt = ec.nt_of_class(g.length)
        sp = sorted(set(32 // p[4] if p[4] else 0 for p in ec.split_plan(len(g.unmapped), g.length, c.read_len, nt)))
        print(cid, f"G0={g.length} Wn={g.length + L - 1} reads={len(g.unmapped)} nt={nt} units={sp}")
