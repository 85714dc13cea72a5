"""Read length as a dimension.  L selects code in the engine -- the partial E-step's tile count (two tiles per side up to
L = 129, four for 130-200), its row strides (L % 8, L % 16), the shared-factor chain's tail (L % 4), the pair form below
L = 32, the buffers sized for FIG_MAX_READLEN = 200 -- so the one-lane emulation of the engine is compared with the oracle
byte for byte across those edges, in both modes, and the oracle with the reference's own binary wherever the reference's
behaviour is defined (oracle/README.md, "Read-length domain": clipped reads at most 104 bases inside the gap, L <= 199)."""
import os

import pytest

import util
from tools.compare_emu import run_one
from tools.compare_ref import compare
from tools.fuzz_ref import READLEN_SWEEP, REF_MAX_HANG, clip_hang, max_hang, mk_readlen, ref_defined

MODES = ["partial", "unmapped"]


@pytest.mark.parametrize("L", READLEN_SWEEP)
@pytest.mark.parametrize("mode", MODES)
def test_emulation_matches_oracle_across_read_lengths(mode, L, tmp_path):
    """Output files, placeReads calls and algorithmic flops of the emulation equal the oracle's; the case is a live one: the
    oracle evaluated candidates for every gap and placed reads (valid_count > 0) in each."""
    case = mk_readlen(mode, L)
    assert case.read_len == L and all(len(g.partial) > 0 for g in case.gaps)
    assert run_one(case, str(tmp_path), exe=util.EMU, verbose=False, trace=True)
    cands, _ = util.parse_trace(os.path.join(str(tmp_path), "ora.trace"))
    for g in range(len(case.gaps)):
        assert g in cands and max(c[3] for c in cands[g]) > 0, f"gap {g}: no read placed"


@pytest.mark.skipif(not os.path.exists(util.REF_FIGBIRD), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("L", READLEN_SWEEP)
@pytest.mark.parametrize("mode", MODES)
def test_oracle_matches_live_reference_across_read_lengths(mode, L, tmp_path):
    """The sweep's cases as they are where the reference is defined on them; otherwise (a clipped read hangs more than 104
    bases into a gap, or L = 200) the same case at the nearest point of the domain: L = 199 for 200, the offending reads taken
    out.  Outside the domain the oracle is the definition and there is nothing to compare."""
    case = mk_readlen(mode, min(L, 199))
    if not ref_defined(case):
        clip_hang(case)
    assert ref_defined(case) and max_hang(case) <= REF_MAX_HANG
    assert compare(case, str(tmp_path), verbose=False)


def test_sweep_reaches_both_sides_of_the_reference_domain():
    """The sweep is not confined to the reference's domain: most cases from L = 128 up hold reads that hang more than 104 bases
    into a gap (there the emulation and the device answer to the oracle alone), every shorter one is inside it."""
    inside = {(m, L) for m in MODES for L in READLEN_SWEEP if ref_defined(mk_readlen(m, L))}
    assert all((m, L) in inside for m in MODES for L in READLEN_SWEEP if L <= 75)
    assert all((m, 200) not in inside for m in MODES)
    assert sum((m, L) not in inside for m in MODES for L in READLEN_SWEEP if L >= 128) >= 12
