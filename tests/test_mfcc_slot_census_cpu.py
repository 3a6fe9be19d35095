"""Issue-slot census of the MFCC kernel compiled for the reference geometry (CPU: hipcc cross-compiles to ISA without a GPU).

kws_mfcc_i16_ref_kernel exists to issue fewer instructions that neither compute nor move data than the generic
wavefront-resident kernel (a wavefront of these kernels issues one instruction per ~6.8 cycles whatever its
kind).  tools/mfcc_slot_census.py counts a kernel's frame-pair loop by kind from the ISA of one compilation; the checks here
are the constraints the kernel was built under and a RELATIVE comparison with the generic kernel of the same compilation --
no absolute count is fixed."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import mfcc_slot_census as census  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(census.lint.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def counts():
    isa = census.lint.compile_to_isa(census.SRC)  # the compilation tests/test_isa_hazards.py lints (cached)
    return {k: census.census(isa, k) for k in ("kws_mfcc_i16_kernel", "kws_mfcc_i16_ref_kernel", "kws_mfcc_i16_ref_noflag_kernel")}


def test_the_census_finds_the_loops_it_counts(counts):
    for name, c in counts.items():
        assert c["transforms"] >= 1 and c["pair"]["packed"] > 100 and c["pair"]["dpp"] > 30 and c["pair"]["lds"] > 50, (name, c)
        assert all(c["chunk"][k] >= c["pair"][k] for k in census.KINDS), name  # the chunk loop contains the pair loop


@pytest.mark.parametrize("kernel", ["kws_mfcc_i16_ref_kernel", "kws_mfcc_i16_ref_noflag_kernel"])
def test_reference_kernel_keeps_its_register_and_scratch_constraints(counts, kernel):
    c = counts[kernel]
    assert c["vgpr_count"] is not None and c["vgpr_count"] <= 128, c["vgpr_count"]  # four wavefronts per SIMD
    assert c["scratch_in_chunk_loop"] == [], c["scratch_in_chunk_loop"]


def test_reference_pair_loop_issues_fewer_non_arithmetic_slots_than_the_generic(counts):
    gen, ref = counts["kws_mfcc_i16_kernel"]["pair"], counts["kws_mfcc_i16_ref_kernel"]["pair"]
    print("[census] kind generic reference: " + ", ".join(f"{k} {gen[k]} {ref[k]}" for k in census.KINDS))
    assert ref["s_nop"] < gen["s_nop"]
    assert ref["scalar"] + ref["branch"] < gen["scalar"] + gen["branch"]
    assert ref["select"] < gen["select"]
