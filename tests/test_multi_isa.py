"""The multi-direction tangent-linear kernels (`tl_dirs_kernel`, `tl_dirs_step_kernel`) on the compiled gfx950 assembly
(csrc/check_ring_isa.py, no GPU needed): eight instantiations each under names no other check counts, nothing spills to
scratch, and no prefetch is waited for at its load site.

`check_prefetch_distance` judges every batch of >= 14 loads inside a loop of >= 600 lines by the first wait that reaches
into it, in program order.  These kernels have two such batches: the next LEVEL's state words (outer loop) and the next
DIRECTION's perturbation words (inner loop, which is itself that long).  The helper expresses both; it does not tell which
of the two a batch is, so what is asserted is the number of batches seen: two in the instantiations `tl_multi` /
`tl_step_multi` launch with the drivers' switches, at least one in every other (hipcc may split a batch of one of the
evaporation instantiations below the helper's threshold).  Left unchecked: that the five carry words per direction are
the only LDS traffic of the direction loop."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

FAMILIES = ("tl_dirs_kernelI", "tl_dirs_step_kernelI")
#: the substrings tests/test_masked_isa.py, test_step_isa.py, test_ring_isa.py and check_all count instantiations by
COUNTED_ELSEWHERE = ("tl_kernelI", "tl_masked_kernelI", "tl_step_kernelI", "masked_kernelI", "tl_ring_kernelI")


@pytest.fixture(scope="module")
def tl_asm(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    return isa.compile_to_asm("cloudsc2_tl.hip", str(tmp_path_factory.mktemp("isa")))


def _names(asm, family):
    return [n for n, _ in isa._kernels(asm, family)]


def test_eight_instantiations_per_family_under_names_nobody_else_counts(tl_asm):
    for family in FAMILIES:
        names = _names(tl_asm, family)
        assert len(names) == 8, (family, names)            # T x REG x EVAP
        for name in names:
            assert not any(k in name for k in COUNTED_ELSEWHERE), name
    assert not set(_names(tl_asm, FAMILIES[0])) & set(_names(tl_asm, FAMILIES[1]))
    # ... and the families that were there are the eight instantiations each that they were
    for family in ("tl_masked_kernelI", "tl_step_kernelI", "tl_ring_kernelI"):
        assert len(_names(tl_asm, family)) == 8, family


def test_no_instantiation_spills(tl_asm):
    for family in FAMILIES:
        for name in _names(tl_asm, family):
            assert isa.kernel_resources(tl_asm, name)["ScratchSize"] == 0, name


def test_fp32_keeps_two_waves_per_simd(tl_asm):
    """what the LDS budget of the launcher assumes: at most 3 workgroups of 40 KB carry + level table per CU"""
    for family in FAMILIES:
        assert isa.kernel_resources(tl_asm, family + "fLb1ELb0E")["Occupancy"] >= 2


def test_prefetches_are_not_waited_for_at_the_load_site(tl_asm):
    for family in FAMILIES:
        for name in _names(tl_asm, family):
            assert isa.check_prefetch_distance(tl_asm, name) >= 1, name
        for t in "df":                                     # LREGCL, no evaporation: what the derivative rules launch
            assert isa.check_prefetch_distance(tl_asm, f"{family}{t}Lb1ELb0E") == 2, (family, t)
