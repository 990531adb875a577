"""The multi-direction adjoint kernels (`ad_dirs_kernel`, `ad_dirs_step_kernel`) on the compiled gfx950 assembly
(csrc/check_ring_isa.py, no GPU needed): eight instantiations each under names no other check counts, the families that
were there are what they were, nothing spills to scratch, and the prefetch of the next level is not waited for at its
load site.

`check_prefetch_distance` judges every batch of >= 14 loads inside a loop of >= 600 lines by the first wait that reaches
into it, in program order.  The LEVEL batch of these kernels (15 or 16 state words, `aph` and the two trajectory flux
words of the next level) is such a batch; it is issued in front of ad_forward and first waited for behind the first
direction's ad_backward.  Left unchecked: the per-DIRECTION forcing batch is at most nine loads, below the helper's
threshold of 14, so whether the next direction's forcing is waited for early is not seen by this test.  No occupancy figure
is asserted either; docs/TUNING_LOG.md 3.19 records what hipcc gave."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

FAMILIES = ("ad_dirs_kernelI", "ad_dirs_step_kernelI")
#: the substrings tests/test_masked_isa.py, test_step_isa.py and check_all count instantiations by
COUNTED_ELSEWHERE = ("9ad_kernelI", "ad_masked_kernelI", "ad_step_kernelI", "masked_kernelI")


@pytest.fixture(scope="module")
def ad_asm(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    return isa.compile_to_asm("cloudsc2_ad.hip", str(tmp_path_factory.mktemp("isa")))


def _names(asm, family):
    return [n for n, _ in isa._kernels(asm, family)]


def test_eight_instantiations_per_family_under_names_nobody_else_counts(ad_asm):
    for family in FAMILIES:
        names = _names(ad_asm, family)
        assert len(names) == 8, (family, names)            # T x REG x FIX
        for name in names:
            assert not any(k in name for k in COUNTED_ELSEWHERE), name
    assert not set(_names(ad_asm, FAMILIES[0])) & set(_names(ad_asm, FAMILIES[1]))
    # ... and the families that were there are the eight instantiations each that they were
    for family in ("ad_masked_kernelI", "ad_step_kernelI"):
        assert len(_names(ad_asm, family)) == 8, family


def test_no_instantiation_spills(ad_asm):
    seen = 0
    for family in FAMILIES:
        for name in _names(ad_asm, family):
            assert isa.kernel_resources(ad_asm, name)["ScratchSize"] == 0, name
            seen += 1
    assert seen == 16


def test_the_level_prefetch_is_not_waited_for_at_the_load_site(ad_asm):
    for family in FAMILIES:
        for name in _names(ad_asm, family):
            assert isa.check_prefetch_distance(ad_asm, name) >= 1, name
