"""The kernels of cloudsc2_ad_evap.hip on the compiled gfx950 assembly, with the helpers of csrc/check_ring_isa.py (no GPU):
none of the 32 instantiations spills, no batch of level loads - sweep 1's and sweep 2's - is waited for at its load site, and
the families of cloudsc2_ad.hip are the instantiations they were."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

FAMILIES = ("ad_cover_kernelI", "ad_cover_step_kernelI", "ad_cover_dirs_kernelI", "ad_cover_dirs_step_kernelI")
COUNTED_ELSEWHERE = ("9ad_kernelI", "ad_masked_kernelI", "ad_step_kernelI", "masked_kernelI", "ad_dirs_kernelI",
                     "ad_dirs_step_kernelI", "ad_ens_kernelI", "ad_ens_step_kernelI", "tl_kernelI", "nl_kernelI")


def _compile(tmp_path_factory, src):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    return isa.compile_to_asm(src, str(tmp_path_factory.mktemp("isa")))


@pytest.fixture(scope="module")
def evap_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "cloudsc2_ad_evap.hip")


@pytest.fixture(scope="module")
def ad_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "cloudsc2_ad.hip")


def _names(asm, family):
    return [n for n, _ in isa._kernels(asm, family)]


def test_eight_instantiations_per_family_under_names_nobody_else_counts(evap_asm):
    seen = set()
    for family in FAMILIES:
        names = _names(evap_asm, family)
        assert len(names) == 8, (family, names)                     # T x REG x FIX
        for name in names:
            assert not any(k in name for k in COUNTED_ELSEWHERE), name
        assert not seen & set(names)
        seen |= set(names)
    for k in COUNTED_ELSEWHERE:                                      # the new unit defines none of the existing kernels
        assert not _names(evap_asm, k), k


def test_no_instantiation_spills(evap_asm):
    spills = {n: isa.kernel_resources(evap_asm, n)["ScratchSize"] for f in FAMILIES for n in _names(evap_asm, f)}
    assert len(spills) == 32
    assert not {n: s for n, s in spills.items() if s}, {n: s for n, s in spills.items() if s}


def test_fp32_single_kernels_keep_two_waves_per_simd(evap_asm):
    for family in FAMILIES[:2]:
        for name in _names(evap_asm, family + "f"):
            assert isa.kernel_resources(evap_asm, name)["Occupancy"] >= 2, name


def test_level_batches_are_not_waited_for_at_the_load_site(evap_asm):
    """`check_prefetch_distance` raises on a batch that is; every instantiation's sweep 2 must have been seen"""
    for family in FAMILIES:
        for name in _names(evap_asm, family):
            assert isa.check_prefetch_distance(evap_asm, name) >= 1, name


def test_the_families_of_cloudsc2_ad_are_what_they_were(ad_asm):
    for family, n in (("ad_masked_kernelI", 8), ("ad_step_kernelI", 8), ("ad_dirs_kernelI", 8), ("ad_dirs_step_kernelI", 8),
                      ("ad_ens_kernelI", 8), ("ad_ens_step_kernelI", 8), ("9ad_kernelI", 40)):
        assert len(_names(ad_asm, family)) == n, (family, len(_names(ad_asm, family)))
    assert not _names(ad_asm, "ad_cover")
