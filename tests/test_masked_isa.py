"""The masked TL / AD kernels keep the register path's one level of prefetch only if hipcc still counts their loads: every
load is issued unconditionally (an absent field reads the zero line), so the wait for a level's words must not come at the
load site.  Checked on the compiled gfx950 assembly with the project's own guard (csrc/check_ring_isa.py), no GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402


def _compile(tmp_path_factory, src):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    return isa.compile_to_asm(src, str(tmp_path_factory.mktemp("isa")))


@pytest.fixture(scope="module")
def tl_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "cloudsc2_tl.hip")


@pytest.fixture(scope="module")
def ad_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "cloudsc2_ad.hip")


def test_masked_tl_prefetch_is_not_waited_for_at_the_load_site(tl_asm):
    assert isa.check_prefetch_distance(tl_asm, "tl_masked_kernelI") == 8          # T x REG x EVAP, one level loop each
    assert isa.check_prefetch_distance(tl_asm, "tl_masked_kernelIdLb1ELb0E") == 1  # the drivers' switches


def test_masked_ad_prefetch_is_not_waited_for_at_the_load_site(ad_asm):
    assert isa.check_prefetch_distance(ad_asm, "ad_masked_kernelI") == 8          # T x REG x FIX, one sweep each
    assert isa.check_prefetch_distance(ad_asm, "ad_masked_kernelIdLb1ELb1E") == 1  # what autodiff's backward runs


def test_masked_kernels_do_not_spill(tl_asm, ad_asm):
    for asm, key in ((tl_asm, "tl_masked_kernelIdLb1ELb0E"), (tl_asm, "tl_masked_kernelIfLb1ELb0E"),
                     (ad_asm, "ad_masked_kernelIdLb1ELb0E"), (ad_asm, "ad_masked_kernelIfLb1ELb0E"),
                     (ad_asm, "ad_masked_kernelIdLb1ELb1E"), (ad_asm, "ad_masked_kernelIfLb1ELb1E")):
        assert isa.kernel_resources(asm, key)["ScratchSize"] == 0, key


def test_masked_kernels_exist_under_names_the_dense_counts_do_not_match(tl_asm, ad_asm):
    """eight instantiations each, and their mangled names are not picked up by the prefixes tests/test_ring_isa.py counts"""
    for asm, pre in ((tl_asm, "tl_masked_kernelI"), (ad_asm, "ad_masked_kernelI")):
        names = [name for name, _ in isa._kernels(asm, pre)]
        assert len(names) == 8, (pre, names)
        for name in names:
            assert not any(k in name for k in ("tl_kernelI", "ad_kernelI", "nl_kernelI", "tl_ring_kernelI")), name
