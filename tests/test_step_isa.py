"""The step kernels (`tl_step_kernel`, `ad_step_kernel`: the masked sweeps with `saturation`'s derivative fused in) are held
to what the masked kernels are held to, on the compiled gfx950 assembly (csrc/check_ring_isa.py, no GPU needed): the
prefetch of the next level is not waited for at the load site, nothing spills to scratch, and the masked kernels are still
the eight instantiations each that they were."""
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


def test_step_tl_prefetch_is_not_waited_for_at_the_load_site(tl_asm):
    assert isa.check_prefetch_distance(tl_asm, "tl_step_kernelI") == 8          # T x REG x EVAP, one level loop each
    assert isa.check_prefetch_distance(tl_asm, "tl_step_kernelIdLb1ELb0E") == 1  # what cloudsc2_step's jvp runs


def test_step_ad_prefetch_is_not_waited_for_at_the_load_site(ad_asm):
    assert isa.check_prefetch_distance(ad_asm, "ad_step_kernelI") == 8          # T x REG x FIX, one sweep each
    assert isa.check_prefetch_distance(ad_asm, "ad_step_kernelIdLb1ELb1E") == 1  # what cloudsc2_step's backward runs


def test_step_kernels_do_not_spill(tl_asm, ad_asm):
    """every instantiation, first of all the ones `cloudsc2_step` launches (LREGCL; AD_TRAJ_FIX = 1 for the adjoint)"""
    launched = [(tl_asm, "tl_step_kernelIdLb1ELb0E"), (tl_asm, "tl_step_kernelIfLb1ELb0E"),
                (ad_asm, "ad_step_kernelIdLb1ELb1E"), (ad_asm, "ad_step_kernelIfLb1ELb1E")]
    every = [(asm, name) for asm, pre in ((tl_asm, "tl_step_kernelI"), (ad_asm, "ad_step_kernelI"))
             for name, _ in isa._kernels(asm, pre)]
    assert len(every) == 16
    for asm, key in launched + every:
        assert isa.kernel_resources(asm, key)["ScratchSize"] == 0, key
    assert isa.kernel_resources(ad_asm, "ad_step_kernelIfLb1ELb1E")["Occupancy"] >= 3      # as ad_masked_kernel fp32


def test_the_kernel_families_are_told_apart_by_name(tl_asm, ad_asm):
    """eight step and still eight masked instantiations each; no step name is picked up by a prefix another check counts"""
    for asm, step, masked in ((tl_asm, "tl_step_kernelI", "tl_masked_kernelI"), (ad_asm, "ad_step_kernelI", "ad_masked_kernelI")):
        assert len([n for n, _ in isa._kernels(asm, masked)]) == 8, masked
        names = [n for n, _ in isa._kernels(asm, step)]
        assert len(names) == 8, (step, names)
        for name in names:
            assert not any(k in name for k in ("tl_kernelI", "ad_kernelI", "nl_kernelI", "tl_ring_kernelI", "masked_kernelI")), name
