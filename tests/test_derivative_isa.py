"""The derivative kernels on the compiled gfx950 assembly, checked with the project's own guard (csrc/check_ring_isa.py), no
GPU needed.  `cloudsc2_tl.hip` and `cloudsc2_ad.hip` are compiled once each for all of these tests.

masked (`tl_masked_kernel`, `ad_masked_kernel`): they keep the register path's one level of prefetch only if hipcc still
counts their loads: every load is issued unconditionally (an absent field reads the zero line), so the wait for a level's
words must not come at the load site.

step (`tl_step_kernel`, `ad_step_kernel`: the masked sweeps with `saturation`'s derivative fused in): held to what the
masked kernels are held to: the prefetch of the next level is not waited for at the load site, nothing spills to scratch,
and the masked kernels are still the eight instantiations each that they were.

multi-direction (`tl_dirs_kernel`, `tl_dirs_step_kernel`, `ad_dirs_kernel`, `ad_dirs_step_kernel`): eight instantiations
each under names no other check counts, the families that were there are what they were, nothing spills to scratch, and no
prefetch is waited for at its load site.

`check_prefetch_distance` judges every batch of >= 14 loads inside a loop of >= 600 lines by the first wait that reaches
into it, in program order.
  * The multi-direction TL kernels have two such batches: the next LEVEL's state words (outer loop) and the next
    DIRECTION's perturbation words (inner loop, which is itself that long).  The helper expresses both; it does not tell
    which of the two a batch is, so what is asserted is the number of batches seen: two in the instantiations `tl_multi` /
    `tl_step_multi` launch with the drivers' switches, at least one in every other (hipcc may split a batch of one of the
    evaporation instantiations below the helper's threshold).  Left unchecked: that the five carry words per direction are
    the only LDS traffic of the direction loop.
  * The LEVEL batch of the multi-direction AD kernels (15 or 16 state words, `aph` and the two trajectory flux words of the
    next level) is such a batch; it is issued in front of ad_forward and first waited for behind the first direction's
    ad_backward.  Left unchecked: the per-DIRECTION forcing batch is at most nine loads, below the helper's threshold of
    14, so whether the next direction's forcing is waited for early is not seen by this test.  No occupancy figure is
    asserted for them either; docs/TUNING_LOG.md 3.19 records what hipcc gave."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

#: multi-direction family -> (the prefixes its own instantiations are counted by, the substrings the checks of the other
#: families - dense, masked, step and ring, here, in tests/test_ring_isa.py and in check_all - count instantiations by)
PREFIXES = {
    "tl_dirs": (("tl_dirs_kernelI", "tl_dirs_step_kernelI"),
                ("tl_kernelI", "tl_masked_kernelI", "tl_step_kernelI", "masked_kernelI", "tl_ring_kernelI")),
    "ad_dirs": (("ad_dirs_kernelI", "ad_dirs_step_kernelI"),
                ("9ad_kernelI", "ad_masked_kernelI", "ad_step_kernelI", "masked_kernelI")),
}


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


def _names(asm, family):
    return [n for n, _ in isa._kernels(asm, family)]


# ---- masked -----------------------------------------------------------------------------------------------------------------
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


# ---- step -------------------------------------------------------------------------------------------------------------------
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


# ---- multi-direction tangent-linear -----------------------------------------------------------------------------------------
def test_tl_dirs_eight_instantiations_per_family_under_names_nobody_else_counts(tl_asm):
    FAMILIES, COUNTED_ELSEWHERE = PREFIXES["tl_dirs"]
    for family in FAMILIES:
        names = _names(tl_asm, family)
        assert len(names) == 8, (family, names)            # T x REG x EVAP
        for name in names:
            assert not any(k in name for k in COUNTED_ELSEWHERE), name
    assert not set(_names(tl_asm, FAMILIES[0])) & set(_names(tl_asm, FAMILIES[1]))
    # ... and the families that were there are the eight instantiations each that they were
    for family in ("tl_masked_kernelI", "tl_step_kernelI", "tl_ring_kernelI"):
        assert len(_names(tl_asm, family)) == 8, family


def test_tl_dirs_no_instantiation_spills(tl_asm):
    FAMILIES, _ = PREFIXES["tl_dirs"]
    for family in FAMILIES:
        for name in _names(tl_asm, family):
            assert isa.kernel_resources(tl_asm, name)["ScratchSize"] == 0, name


def test_fp32_keeps_two_waves_per_simd(tl_asm):
    """what the LDS budget of the launcher assumes: at most 3 workgroups of 40 KB carry + level table per CU"""
    FAMILIES, _ = PREFIXES["tl_dirs"]
    for family in FAMILIES:
        assert isa.kernel_resources(tl_asm, family + "fLb1ELb0E")["Occupancy"] >= 2


def test_prefetches_are_not_waited_for_at_the_load_site(tl_asm):
    FAMILIES, _ = PREFIXES["tl_dirs"]
    for family in FAMILIES:
        for name in _names(tl_asm, family):
            assert isa.check_prefetch_distance(tl_asm, name) >= 1, name
        for t in "df":                                     # LREGCL, no evaporation: what the derivative rules launch
            assert isa.check_prefetch_distance(tl_asm, f"{family}{t}Lb1ELb0E") == 2, (family, t)


# ---- multi-direction adjoint ------------------------------------------------------------------------------------------------
def test_ad_dirs_eight_instantiations_per_family_under_names_nobody_else_counts(ad_asm):
    FAMILIES, COUNTED_ELSEWHERE = PREFIXES["ad_dirs"]
    for family in FAMILIES:
        names = _names(ad_asm, family)
        assert len(names) == 8, (family, names)            # T x REG x FIX
        for name in names:
            assert not any(k in name for k in COUNTED_ELSEWHERE), name
    assert not set(_names(ad_asm, FAMILIES[0])) & set(_names(ad_asm, FAMILIES[1]))
    # ... and the families that were there are the eight instantiations each that they were
    for family in ("ad_masked_kernelI", "ad_step_kernelI"):
        assert len(_names(ad_asm, family)) == 8, family


def test_ad_dirs_no_instantiation_spills(ad_asm):
    FAMILIES, _ = PREFIXES["ad_dirs"]
    seen = 0
    for family in FAMILIES:
        for name in _names(ad_asm, family):
            assert isa.kernel_resources(ad_asm, name)["ScratchSize"] == 0, name
            seen += 1
    assert seen == 16


def test_the_level_prefetch_is_not_waited_for_at_the_load_site(ad_asm):
    FAMILIES, _ = PREFIXES["ad_dirs"]
    for family in FAMILIES:
        for name in _names(ad_asm, family):
            assert isa.check_prefetch_distance(ad_asm, name) >= 1, name
