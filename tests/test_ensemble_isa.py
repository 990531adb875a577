"""The ensemble kernels (`nl_ens_kernel`, `tl_ens_kernel`, `tl_ens_step_kernel`, `ad_ens_kernel`, `ad_ens_step_kernel`) on
the compiled gfx950 assembly, checked with the project's own guard (csrc/check_ring_isa.py), no GPU needed.  Resources and
wait placement only: each family has its instantiations under names no existing check counts, nothing spills to scratch,
the prefetch of the next level is not waited for at the load site - in as many batches as the single-form twin has - and
the fp32 occupancy is no lower than the twin's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

#: family prefix -> (source, instantiations, the single-form twin's prefix)
FAMILIES = {
    "nl_ens_kernelI": ("cloudsc2_nl.hip", 16, "9nl_kernelI"),            # T x EVAP x LIN x FUSE {0, 1}
    "tl_ens_kernelI": ("cloudsc2_tl.hip", 8, "tl_masked_kernelI"),       # T x REG x EVAP
    "tl_ens_step_kernelI": ("cloudsc2_tl.hip", 8, "tl_step_kernelI"),
    "ad_ens_kernelI": ("cloudsc2_ad.hip", 8, "ad_masked_kernelI"),       # T x REG x FIX
    "ad_ens_step_kernelI": ("cloudsc2_ad.hip", 8, "ad_step_kernelI"),
}
#: the substrings the existing checks count instantiations by (check_all, tests/test_ring_isa.py, tests/test_derivative_isa.py)
COUNTED = ("9nl_kernelI", "9tl_kernelI", "9ad_kernelI", "tl_kernelI", "tl_masked_kernelI", "tl_step_kernelI", "ad_masked_kernelI",
           "ad_step_kernelI", "masked_kernelI", "tl_ring_kernelI", "nl_ring_kernelI", "tl_dirs_kernelI", "tl_dirs_step_kernelI",
           "ad_dirs_kernelI", "ad_dirs_step_kernelI", "nl_taylor_multi_kernelI")
#: (ensemble instantiation, its twin) of what `autodiff` launches with the drivers' switches, per precision: template
#: arguments <T, REG, EVAP> (TL), <T, REG, FIX> (AD, AD_TRAJ_FIX = 1), <T, EVAP, LIN, PINK, FUSE> (NL)
LAUNCHED = [
    ("cloudsc2_tl.hip", "tl_ens_kernelI{t}Lb1ELb0E", "tl_masked_kernelI{t}Lb1ELb0E"),
    ("cloudsc2_tl.hip", "tl_ens_step_kernelI{t}Lb1ELb0E", "tl_step_kernelI{t}Lb1ELb0E"),
    ("cloudsc2_ad.hip", "ad_ens_kernelI{t}Lb1ELb1E", "ad_masked_kernelI{t}Lb1ELb1E"),
    ("cloudsc2_ad.hip", "ad_ens_step_kernelI{t}Lb1ELb1E", "ad_step_kernelI{t}Lb1ELb1E"),
    ("cloudsc2_nl.hip", "nl_ens_kernelI{t}Lb0ELb1ELb{pink}ELi0E", "9nl_kernelI{t}Lb0ELb1ELb{pink}ELi0ELb0E"),
    ("cloudsc2_nl.hip", "nl_ens_kernelI{t}Lb0ELb1ELb{pink}ELi1E", "9nl_kernelI{t}Lb0ELb1ELb{pink}ELi1ELb0E"),
]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    out = str(tmp_path_factory.mktemp("isa"))
    return {src: isa.compile_to_asm(src, out) for src in ("cloudsc2_nl.hip", "cloudsc2_tl.hip", "cloudsc2_ad.hip")}


def _names(asm, prefix):
    return [n for n, _ in isa._kernels(asm, prefix)]


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_each_family_has_its_instantiations_under_names_nothing_else_counts(asm, prefix):
    src, count, _ = FAMILIES[prefix]
    names = _names(asm[src], prefix)
    assert len(names) == count and len(set(names)) == count, names
    for n in names:
        assert not any(c in n for c in COUNTED), n


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_no_scratch_and_the_prefetch_is_not_waited_for_at_the_load_site(asm, prefix):
    src, count, _ = FAMILIES[prefix]
    for n in _names(asm[src], prefix):
        assert isa.kernel_resources(asm[src], n)["ScratchSize"] == 0, (n, "spills to scratch")
        assert isa.check_prefetch_distance(asm[src], n) >= 1, (n, "level loop not seen")


@pytest.mark.parametrize("t,pink", [("d", 1), ("f", 0)])
@pytest.mark.parametrize("src,ens,twin", LAUNCHED)
def test_launched_instantiations_match_their_single_form_twins(asm, src, ens, twin, t, pink):
    ens, twin = ens.format(t=t, pink=pink), twin.format(t=t, pink=pink)
    assert len(_names(asm[src], ens)) == 1 and len(_names(asm[src], twin)) == 1, (ens, twin)
    assert isa.check_prefetch_distance(asm[src], ens) == isa.check_prefetch_distance(asm[src], twin) >= 1
    r, r0 = isa.kernel_resources(asm[src], ens), isa.kernel_resources(asm[src], twin)
    print(f"{ens}: {r}   twin {twin}: {r0}")
    assert r["ScratchSize"] == 0
    if t == "f":
        assert r["Occupancy"] >= r0["Occupancy"], (r, r0)
