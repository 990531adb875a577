"""The members-times-directions adjoint kernels (`ad_mdirs_kernel`, `ad_mdirs_step_kernel`) on the compiled gfx950 assembly,
checked with the project's own guard (csrc/check_ring_isa.py), no GPU needed.  Resources and wait placement only: each
kernel has its eight instantiations under names no existing check counts, nothing spills to scratch, the prefetch of the
next level is not waited for at the load site - in as many batches as the `ad_dirs_*` twin has - and neither the VGPR count
nor the fp32 occupancy is worse than the twin's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402
import test_derivative_isa  # noqa: E402
import test_ensemble_isa  # noqa: E402
import test_evap_ensemble_isa  # noqa: E402

#: family prefix -> the single-ensemble twin's prefix
FAMILIES = {"ad_mdirs_kernelI": "ad_dirs_kernelI", "ad_mdirs_step_kernelI": "ad_dirs_step_kernelI"}
#: the substrings the existing checks count instantiations by: the lists of the other ISA test modules themselves
COUNTED = tuple(sorted(set(test_ensemble_isa.COUNTED) | set(test_ensemble_isa.FAMILIES) | set(test_evap_ensemble_isa.COUNTED)
                       | set(test_evap_ensemble_isa.FAMILIES)
                       | {k for own, others in test_derivative_isa.PREFIXES.values() for k in own + others}))
FLAGS = [f"Lb{reg}ELb{fix}E" for reg in (0, 1) for fix in (0, 1)]     # REG x FIX


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    return isa.compile_to_asm("cloudsc2_ad.hip", str(tmp_path_factory.mktemp("isa")))


def _names(asm, prefix):
    return [n for n, _ in isa._kernels(asm, prefix)]


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_eight_instantiations_under_names_nothing_else_counts(asm, prefix):
    names = _names(asm, prefix)
    assert len(names) == 8 and len(set(names)) == 8, names          # T x REG x FIX
    for n in names:
        assert not any(c in n for c in COUNTED), n
    assert len(_names(asm, FAMILIES[prefix])) == 8                  # the twin is what it was


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_nothing_spills_and_the_prefetch_is_not_waited_for_at_the_load_site(asm, prefix):
    names = _names(asm, prefix)
    assert len(names) == 8, names
    for n in names:
        assert isa.kernel_resources(asm, n)["ScratchSize"] == 0, (n, "spills to scratch")
        assert isa.check_prefetch_distance(asm, n) >= 1, (n, "level loop not seen")


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("t", ["d", "f"])
@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_every_instantiation_matches_its_twin(asm, prefix, t, flags):
    ens, twin = prefix + t + flags, FAMILIES[prefix] + t + flags
    assert len(_names(asm, ens)) == 1 and len(_names(asm, twin)) == 1, (ens, twin)
    assert isa.check_prefetch_distance(asm, ens) == isa.check_prefetch_distance(asm, twin) >= 1
    r, r0 = isa.kernel_resources(asm, ens), isa.kernel_resources(asm, twin)
    print(f"{ens}: {r}   twin {twin}: {r0}")
    assert r["ScratchSize"] == 0
    assert r["NumVgprs"] <= r0["NumVgprs"], (r, r0)
    if t == "f":
        assert r["Occupancy"] >= r0["Occupancy"], (r, r0)
