"""The ensemble forms of the cover kernels (`ad_cover_ens_kernel`, `ad_cover_ens_step_kernel`) on the compiled gfx950 assembly,
from the resource metadata hipcc writes behind each kernel (csrc/check_ring_isa.py's reader; no GPU): each family has its
eight instantiations under names no existing check counts, none uses scratch, and each keeps the occupancy of its
single-member counterpart - `ad_cover_kernel` / `ad_cover_step_kernel` with the same template arguments, read from the same
build, so no register count is written down here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

#: family prefix -> the single-member counterpart's prefix
FAMILIES = {"ad_cover_ens_kernelI": "ad_cover_kernelI", "ad_cover_ens_step_kernelI": "ad_cover_step_kernelI"}
#: the substrings the existing checks count the kernels of this unit and of cloudsc2_ad.hip by (tests/test_evap_adjoint_isa.py)
COUNTED = ("ad_cover_kernelI", "ad_cover_step_kernelI", "ad_cover_dirs_kernelI", "ad_cover_dirs_step_kernelI", "9ad_kernelI",
           "ad_masked_kernelI", "ad_step_kernelI", "masked_kernelI", "ad_dirs_kernelI", "ad_dirs_step_kernelI", "ad_ens_kernelI",
           "ad_ens_step_kernelI", "tl_kernelI", "nl_kernelI")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    return isa.compile_to_asm("cloudsc2_ad_evap.hip", str(tmp_path_factory.mktemp("isa")))


def _names(asm, prefix):
    return [n for n, _ in isa._kernels(asm, prefix)]


def _pairs(asm, family):
    """(ensemble instantiation, its single-member counterpart): the same <T, REG, FIX>"""
    for name in _names(asm, family):
        args = name[name.index(family) + len(family):].split("EEvNS")[0]        # e.g. dLb1ELb0
        twins = _names(asm, FAMILIES[family] + args + "EEvNS")
        assert len(twins) == 1, (name, twins)
        yield name, twins[0]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_eight_instantiations_under_names_nothing_else_counts(asm, family):
    names = _names(asm, family)
    assert len(names) == 8 and len(set(names)) == 8, names          # T x REG x FIX
    for t in "df":
        assert len(_names(asm, family + t)) == 4, (family, t)
    for n in names:
        assert not any(c in n for c in COUNTED), n


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_no_scratch_and_the_occupancy_of_the_single_member_counterpart(asm, family):
    pairs = list(_pairs(asm, family))
    assert len(pairs) == 8
    for name, twin in pairs:
        r, r0 = isa.kernel_resources(asm, name), isa.kernel_resources(asm, twin)
        print(f"{name}: {r}   counterpart: {r0}")
        assert r["ScratchSize"] == 0, (name, "uses scratch", r)
        assert r["Occupancy"] >= r0["Occupancy"], (name, r, r0)
