"""Host-side contract of the masked TL / AD entries (`cloudsc2_tl_masked_*`, `cloudsc2_ad_masked_*`): every argument error
is settled before anything is launched, so none of this needs a GPU."""
import ctypes

import pytest

from abi_calls import call  # noqa: F401  (a fixture)

FAMILY = "masked"


def test_abi_version_is_4(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import ABI_VERSION

    assert ABI_VERSION == 4 and hip_lib.cloudsc2_abi_version() == 4


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_null_required_pointers_are_argument_errors(call, sfx):
    p, P = call.params(), call.P
    assert call.tl(p, in_=call.arr([P] * 7 + [0] + [P] * 8), sfx=sfx) == -1 and "in[7]" in call.err()
    assert call.ad(p, in_=call.arr([0] + [P] * 15), sfx=sfx) == -1 and "in[0]" in call.err()
    assert call.tl(p, eta=None, sfx=sfx) == -1 and "eta" in call.err()
    assert call.ad(p, eta=None, sfx=sfx) == -1
    assert call.ad(p, tl=None, sfx=sfx) == -1 and "traj_fplsl" in call.err()
    assert call.ad(p, tn=None, sfx=sfx) == -1
    assert call.tl(p, in_i=ctypes.POINTER(ctypes.c_void_p)(), sfx=sfx) == -1 and "in_i" in call.err()


def test_all_null_outputs_are_an_argument_error(call):
    p = call.params()
    assert call.ad(p, out_adj=call.arr([0] * 16)) == -1 and "out_adj" in call.err()
    assert call.tl(p, out_i=call.arr([0] * 10)) == -1 and "out_i" in call.err()


def test_null_input_entry_needs_the_zero_line(call):
    p, P = call.params(), call.P
    assert call.ad(p, in_adj=call.arr([0] + [P] * 9), zero=None) == -1 and "zero_line" in call.err()
    assert call.tl(p, in_i=call.arr([P] * 15 + [0]), zero=None) == -1 and "zero_line" in call.err()
    assert call.tl(p, in_i=call.arr([P] * 15 + [0]), zero=P + 8) == -1 and "aligned" in call.err()


def test_partially_null_nl_outputs_are_an_argument_error(call):
    p, P = call.params(), call.P
    assert call.tl(p, out=call.arr([P] * 4 + [0] + [P] * 5)) == -1 and "out" in call.err()


def test_evaporation_switches_are_unsupported_by_the_masked_adjoint(call):
    assert call.ad(call.params(LEVAPLS2=True)) == -2 and "LEVAPLS2" in call.err()
    assert call.ad(call.params(LDRAIN1D=True)) == -2


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
def test_fields_of_4_gib_are_refused_by_name(call, sfx, big):
    p = call.params()
    assert call.tl(p, nx=big, ls=big, sfx=sfx) == -2 and "4 GiB" in call.err()
    assert call.ad(p, nx=big, ls=big, sfx=sfx) == -2 and "4 GiB" in call.err()


def test_empty_call_is_a_successful_no_op(call):
    p = call.params()
    none16, none10 = call.arr([0] * 16), call.arr([0] * 10)
    assert call.tl(p, nx=0, in_=none16, in_i=none16, zero=None, eta=None, out_i=none10) == 0
    assert call.ad(p, nx=0, in_=none16, in_adj=none10, zero=None, eta=None, tl=None, tn=None, out_adj=none16) == 0


def test_autodiff_refuses_host_tensors(hip_lib):
    import torch

    import gt4py_dwarf_p_cloudsc2_tl_ad_amd as pkg
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN

    assert pkg.cloudsc2 is autodiff.cloudsc2 and pkg.tl_masked is autodiff.tl_masked and pkg.ad_masked is autodiff.ad_masked
    nx, nz = 8, 4
    state = {n: storage.zeros(nx, nz, torch.float64, "cpu") for n in NL_IN}
    eta = torch.zeros(nz + 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        autodiff.tl_masked(state, {"t": state["t"]}, eta, 3600.0, want=("tnd_t",))
    with pytest.raises(ValueError, match="GPU"):
        autodiff.ad_masked(state, {"tnd_t": state["t"]}, eta, 3600.0, traj={"fplsl": state["t"], "fplsn": state["q"]},
                           want=("t",))
    with pytest.raises(ValueError, match="GPU"):
        autodiff.cloudsc2(state, eta, 3600.0)
