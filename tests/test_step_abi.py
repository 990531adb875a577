"""Host-side contract of the derivative entries of the whole step (`cloudsc2_saturation_tl_*` / `_ad_*`, `cloudsc2_tl_step_*`
/ `cloudsc2_ad_step_*`): every argument error is settled before anything is launched, so none of this needs a GPU."""
import pytest

from abi_calls import call  # noqa: F401  (a fixture)
from abi_calls import header as _header

FAMILY = "step"
SYMBOLS = [f"cloudsc2_{n}_{s}" for n in ("saturation_tl", "saturation_ad", "tl_step", "ad_step") for s in ("f64", "f32")]


def test_the_eight_symbols_are_exported_and_declared(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import ABI_VERSION

    header = _header()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, s), s
        assert f"int32_t {s}(" in header, s
    assert _lib.SIGNATURES["cloudsc2_tl_step_f64"] == _lib.SIGNATURES["cloudsc2_tl_masked_f64"]
    assert _lib.SIGNATURES["cloudsc2_ad_step_f32"] == _lib.SIGNATURES["cloudsc2_ad_masked_f32"]
    assert len(_lib.SIGNATURES["cloudsc2_saturation_tl_f64"][1]) == 11 and len(_lib.SIGNATURES["cloudsc2_saturation_ad_f64"][1]) == 11
    assert not any(lay.entry in ("tl_step", "ad_step", "saturation_tl", "saturation_ad") for lay in _lib.LAYOUTS.values())
    assert ABI_VERSION == 4 and hip_lib.cloudsc2_abi_version() == 4          # purely additive


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_qsat_slots_must_be_null(call, sfx):
    p, P = call.params(), call.P
    assert call.tl(p, in_i=call.arr([P] * 16), sfx=sfx) == -1 and "in_i[NL_IN_QSAT]" in call.err()
    assert call.ad(p, out_adj=call.arr([P] * 16), sfx=sfx) == -1 and "out_adj[NL_IN_QSAT]" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
def test_a_null_qsat_trajectory_is_accepted_as_far_as_the_launch(call, sfx, big):
    """in[NL_IN_QSAT] == NULL passes every pointer check: the call is refused only by a later check (the field size, the
    last one before the launch), while any other NULL trajectory field is refused by name before it.  Nothing is launched
    on dummy pointers."""
    p, P = call.params(), call.P
    assert call.tl(p, nx=big, ls=big, sfx=sfx) == -2 and "4 GiB" in call.err()
    assert call.ad(p, nx=big, ls=big, sfx=sfx) == -2 and "4 GiB" in call.err()
    assert call.tl(p, nx=big, ls=big, in_=call.arr([P] * 16), sfx=sfx) == -2 and "4 GiB" in call.err()      # present: fine too
    assert call.tl(p, nx=big, ls=big, in_=call.arr([P] * 11 + [0] + [P] * 4), sfx=sfx) == -1 and "in[11]" in call.err()
    assert call.ad(p, nx=big, ls=big, in_=call.arr([0] + [P] * 15), sfx=sfx) == -1 and "in[0]" in call.err()
    # the NULL qsat perturbation needs no zero line; any other NULL perturbation does
    assert call.tl(p, nx=big, ls=big, zero=None, sfx=sfx) == -2 and "4 GiB" in call.err()
    assert call.tl(p, nx=big, ls=big, in_i=call.arr([0, 0] + [P] * 7 + [0] + [P] * 6), zero=None, sfx=sfx) == -1 and "zero_line" in call.err()
    assert call.ad(p, nx=big, ls=big, in_adj=call.arr([0] + [P] * 9), zero=None, sfx=sfx) == -1 and "zero_line" in call.err()


def test_only_the_lphylin_form_is_fused(call):
    p = call.params(LPHYLIN=False)
    assert call.tl(p) == -2 and "LPHYLIN" in call.err()
    assert call.ad(p) == -2 and "LPHYLIN" in call.err()


def test_evaporation_switches_are_unsupported_by_the_step_adjoint(call):
    assert call.ad(call.params(LEVAPLS2=True)) == -2 and "LEVAPLS2" in call.err()
    assert call.ad(call.params(LDRAIN1D=True)) == -2 and "LDRAIN1D" in call.err()


def test_required_pointers_and_outputs(call):
    p = call.params()
    assert call.tl(p, eta=None) == -1 and "eta" in call.err()
    assert call.ad(p, tl=None) == -1 and "traj_fplsl" in call.err()
    assert call.ad(p, out_adj=call.arr([0] * 16)) == -1 and "out_adj" in call.err()
    assert call.tl(p, out_i=call.arr([0] * 10)) == -1 and "out_i" in call.err()


def test_empty_calls_are_successful_no_ops(call):
    p = call.params()
    none16, none10 = call.arr([0] * 16), call.arr([0] * 10)
    assert call.tl(p, nx=0, in_=none16, in_i=none16, zero=None, eta=None, out_i=none10) == 0
    assert call.ad(p, nx=0, in_=none16, in_adj=none10, zero=None, eta=None, tl=None, tn=None, out_adj=none16) == 0
    assert call.sat_tl(p, nx=0, ap=None, t=None, ap_i=None, t_i=None, qsat=None, qsat_i=None) == 0
    assert call.sat_ad(p, nx=0, ap=None, t=None, q=None, ap_adj=None, t_adj=None) == 0


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_saturation_derivative_argument_errors(call, sfx):
    p = call.params()
    assert call.sat_tl(p, ap_i=None, t_i=None, sfx=sfx) == -1 and "ap_i" in call.err() and "t_i" in call.err()
    assert call.sat_ad(p, ap_adj=None, t_adj=None, sfx=sfx) == -1 and "ap_adj" in call.err() and "t_adj" in call.err()
    assert call.sat_tl(p, ap=None, sfx=sfx) == -1 and "ap" in call.err()
    assert call.sat_tl(p, t=None, sfx=sfx) == -1 and " t " in call.err()
    assert call.sat_tl(p, qsat_i=None, sfx=sfx) == -1 and "qsat_i" in call.err()
    assert call.sat_ad(p, q=None, sfx=sfx) == -1 and "qsat_adj" in call.err()
    assert call.sat_ad(p, nx=-1, sfx=sfx) == -1 and "nx" in call.err()


def test_cloudsc2_step_refuses_host_tensors_and_a_state_with_qsat(hip_lib):
    import torch

    import gt4py_dwarf_p_cloudsc2_tl_ad_amd as pkg
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN

    for n in ("cloudsc2_step", "saturation", "saturation_tl", "saturation_ad", "tl_step", "ad_step"):
        assert getattr(pkg, n) is getattr(autodiff, n), n
    assert autodiff.STEP_IN == tuple(n for n in NL_IN if n != "qsat")
    nx, nz = 8, 4
    full = {n: storage.zeros(nx, nz, torch.float64, "cpu") for n in NL_IN}
    state = {n: f for n, f in full.items() if n != "qsat"}
    eta = torch.zeros(nz + 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        autodiff.cloudsc2_step(state, eta, 3600.0)
    with pytest.raises(ValueError, match="`cloudsc2`"):
        autodiff.cloudsc2_step(full, eta, 3600.0)
    with pytest.raises(ValueError, match="missing"):
        autodiff.cloudsc2_step({n: f for n, f in state.items() if n != "t"}, eta, 3600.0)
    with pytest.raises(ValueError, match="GPU"):
        autodiff.saturation(state["ap"], state["t"])
    with pytest.raises(ValueError, match="GPU"):
        autodiff.saturation_tl(state["ap"], state["t"], t_i=state["q"])
    with pytest.raises(ValueError, match="GPU"):
        autodiff.saturation_ad(state["ap"], state["t"], state["q"])
    with pytest.raises(ValueError, match="nothing to propagate"):
        autodiff.saturation_tl(state["ap"], state["t"])
    with pytest.raises(ValueError, match="GPU"):
        autodiff.tl_step(state, {"t": state["t"]}, eta, 3600.0, want=("tnd_t",))
    with pytest.raises(ValueError, match="want"):
        autodiff.ad_step(state, {"tnd_t": state["t"]}, eta, 3600.0, traj={"fplsl": state["t"], "fplsn": state["q"]},
                         want=("qsat",))
