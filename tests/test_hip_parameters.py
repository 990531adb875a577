"""The HIP kernels on parameter sets other than the provisional defaults (tests/param_support.py), held to the NumPy oracle
run with the same set.  tests/test_parameter_sets.py proves on the oracle alone that every comparison made here would
fail if the kernel ignored the moved parameter, read its twin (RTICE for RTICECU, ZQMAX for QMAX, RTT for RTWAT ...) or
recomputed a derived constant from the others: the set changes the expected values by more than 10 x the bound.

  * one parameter at a time, float64: `saturation` in the modes that read it, `cloudsc2_nl`, `cloudsc2_tl` with general
    increments and `cloudsc2_ad` forced with the TL output; with the evaporation block (LEVAPLS2, dt = 60 s) for the
    parameters it uses differently, and NL without LPHYLIN for those that only its foealfa reads;
  * the joint set, float64 and float32, wherever a `Cloudsc2Params` goes: NL on both memory paths, fused with saturation,
    perturbed, the Taylor reductions, `cloudsc2_tl_incremented`, `cloudsc2_ad_from_trajectory`, the masked / step / multi /
    ensemble derivative entries, `saturation_tl` / `saturation_ad`, and `autodiff.cloudsc2_step` in both modes.

Bounds are those of the default-parameter tests of the same entries (grid_support.py: `assert_close` at its default for
values, 100 x for TL outputs and adjoints; tests/test_step_grad.py: 1000 x for gradients through `cloudsc2_step`).  No
column is excluded anywhere and no bound is widened."""
import numpy as np
import pytest

from derivative_support import STEP_IN, Box, Ens, ens_nl
from grid_support import (Held, device_eta, hold_dense, hold_ensemble, hold_masked, hold_multi, hold_nl, hold_perturbed)
from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import _REAL_FIELDS
from helpers import NL_IN, NL_OUT, adjoint_nlev_of, assert_close, from_device, nlev_of, run_oracle_tl, to_device
from param_support import EVAP_PARAMS, NOLIN_PARAMS, NX, NZ, READS, SATURATION_MODES, param_case

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]


def hold_saturation(held, gpu, case, mode):
    """the stencil `saturation` in one of its three forms against the oracle's under the case's externals"""
    box = Box(case.nx, case.nz, case.dtype, gpu, False)
    out = box.nan()
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

    compile_stencil("saturation", case.ext(**SATURATION_MODES[mode]))(
        in_ap=box.put(case.fields["in_ap"]), in_t=box.put(case.fields["in_t"]), out_qsat=out, origin=(0, 0, 0),
        domain=(case.nx, 1, case.nz), validate_args=True, exec_info=None)
    held.field(f"saturation[{mode}]", from_device(out)[:case.nz], case.saturation(mode)["qsat"][:case.nz])


@pytest.mark.parametrize("param", _REAL_FIELDS)
def test_one_parameter_moved(gpu, param):
    dtype = np.float64
    held = Held(f"{param} moved", dtype)
    case = param_case(param, dtype)
    for mode in SATURATION_MODES:
        if param in READS[f"saturation[{mode}]"]:
            hold_saturation(held, gpu, case, mode)
    if param in READS["nl"]:
        hold_nl(held, gpu, case, NX, "ring")
        hold_nl(held, gpu, case, NX, "prefetch")
        hold_dense(held, gpu, case, NX, fix=1)        # every column the liveness proof used, the planted ones included
    if param in EVAP_PARAMS:
        evap = param_case(param, dtype, "evap")
        hold_nl(held, gpu, evap, NX, "ring")
        hold_dense(held, gpu, evap, NX, fix=1)
    if param in NOLIN_PARAMS:
        hold_nl(held, gpu, param_case(param, dtype, "nolin"), NX, "ring")
    held.done()


# ----------------------------------------------------------------------------------------------
# the joint sets
# ----------------------------------------------------------------------------------------------
JOINT = pytest.mark.parametrize("name", ["joint", "joint_opposite"])


@pytest.mark.parametrize("dtype", DTYPES)
@JOINT
def test_joint_set_saturation_and_nl_paths(gpu, name, dtype):
    """`saturation` in its three forms; `cloudsc2_nl` on the LDS ring (whole waves, a ragged wave) and on the
    register-prefetch path (the column-1 window of wider storages); `cloudsc2_nl_saturation` on both; NL with the
    evaporation block and without LPHYLIN"""
    case = param_case(name, dtype, own_qsat=True)
    held = Held(f"{name} nl", dtype)
    for mode in SATURATION_MODES:
        hold_saturation(held, gpu, case, mode)
    hold_nl(held, gpu, case, 64, "ring")
    hold_nl(held, gpu, case, NX, "ring")
    hold_nl(held, gpu, case, NX, "prefetch")
    hold_nl(held, gpu, case, 64, "fused")
    hold_nl(held, gpu, case, NX, "fused prefetch")
    for switches in ("evap", "nolin"):
        other = param_case(name, dtype, switches, own_qsat=True)
        hold_nl(held, gpu, other, NX, "ring")
        hold_nl(held, gpu, other, NX, "prefetch")
    held.done()


def _general_increments(case):
    rng = np.random.default_rng(17)
    return {k + "_i": (v * rng.uniform(-0.02, 0.02, size=v.shape)).astype(v.dtype) for k, v in case.fields.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@JOINT
def test_joint_set_perturbed_and_taylor_kernels(gpu, name, dtype):
    """`cloudsc2_nl_perturbed`, `cloudsc2_nl_taylor` and `cloudsc2_nl_taylor_multi` against the oracle's separate calls"""
    case = param_case(name, dtype, own_qsat=True)
    held = Held(f"{name} perturbed", dtype)
    hold_perturbed(held, gpu, case, _general_increments(case), (1.0, 0.5, 1e-2))
    held.done()


@pytest.mark.parametrize("dtype", DTYPES)
@JOINT
def test_joint_set_tl_incremented(gpu, name, dtype):
    """`cloudsc2_tl_incremented` (state_increment inside the TL kernel) against the oracle's state_increment + cloudsc2_tl"""
    from helpers import increments

    case = param_case(name, dtype, own_qsat=True)
    nx, nz, f1 = case.nx, case.nz, 0.01
    ext = case.ext()
    want_nl, want_tl = run_oracle_tl(case.fields, increments(case.fields, f1), case.eta, case.dt, ext)
    box = Box(nx, nz, dtype, gpu, False)
    out, out_i = {n: box.nan() for n in NL_OUT}, {n: box.nan() for n in NL_OUT}
    box.stencil("cloudsc2_tl_incremented", ext, device_eta(gpu, case.eta), case.dt, f=f1,
                **{"in_" + n: f for n, f in box.state(case.fields).items()}, **{"out_" + n: f for n, f in out.items()},
                **{"out_" + n + "_i": f for n, f in out_i.items()})
    held = Held(f"{name} tl_incremented", dtype)
    held.fields("tl_incremented out", out, want_nl, NL_OUT, nlev_of, nz, nx)
    held.fields("tl_incremented out_i", out_i, want_tl, NL_OUT, nlev_of, nz, nx, 100.0)
    held.done()


@pytest.mark.parametrize("dtype", DTYPES)
@JOINT
def test_joint_set_derivative_kernels(gpu, name, dtype):
    """`cloudsc2_tl` on its LDS ring and its register path, `cloudsc2_ad`, `cloudsc2_ad_from_trajectory` (AD_TRAJ_FIX = 1);
    `tl_masked` / `ad_masked`, `tl_step` / `ad_step`, `tl_multi` / `ad_multi` at 2 directions, the 2-member ensemble entries
    `cloudsc2_{nl,tl,ad}_ens`; TL / AD with the evaporation block"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    case = param_case(name, dtype, own_qsat=True)
    held = Held(f"{name} derivatives", dtype)
    hold_dense(held, gpu, case, 64, fix=0)
    hold_dense(held, gpu, case, NX, fix=1)
    box = Box(NX, NZ, dtype, gpu, False)
    ext, eta = case.ext(AD_TRAJ_FIX=1), device_eta(gpu, case.eta)
    st = box.state(case.fields)
    forcing = {n: box.put(case.tl(0)[n]) for n in NL_OUT}
    traj = {n: box.put(case.nl()[n]) for n in ("fplsl", "fplsn")}
    adj = box.dense_ad_traj(st, forcing, traj, ext, eta, case.dt)
    assert _lib.last_kernel() == "cs2::ad_kernel<trajectory>", _lib.last_kernel()
    held.fields("ad_from_trajectory", adj, case.ad(0, 1), NL_IN, adjoint_nlev_of, NZ, NX, 100.0)
    hold_masked(held, gpu, case, NX, step=False)
    hold_masked(held, gpu, case, NX, step=True)
    hold_multi(held, gpu, case, NX, ndir=2)
    hold_ensemble(held, gpu, case, NX)
    evap = param_case(name, dtype, "evap", own_qsat=True)
    hold_dense(held, gpu, evap, 64, fix=1)
    hold_dense(held, gpu, evap, NX, fix=1)
    hold_masked(held, gpu, evap, NX, step=False)
    held.done()


@pytest.mark.parametrize("dtype", DTYPES)
@JOINT
def test_joint_set_fused_ensemble_nl(gpu, name, dtype):
    """`cloudsc2_nl_fused_ens` on two members (the columns, and the columns in reverse order): outputs and qsat"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    case = param_case(name, dtype, own_qsat=True)
    ens = Ens(Box(NX, NZ, dtype, gpu, False), 2, 0)
    both = lambda a: [a, np.ascontiguousarray(a[:, ::-1])]  # noqa: E731
    state = {n: ens.put(both(case.fields["in_" + n])) for n in NL_IN if n != "qsat"}
    out, qsat = {n: ens.nan() for n in NL_OUT}, ens.nan()
    ens_nl(ens, case.ext(), state, device_eta(gpu, case.eta), case.dt, out, qsat)
    assert _lib.last_kernel() == "cs2::nl_ens_kernel<saturation>", _lib.last_kernel()
    held = Held(f"{name} nl_fused_ens", dtype)
    for m in range(2):
        held.fields(f"nl_fused_ens[{m}]", {n: f[m] for n, f in out.items()}, case.nl(), NL_OUT, nlev_of, NZ, NX,
                    reversed_columns=m == 1)
        held.fields(f"nl_fused_ens[{m}]", {"qsat": qsat[m]}, {"qsat": case.fields["in_qsat"]}, ("qsat",), nlev_of, NZ, NX,
                    reversed_columns=m == 1)
    held.done()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", list(SATURATION_MODES))
@JOINT
def test_joint_set_saturation_derivatives(gpu, name, mode, dtype):
    """`saturation_tl` / `saturation_ad` against the analytic derivative of the reference's formula under the set, at
    `assert_close`'s default as tests/test_saturation_grad.py holds them"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff
    from saturation_oracle import saturation_derivative

    case = param_case(name, dtype, own_qsat=True)
    ext = case.ext(**SATURATION_MODES[mode])
    ap, t = case.fields["in_ap"], case.fields["in_t"]
    _, g_t, g_ap, clipped = saturation_derivative(ap, t, ext)
    assert (g_t[:NZ] != 0).any() and not clipped[:NZ].all()
    rng = np.random.default_rng(11)
    t_i = rng.standard_normal(t.shape).astype(dtype)
    ap_i = (0.01 * ap * rng.standard_normal(t.shape)).astype(dtype)
    q_adj = rng.standard_normal(t.shape).astype(dtype)
    dev = to_device(dict(ap=ap, t=t, ap_i=ap_i, t_i=t_i, q_adj=q_adj), gpu)
    qsat, qsat_i = autodiff.saturation_tl(dev["ap"], dev["t"], dev["ap_i"], dev["t_i"], ext, write_qsat=True)
    assert _lib.last_kernel() == "cs2::saturation_tl_kernel"
    adj = autodiff.saturation_ad(dev["ap"], dev["t"], dev["q_adj"], ext)
    assert _lib.last_kernel() == "cs2::saturation_ad_kernel"
    assert_close("qsat", from_device(qsat)[:NZ], case.saturation(mode)["qsat"][:NZ], dtype)
    want_i = g_t * t_i.astype(np.float64) + g_ap * ap_i.astype(np.float64)
    assert_close("qsat_i", from_device(qsat_i)[:NZ], want_i[:NZ].astype(dtype), dtype)
    for n, g in (("ap", g_ap), ("t", g_t)):
        assert_close(n + "_adj", from_device(adj[n])[:NZ], (g * q_adj.astype(np.float64))[:NZ].astype(dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@JOINT
def test_joint_set_through_autodiff_step(gpu, name, dtype):
    """`autodiff.cloudsc2_step` with the set as its externals: backward mode gives the oracle's adjoint of the step and
    forward mode its TL - the Python layer carries the externals into the forward launch, `ad_step` and `tl_step`"""
    import torch
    import torch.autograd.forward_ad as fwad

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, cloudsc2_step

    case = param_case(name, dtype, own_qsat=True)
    ext = {k: v for k, v in case.ext().items() if k != "NLEV"}
    dev = to_device(case.fields, gpu)
    eta = device_eta(gpu, case.eta)
    names = ("t", "q", "ap")
    state = {n: dev["in_" + n] for n in STEP_IN}
    for n in names:
        state[n].requires_grad_(True)
    forcing = to_device({n: case.tl(0)[n] for n in NL_OUT}, gpu)
    out = cloudsc2_step(state, eta, case.dt, ext)
    held = Held(f"{name} cloudsc2_step", dtype)
    held.fields("step forward", {n: out[n].detach() for n in NL_OUT}, case.nl(), NL_OUT, nlev_of, NZ, NX, padding_nan=False)
    held.field("step qsat", from_device(out["qsat"].detach())[:NZ], case.fields["in_qsat"][:NZ])
    grads = torch.autograd.grad([out[n] for n in NL_OUT], [state[n] for n in names], [forcing[n] for n in NL_OUT])
    assert _lib.last_kernel() == "cs2::ad_step_kernel", _lib.last_kernel()
    want = case.ad(0, 1, step=True)
    for n, g in zip(names, grads):
        held.field(f"step grad {n}", from_device(g)[:NZ], want[n][:NZ], 1000.0)
    u = {n: case.dirs[0][n] for n in STEP_IN}
    h = to_device(u, gpu)
    with fwad.dual_level():
        dual = {n: fwad.make_dual(state[n].detach(), h[n]) for n in STEP_IN}
        tangents = {n: fwad.unpack_dual(v).tangent.clone() for n, v in cloudsc2_step(dual, eta, case.dt, ext).items() if n in NL_OUT}
    assert _lib.last_kernel() == "cs2::tl_step_kernel", _lib.last_kernel()
    held.fields("step jvp", tangents, case.tl(0, True), NL_OUT, nlev_of, NZ, NX, 100.0, padding_nan=False)
    held.done()
