"""`autodiff.cloudsc2_step`: the step `saturation` + `cloudsc2_nl` with its TOTAL derivative.  Expected values are composed
on the CPU from pieces that exist: the oracle's `saturation` and TL / AD of `cloudsc2` (tests/helpers.py), chained with the
analytic derivative of `saturation` (tests/saturation_oracle.py).  Reverse mode must be ONE `ad_step_kernel` launch whose
`t` gradient contains the path through `qsat`; forward mode one `tl_step_kernel` launch; the two are transposes.

Tolerances are the ones the suite already holds these kernels to: 1000 x `assert_close` for adjoints and 100 x for TL
perturbations against the oracle (tests/test_autodiff.py), 100 x where two kernels contract the same level function
differently (tests/test_hip_masked.py), |norm1 - norm2| / (eps norm2) < 1e4 per column for the transpose identity."""
import numpy as np
import pytest

from derivative_support import STEP_IN, autodiff_case as _case, device_state
from helpers import NL_OUT, assert_close, externals, from_device, increments, nlev_of, run_oracle_ad, run_oracle_tl, to_device

pytestmark = pytest.mark.gpu
NX, NZ = 200, 137          # `autodiff_case`'s own


def _state(gpu, c, grad=()):
    return device_state(gpu, c, STEP_IN, grad)


def _forcing(c, **given):
    return {n: given.get(n, np.zeros_like(c["w"])) for n in NL_OUT}


def _total(c, adj):
    """the oracle's adjoint of cloudsc2 chained with saturation's derivative: (t, ap, the chain term of t)"""
    chain_t = c["g_t"] * adj["qsat"].astype(np.float64)
    chain_ap = c["g_ap"] * adj["qsat"].astype(np.float64)
    return adj["t"].astype(np.float64) + chain_t, adj["ap"].astype(np.float64) + chain_ap, chain_t


@pytest.mark.parametrize("nx", [NX, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_backward_is_one_step_launch_and_equals_the_composed_oracle(gpu, dtype, nx):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, cloudsc2, cloudsc2_step

    c = _case(dtype, nx)
    state, eta, dt, w = _state(gpu, c, grad=("t", "q", "ap", "tnd_cml_t"))
    out = cloudsc2_step(state, eta, dt, externals())
    assert not out["qsat"].requires_grad and out["tnd_t"].requires_grad
    (out["tnd_t"].sum() + (out["fplsl"] * w).sum()).backward()
    assert _lib.last_kernel() == "cs2::ad_step_kernel"
    # the partial derivative at fixed qsat: `cloudsc2` on the same state with the step's own qsat
    # (fresh storages of the same layout: `clone()` of a field with a padded level pitch would pack it)
    part = dict(_state(gpu, c, grad=("t", "q", "ap", "tnd_cml_t"))[0], qsat=out["qsat"].detach())
    pout = cloudsc2(part, eta, dt, externals())
    (pout["tnd_t"].sum() + (pout["fplsl"] * w).sum()).backward()
    assert _lib.last_kernel() == "cs2::ad_masked_kernel"
    torch.cuda.synchronize()
    forcing = _forcing(c, tnd_t=np.ones_like(c["w"]), fplsl=c["w"].copy())
    _, adj = run_oracle_ad(c["fields"], forcing, c["eta"], dt, externals(NLEV=NZ, AD_TRAJ_FIX=1), traj=c["nl0"])
    want_t, want_ap, chain_t = _total(c, adj)
    got = {n: from_device(state[n].grad) for n in ("t", "q", "ap", "tnd_cml_t")}
    assert_close("grad t", got["t"][:NZ], want_t[:NZ].astype(dtype), dtype, rtol_mul=1000.0)
    assert_close("grad ap", got["ap"][:NZ], want_ap[:NZ].astype(dtype), dtype, rtol_mul=1000.0)
    assert_close("grad q", got["q"][:NZ], adj["q"][:NZ], dtype, rtol_mul=1000.0)
    # the path through qsat is there: total - partial is the chain term.  The oracle's chain term is non-zero in EVERY
    # column but not in more than half of the POINTS: qsat only acts where cloud forms, and for this loss the oracle gives
    # 18.6 % of the points at 200 columns (13.9 % in the single column) - measured on the CPU oracle, asserted here as > 10 %.
    assert (chain_t[:NZ] != 0).any(axis=0).all() and (chain_t[:NZ] != 0).mean() > 0.1, float((chain_t[:NZ] != 0).mean())
    diff = got["t"].astype(np.float64) - from_device(part["t"].grad).astype(np.float64)
    assert_close("grad t, total - partial", diff[:NZ].astype(dtype), chain_t[:NZ].astype(dtype), dtype,
                 scale=float(np.abs(want_t).max()), rtol_mul=1000.0)
    # a fold that is silently missing leaves diff == 0, an error of exactly max |chain| - which the float32 bound above
    # (0.05 of the field's scale + 0.5 |chain|) would let pass in the single column
    assert np.abs(diff - chain_t)[:NZ].max() < 0.5 * np.abs(chain_t).max()
    # ... and it is folded into the t store only: tnd_cml_t stays dt x the t adjoint of cloudsc2 itself
    assert np.array_equal(got["tnd_cml_t"][:NZ], from_device(part["tnd_cml_t"].grad)[:NZ])
    assert not got["t"][NZ:].any() and not got["ap"][NZ:].any()


def _tangent_case(c):
    """1 % perturbations of t, ap, q and the oracle's TL outputs for them with qsat_i = g_t t_i + g_ap ap_i"""
    if "tl" not in c:
        fi = increments(c["fields"], 0.01)
        u = {n: fi["in_" + n + "_i"] for n in ("t", "ap", "q")}
        pert = {k: np.zeros_like(v) for k, v in fi.items()}
        pert.update({"in_" + n + "_i": v for n, v in u.items()})
        pert["in_qsat_i"] = (c["g_t"] * u["t"].astype(np.float64) + c["g_ap"] * u["ap"].astype(np.float64)).astype(u["t"].dtype)
        c["u"], c["tl"] = u, run_oracle_tl(c["fields"], pert, c["eta"], c["dt"], dict(c["ext"], NLEV=NZ))[1]
    return c["u"], c["tl"]


def _jvp(gpu, c, state, eta, dt, u, ext=None):
    import torch.autograd.forward_ad as fwad

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import cloudsc2_step

    h = to_device(u, gpu)
    with fwad.dual_level():
        dual = dict(state, **{n: fwad.make_dual(state[n].detach(), h[n]) for n in u})
        out = cloudsc2_step(dual, eta, dt, ext)
        tangents = {n: fwad.unpack_dual(out[n]).tangent for n in NL_OUT}
        assert fwad.unpack_dual(out["qsat"]).tangent is None
    return {n: t.clone() for n, t in tangents.items()}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_forward_mode_is_one_step_launch_and_equals_the_composed_tl(gpu, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    c = _case(dtype)
    u, want_i = _tangent_case(c)
    state, eta, dt, _ = _state(gpu, c)
    tangents = _jvp(gpu, c, state, eta, dt, u)
    assert _lib.last_kernel() == "cs2::tl_step_kernel"
    torch.cuda.synchronize()
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        assert_close(f"jvp out_{n}", from_device(tangents[n])[:k], want_i[n][:k], dtype, rtol_mul=100.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_vjp_is_the_transpose_of_jvp(gpu, dtype):
    """<J u, w> == <u, J^T w> per column, u on t, ap, q and w = J u on all ten outputs: |norm1 - norm2| / (eps norm2) < 1e4"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import cloudsc2_step

    c = _case(dtype)
    u, _ = _tangent_case(c)
    state, eta, dt, _ = _state(gpu, c, grad=tuple(u))
    jv = _jvp(gpu, c, state, eta, dt, u)
    out = cloudsc2_step(state, eta, dt)
    grads = torch.autograd.grad([out[n] for n in NL_OUT], [state[n] for n in u], [jv[n] for n in NL_OUT])
    torch.cuda.synchronize()
    norm1 = sum((from_device(jv[n]).astype(np.float64)[:nlev_of(n, NZ)] ** 2).sum(axis=0) for n in NL_OUT)
    norm2 = sum((u[n].astype(np.float64)[:NZ] * from_device(g).astype(np.float64)[:NZ]).sum(axis=0) for n, g in zip(u, grads))
    assert (norm2 != 0).all()
    norm3 = np.abs(norm1 - norm2) / (np.finfo(dtype).eps * np.abs(norm2))
    print(f"step vjp/jvp identity {np.dtype(dtype).name}: max {norm3.max():.3e} x eps")
    assert (norm3 < 1e4).all(), float(norm3.max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_launches_equal_the_unfused_composition(gpu, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    c = _case(dtype)
    u, tl_i = _tangent_case(c)
    state, eta, dt, w = _state(gpu, c)
    ext = externals(NLEV=NZ, AD_TRAJ_FIX=1)
    # tangent-linear: tl_step against saturation_tl + tl_masked
    pert = to_device(u, gpu)
    nl, fused_i = autodiff.tl_step(state, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    assert _lib.last_kernel() == "cs2::tl_step_kernel"
    qsat, qsat_i = autodiff.saturation_tl(state["ap"], state["t"], pert["ap"], pert["t"], ext, write_qsat=True)
    full = dict(state, qsat=qsat)
    _, comp_i = autodiff.tl_masked(full, dict(pert, qsat=qsat_i), eta, dt, ext, want=NL_OUT)
    # adjoint: ad_step against ad_masked wanting qsat + saturation_ad(accumulate)
    forcing = to_device({n: tl_i[n] for n in NL_OUT}, gpu)
    traj = {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}
    want = ("t", "ap", "q", "ql", "qi", "aph", "tnd_cml_t")
    fused = autodiff.ad_step(state, forcing, eta, dt, ext, traj=traj, want=want)
    assert _lib.last_kernel() == "cs2::ad_step_kernel"
    comp = autodiff.ad_masked(full, forcing, eta, dt, ext, traj=traj, want=want + ("qsat",))
    autodiff.saturation_ad(state["ap"], state["t"], comp["qsat"], ext, want=("ap", "t"), into={n: comp[n] for n in ("ap", "t")})
    assert _lib.last_kernel() == "cs2::saturation_ad_kernel"
    torch.cuda.synchronize()
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        assert_close(f"tl_step out_{n}_i", from_device(fused_i[n])[:k], from_device(comp_i[n])[:k], dtype, rtol_mul=100.0)
    for n in want:
        k = NZ + 1 if n == "aph" else NZ
        assert_close(f"ad_step out_{n}_i", from_device(fused[n])[:k], from_device(comp[n])[:k], dtype, rtol_mul=100.0)
        assert not from_device(fused[n])[k:].any(), f"{n}: padding level written"


def test_forward_outputs_are_the_fused_nl_stencils_bit_for_bit(gpu):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, cloudsc2_step, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

    c = _case(np.float64)
    state, eta, dt, _ = _state(gpu, c, grad=("t",))
    got = cloudsc2_step(state, eta, dt, externals())
    kernel = _lib.last_kernel()
    outs = {"out_" + n: storage.zeros(NX, NZ, np.float64, gpu) for n in NL_OUT + ("qsat",)}
    compile_stencil("cloudsc2_nl_saturation", externals())(
        **{"in_" + n: f.detach() for n, f in state.items()}, **outs, in_eta=eta, dt=dt, origin=(0, 0, 0), domain=(NX, 1, NZ + 1),
        validate_args=True, exec_info=None)
    assert kernel == _lib.last_kernel() and "nl_ring_kernel" in kernel      # one launch, the headline step's kernel
    for n in NL_OUT + ("qsat",):
        assert torch.equal(got[n].detach(), outs["out_" + n]), n
    assert sorted(got) == sorted(NL_OUT + ("qsat",))


def test_the_other_forms_of_saturation_take_the_composition(gpu):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, cloudsc2_step

    dtype = np.float64
    c = _case(dtype, LPHYLIN=False)
    state, eta, dt, w = _state(gpu, c, grad=("t", "q", "ap"))
    out = cloudsc2_step(state, eta, dt, c["ext"])
    (out["tnd_t"].sum() + (out["fplsl"] * w).sum()).backward()
    assert _lib.last_kernel() == "cs2::saturation_ad_kernel"
    u, want_i = _tangent_case(c)
    tangents = _jvp(gpu, c, {n: f.detach() for n, f in state.items()}, eta, dt, u, c["ext"])
    assert _lib.last_kernel() == "cs2::tl_masked_kernel"
    torch.cuda.synchronize()
    forcing = _forcing(c, tnd_t=np.ones_like(c["w"]), fplsl=c["w"].copy())
    _, adj = run_oracle_ad(c["fields"], forcing, c["eta"], dt, dict(c["ext"], NLEV=NZ, AD_TRAJ_FIX=1), traj=c["nl0"])
    want_t, want_ap, _ = _total(c, adj)
    assert_close("grad t", from_device(state["t"].grad)[:NZ], want_t[:NZ], dtype, rtol_mul=1000.0)
    assert_close("grad ap", from_device(state["ap"].grad)[:NZ], want_ap[:NZ], dtype, rtol_mul=1000.0)
    assert_close("grad q", from_device(state["q"].grad)[:NZ], adj["q"][:NZ], dtype, rtol_mul=1000.0)
    assert_close("qsat", from_device(out["qsat"].detach())[:NZ], c["fields"]["in_qsat"][:NZ], dtype)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        assert_close(f"jvp out_{n}", from_device(tangents[n])[:k], want_i[n][:k], dtype, rtol_mul=100.0)


def test_evaporation_switch_takes_the_dense_adjoint_then_saturation_ad(gpu):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, cloudsc2_step

    dtype = np.float64
    c = _case(dtype, LEVAPLS2=True)
    state, eta, dt, w = _state(gpu, c, grad=("t", "q"))
    out = cloudsc2_step(state, eta, dt, c["ext"])
    (out["tnd_t"] * w).sum().backward()
    assert _lib.last_kernel() == "cs2::saturation_ad_kernel"
    torch.cuda.synchronize()
    _, adj = run_oracle_ad(c["fields"], _forcing(c, tnd_t=c["w"].copy()), c["eta"], dt, dict(c["ext"], NLEV=NZ, AD_TRAJ_FIX=1))
    want_t, _, _ = _total(c, adj)
    assert_close("evap grad t", from_device(state["t"].grad)[:NZ], want_t[:NZ], dtype, rtol_mul=1000.0)
    assert_close("evap grad q", from_device(state["q"].grad)[:NZ], adj["q"][:NZ], dtype, rtol_mul=1000.0)
    assert state["ap"].grad is None


def test_runs_on_a_non_default_stream(gpu):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import cloudsc2_step

    c = _case(np.float64)
    state, eta, dt, w = _state(gpu, c, grad=("t", "ap"))
    ref = cloudsc2_step(state, eta, dt)["tnd_t"].sum()
    g_ref = torch.autograd.grad(ref, [state["t"], state["ap"]])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        loss = cloudsc2_step(state, eta, dt)["tnd_t"].sum()
        g = torch.autograd.grad(loss, [state["t"], state["ap"]])
    side.synchronize()
    assert torch.equal(g[0], g_ref[0]) and torch.equal(g[1], g_ref[1]) and torch.equal(loss, ref)
