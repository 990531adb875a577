"""`cloudsc2`, `cloudsc2_step` and `saturation` under `torch.func`: Jacobian blocks (`jacfwd`, `jacrev`) and `vmap` of `jvp`
on one trajectory.  `jacfwd` and `vmap(jvp)` hand all tangents to ONE rule, which runs the multi-direction tangent-linear
kernel where a width is enabled for the precision (`autodiff.MULTI_WIDTH`); `jacrev` loops over single adjoint launches.
A batched state is refused.

Two columns of 40 levels: 82 inputs, 82 outputs per function.  Bounds: `assert_close` at its default between two ways of
running the same tangent-linear kernels; |norm1 - norm2| / (eps norm2) < 1e4 per column between forward and reverse mode,
the transpose identity of tests/test_step_grad.py (AD_TRAJ_FIX is forced by the derivative rules, so the VJP is the
transpose of the JVP)."""
import numpy as np
import pytest

from derivative_support import STEP_IN, host_case
from helpers import NL_IN, assert_close, externals, increments, to_device

pytestmark = pytest.mark.gpu
NX, NZ = 2, 40
NLEV = NZ + 1
FUNCTIONS = ("cloudsc2_step", "cloudsc2", "saturation")


def _f(gpu, what, dtype):
    """(f, t, host t): f(t) = the `tnd_t` output (`saturation`: qsat) as a function of the field `t`, everything else fixed"""
    import torch

    import gt4py_dwarf_p_cloudsc2_tl_ad_amd as pkg

    fields, eta, dt = host_case(NX, NZ, dtype)
    dev = to_device(fields, gpu)
    eta = torch.as_tensor(eta, device=gpu)
    t = dev["in_t"]
    if what == "saturation":
        return (lambda x: pkg.saturation(dev["in_ap"], x, externals())), t, fields["in_t"]
    names = STEP_IN if what == "cloudsc2_step" else NL_IN
    state = {n: dev["in_" + n] for n in names}
    return (lambda x: getattr(pkg, what)(dict(state, t=x), eta, dt, externals())["tnd_t"]), t, fields["in_t"]


def _matrix(jac):
    """(nx, 1, nlev, nx, 1, nlev) -> float64 [out column, out level, in column, in level]"""
    assert tuple(jac.shape) == (NX, 1, NLEV, NX, 1, NLEV)
    return jac.detach().cpu().numpy().astype(np.float64).reshape(NX, NLEV, NX, NLEV)


def _single_jvps(f, t):
    """the Jacobian from 82 single forward-mode launches (`torch.autograd.forward_ad`), one unit tangent each"""
    import torch
    import torch.autograd.forward_ad as fwad

    cols = []
    for i in range(NX * NLEV):
        e = torch.zeros(NX * NLEV, dtype=t.dtype, device=t.device)
        e[i] = 1.0
        with fwad.dual_level():
            out = f(fwad.make_dual(t, e.view(NX, 1, NLEV)))
            cols.append(fwad.unpack_dual(out).tangent.clone())
    return torch.stack(cols, dim=-1).reshape(NX, 1, NLEV, NX, 1, NLEV)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("what", FUNCTIONS)
def test_jacfwd_is_the_stack_of_single_jvps_and_block_diagonal(gpu, what, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    f, t, _ = _f(gpu, what, dtype)
    jac = torch.func.jacfwd(f)(t)
    kernel = _lib.last_kernel()
    single = {"cloudsc2_step": "tl_step", "cloudsc2": "tl_masked", "saturation": "saturation_tl"}[what]
    if what != "saturation":             # the multi-direction kernel ran, in a precision where a width is enabled
        multi = {"cloudsc2_step": "cs2::tl_dirs_step_kernel", "cloudsc2": "cs2::tl_dirs_kernel"}[what]
        assert kernel == (multi if autodiff.MULTI_WIDTH[t.dtype] > 1 else f"cs2::{single}_kernel"), kernel
    want = _single_jvps(f, t)
    assert _lib.last_kernel() == f"cs2::{single}_kernel"
    torch.cuda.synchronize()
    got, want = _matrix(jac), _matrix(want)
    assert np.abs(want).max() > 0
    assert_close(f"jacfwd {what}", got.astype(dtype), want.astype(dtype), dtype)
    for c in range(NX):
        for o in range(NX):
            if c != o:
                assert not got[c, :, o, :].any(), f"{what}: column {c} depends on column {o}"
        assert got[c, :, c, :].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("what", ["cloudsc2_step", "cloudsc2"])
def test_jacfwd_through_the_multi_direction_kernel(gpu, monkeypatch, what, dtype):
    """the same with the full width switched on, whatever width the precision has by default: the `vmap` rule hands the 82
    tangents to the multi-direction kernel in chunks of 8 (ten full ones and one of 2)"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    f, t, _ = _f(gpu, what, dtype)
    monkeypatch.setitem(autodiff.MULTI_WIDTH, t.dtype, _lib.TL_MAX_DIRS)
    jac = torch.func.jacfwd(f)(t)
    assert _lib.last_kernel() == {"cloudsc2_step": "cs2::tl_dirs_step_kernel", "cloudsc2": "cs2::tl_dirs_kernel"}[what]
    want = _single_jvps(f, t)
    torch.cuda.synchronize()
    assert_close(f"jacfwd {what}, width 8", _matrix(jac).astype(dtype), _matrix(want).astype(dtype), dtype)


@pytest.mark.parametrize("what", FUNCTIONS)
def test_jacrev_is_the_transpose_of_jacfwd(gpu, what):
    """<J u, J u> == <u, J^T (J u)> per column with J u from `jacfwd` and J^T from `jacrev`, u the 1 % increment of t"""
    import torch

    dtype = np.float64
    f, t, host_t = _f(gpu, what, dtype)
    fwd, rev = _matrix(torch.func.jacfwd(f)(t)), _matrix(torch.func.jacrev(f)(t))
    torch.cuda.synchronize()
    u = increments({"in_t": host_t}, 0.01)["in_t_i"].astype(np.float64)        # [level][column]
    for c in range(NX):
        ju = fwd[c, :, c, :] @ u[:, c]
        norm1, norm2 = float(ju @ ju), float(u[:, c] @ (rev[c, :, c, :].T @ ju))
        assert norm2 != 0
        norm3 = abs(norm1 - norm2) / (np.finfo(dtype).eps * abs(norm2))
        print(f"{what} jacrev/jacfwd identity column {c}: {norm3:.3e} x eps")
        assert norm3 < 1e4, norm3
        for o in range(NX):
            if c != o:
                assert not rev[c, :, o, :].any()


@pytest.mark.parametrize("what", FUNCTIONS)
def test_vmap_of_jvp_equals_single_calls(gpu, what):
    import torch

    dtype = np.float64
    f, t, host_t = _f(gpu, what, dtype)
    rng = np.random.default_rng(7)
    tangents = torch.as_tensor(np.stack([(0.01 * (d + 1) * rng.standard_normal(host_t.shape) * host_t).T[:, None, :]
                                         for d in range(5)]), device=gpu)
    got = torch.func.vmap(lambda v: torch.func.jvp(f, (t,), (v,))[1])(tangents)
    want = [torch.func.jvp(f, (t,), (tangents[d],))[1] for d in range(5)]
    torch.cuda.synchronize()
    assert tuple(got.shape) == (5, NX, 1, NLEV)
    for d in range(5):
        a, b = got[d].cpu().numpy()[:, 0, :], want[d].cpu().numpy()[:, 0, :]
        assert np.abs(b).max() > 0
        assert_close(f"vmap(jvp) {what}[{d}]", a, b, dtype)


@pytest.mark.parametrize("what", FUNCTIONS)
def test_a_batched_state_is_refused(gpu, what):
    import torch

    f, t, _ = _f(gpu, what, np.float64)
    with pytest.raises(NotImplementedError, match="only tangents and cotangents may be batched"):
        torch.func.vmap(f)(torch.stack([t, t]))
