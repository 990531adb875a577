"""`cloudsc2` and `cloudsc2_step` in reverse mode under `torch.func` with the multi-direction adjoint switched on
(`autodiff.AD_MULTI_WIDTH` monkeypatched to the full width, whatever width the precision has by default): `jacrev` and
`vmap` of a `vjp` function hand all cotangents to ONE rule, which serves them to `ad_dirs_kernel` / `ad_dirs_step_kernel`
in chunks.  A batched state is still refused.

Two columns of 40 levels, the case of tests/test_autodiff_func.py: 82 inputs, 82 outputs per function.  Bound:
`assert_close` at its default between two ways of running the same adjoint arithmetic."""
import numpy as np
import pytest

from derivative_support import STEP_IN, host_case
from helpers import NL_IN, assert_close, externals, to_device

pytestmark = pytest.mark.gpu
NX, NZ = 2, 40
NLEV = NZ + 1
KERNELS = {"cloudsc2_step": ("cs2::ad_dirs_step_kernel", "cs2::ad_step_kernel"),
           "cloudsc2": ("cs2::ad_dirs_kernel", "cs2::ad_masked_kernel")}


def _f(gpu, what, dtype):
    """(f, t): f(t) = the `tnd_t` output as a function of the field `t`, everything else fixed"""
    import torch

    import gt4py_dwarf_p_cloudsc2_tl_ad_amd as pkg

    fields, eta, dt = host_case(NX, NZ, dtype)
    dev = to_device(fields, gpu)
    eta = torch.as_tensor(eta, device=gpu)
    state = {n: dev["in_" + n] for n in (STEP_IN if what == "cloudsc2_step" else NL_IN)}
    return (lambda x: getattr(pkg, what)(dict(state, t=x), eta, dt, externals())["tnd_t"]), dev["in_t"]


def _full_width(monkeypatch, t):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    monkeypatch.setitem(autodiff.AD_MULTI_WIDTH, t.dtype, _lib.AD_MAX_DIRS)


def _matrix(jac):
    """(nx, 1, nlev, nx, 1, nlev) -> float64 [out column, out level, in column, in level]"""
    assert tuple(jac.shape) == (NX, 1, NLEV, NX, 1, NLEV)
    return jac.detach().cpu().numpy().astype(np.float64).reshape(NX, NLEV, NX, NLEV)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("what", sorted(KERNELS))
def test_jacrev_runs_the_multi_direction_adjoint_and_is_the_stack_of_single_grads(gpu, monkeypatch, what, dtype):
    """82 unit cotangents in chunks of 8: ten full launches and one of 2"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    f, t = _f(gpu, what, dtype)
    _full_width(monkeypatch, t)
    jac = torch.func.jacrev(f)(t)
    assert _lib.last_kernel() == KERNELS[what][0]
    x = t.detach().requires_grad_(True)
    out = f(x)
    rows = []
    for i in range(NX * NLEV):
        e = torch.zeros(NX * NLEV, dtype=t.dtype, device=t.device)
        e[i] = 1.0
        rows.append(torch.autograd.grad(out, x, e.view(NX, 1, NLEV), retain_graph=True)[0])
        assert _lib.last_kernel() == KERNELS[what][1]
    want = torch.stack(rows).reshape(NX, 1, NLEV, NX, 1, NLEV)
    torch.cuda.synchronize()
    got, want = _matrix(jac), _matrix(want)
    assert np.abs(want).max() > 0
    assert_close(f"jacrev {what}, width 8", got.astype(dtype), want.astype(dtype), dtype)
    for c in range(NX):
        for o in range(NX):
            if c != o:
                assert not got[c, :, o, :].any(), f"{what}: column {c} depends on column {o}"
        assert got[c, :, c, :].any()


@pytest.mark.parametrize("what", sorted(KERNELS))
def test_vmap_of_a_vjp_function_equals_single_calls(gpu, monkeypatch, what):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    dtype = np.float64
    f, t = _f(gpu, what, dtype)
    _full_width(monkeypatch, t)
    rng = np.random.default_rng(7)
    cots = torch.as_tensor(np.stack([(d + 1) * rng.standard_normal((NX, 1, NLEV)) for d in range(5)]), device=gpu)
    _, vjp_fn = torch.func.vjp(f, t)
    got = torch.func.vmap(lambda c: vjp_fn(c)[0])(cots)
    assert _lib.last_kernel() == KERNELS[what][0]
    x = t.detach().requires_grad_(True)
    out = f(x)
    want = [torch.autograd.grad(out, x, cots[d], retain_graph=True)[0] for d in range(5)]
    assert _lib.last_kernel() == KERNELS[what][1]
    torch.cuda.synchronize()
    assert tuple(got.shape) == (5, NX, 1, NLEV)
    for d in range(5):
        a, b = got[d].cpu().numpy()[:, 0, :], want[d].cpu().numpy()[:, 0, :]
        assert np.abs(b).max() > 0
        assert_close(f"vmap(vjp) {what}[{d}]", a, b, dtype)


@pytest.mark.parametrize("what", sorted(KERNELS))
def test_a_batched_state_is_still_refused(gpu, monkeypatch, what):
    import torch

    f, t = _f(gpu, what, np.float64)
    _full_width(monkeypatch, t)
    with pytest.raises(NotImplementedError, match="only tangents and cotangents may be batched"):
        torch.func.vmap(f)(torch.stack([t, t]))
    c = torch.ones_like(t)
    with pytest.raises(NotImplementedError, match="only tangents and cotangents may be batched"):
        torch.func.vmap(lambda x: torch.func.vjp(f, x)[1](c)[0])(torch.stack([t, t]))
