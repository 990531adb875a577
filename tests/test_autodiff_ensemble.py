"""`torch.func.vmap` over the STATE of `cloudsc2`, `cloudsc2_step` and `saturation`, and the ensemble Functions
`cloudsc2_ensemble` / `cloudsc2_step_ensemble` underneath: an ensemble of three different states equals the loop over its
members - values, per-member gradients (`vmap(grad)`), the gradient through `vmap`, `vmap(jvp)` - and the one-launch paths
run the ensemble kernels.  `assert_close` at its default: both sides run the same level functions on the same words."""
import numpy as np
import pytest

from derivative_support import SEED, STEP_IN
from helpers import NL_IN, NL_OUT, assert_close, externals, from_device, nl_case, to_device

pytestmark = pytest.mark.gpu
NX, NZ, NMEM = 200, 137, 3
DIFF = ("t", "q")


def _setup(gpu, dtype, names, **flags):
    """-> members (per member {name: field}), stacked {name: (NMEM, NX, 1, NZ+1)}, eta (member 0's: it is shared), dt, the
    externals, a weight field"""
    import torch

    ext = externals(NLEV=NZ, **flags)
    cases = [nl_case(NX, NZ, dtype=dtype, seed=SEED + 100 + m, ext=ext) for m in range(NMEM)]
    members = []
    for fields, _, _ in cases:
        dev = to_device(fields, gpu)
        members.append({n: dev["in_" + n] for n in names})
    stacked = {n: torch.stack([mem[n] for mem in members]) for n in names}
    w = torch.as_tensor(np.random.default_rng(5).standard_normal((NX, 1, NZ + 1)).astype(dtype), device=gpu)
    return members, stacked, torch.as_tensor(cases[0][1], device=gpu), cases[0][2], ext, w


def _fn(which):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    return {"cloudsc2": (autodiff.cloudsc2, NL_IN), "cloudsc2_step": (autodiff.cloudsc2_step, STEP_IN)}[which]


def _close(what, got, want, dtype):
    a, b = from_device(got.detach()), from_device(want.detach())
    assert_close(what, a[:NZ], b[:NZ], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_vmap_over_the_state_equals_the_stacked_members(gpu, which, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    f, names = _fn(which)
    members, stacked, eta, dt, ext, _ = _setup(gpu, dtype, names)
    got = torch.func.vmap(lambda s: f(s, eta, dt, ext))(stacked)
    assert _lib.last_kernel() == ("cs2::nl_ens_kernel" if which == "cloudsc2" else "cs2::nl_ens_kernel<saturation>")
    for m, mem in enumerate(members):
        want = f(mem, eta, dt, ext)
        for n in want:
            assert tuple(got[n].shape) == (NMEM, NX, 1, NZ + 1)
            _close(f"vmap({which}) {n}[{m}]", got[n][m], want[n], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_vmap_of_saturation_equals_the_stacked_members(gpu, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    members, stacked, _, _, ext, w = _setup(gpu, dtype, ("ap", "t"))
    got = torch.func.vmap(lambda ap, t: autodiff.saturation(ap, t, ext))(stacked["ap"], stacked["t"])
    grads = torch.func.vmap(torch.func.grad(lambda t, ap: (autodiff.saturation(ap, t, ext) * w).sum()))(stacked["t"], stacked["ap"])
    for m, mem in enumerate(members):
        _close(f"vmap(saturation)[{m}]", got[m], autodiff.saturation(mem["ap"], mem["t"], ext), dtype)
        want = torch.func.grad(lambda t: (autodiff.saturation(mem["ap"], t, ext) * w).sum())(mem["t"])
        _close(f"vmap(grad(saturation))[{m}]", grads[m], want, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_per_member_gradients_and_the_gradient_through_vmap(gpu, which, dtype):
    """`vmap(grad(cost))(states)` equals the looped `grad(cost)(state_m)`; `grad` of a sum over `vmap(f)` equals the same
    gradients, member by member (the members are independent)"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    f, names = _fn(which)
    members, stacked, eta, dt, ext, w = _setup(gpu, dtype, names)

    def cost(diff, rest):
        out = f({**rest, **diff}, eta, dt, ext)
        return (out["tnd_t"] * w).sum() + (out["tnd_q"] * w).sum()

    split = lambda s: ({n: s[n] for n in DIFF}, {n: s[n] for n in names if n not in DIFF})  # noqa: E731
    per_member = torch.func.vmap(torch.func.grad(cost))(*split(stacked))
    assert _lib.last_kernel() == ("cs2::ad_ens_kernel" if which == "cloudsc2" else "cs2::ad_ens_step_kernel")
    diff, rest = split(stacked)
    through = torch.func.grad(lambda d: torch.func.vmap(cost)(d, rest).sum())(diff)
    assert _lib.last_kernel() == ("cs2::ad_ens_kernel" if which == "cloudsc2" else "cs2::ad_ens_step_kernel")
    for m, mem in enumerate(members):
        want = torch.func.grad(cost)(*split(mem))
        for n in DIFF:
            assert from_device(want[n]).any()
            _close(f"vmap(grad) {which} {n}[{m}]", per_member[n][m], want[n], dtype)
            _close(f"grad(vmap) {which} {n}[{m}]", through[n][m], want[n], dtype)


@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_vmap_of_jvp_over_state_and_tangent(gpu, which):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    dtype = np.float64
    f, names = _fn(which)
    members, stacked, eta, dt, ext, _ = _setup(gpu, dtype, names)
    rest = lambda s: {n: s[n] for n in names if n != "t"}  # noqa: E731

    def push(t, v, others):
        return torch.func.jvp(lambda x: f({**others, "t": x}, eta, dt, ext)["tnd_t"], (t,), (v,))

    v = 0.01 * stacked["t"]
    out, out_i = torch.func.vmap(push)(stacked["t"], v, rest(stacked))
    assert _lib.last_kernel() == ("cs2::tl_ens_kernel" if which == "cloudsc2" else "cs2::tl_ens_step_kernel")
    for m, mem in enumerate(members):
        want, want_i = push(mem["t"], 0.01 * mem["t"], rest(mem))
        assert from_device(want_i).any()
        _close(f"vmap(jvp) {which} primal[{m}]", out[m], want, dtype)
        _close(f"vmap(jvp) {which} tangent[{m}]", out_i[m], want_i, dtype)


def test_in_dims_with_only_t_batched(gpu):
    """A state batched in PART stays refused, with the message tests/test_autodiff_func.py and
    tests/test_autodiff_func_ad_multi.py have held `vmap(f)(torch.stack([t, t]))` to since before there were ensemble
    launches (f a function of `t` alone, the other fields closed over): an ensemble is a batch of whole states.  With the
    shared fields expanded by the caller the same call runs the ensemble launch and equals the loop."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    dtype = np.float64
    members, stacked, eta, dt, ext, _ = _setup(gpu, dtype, NL_IN)
    base = members[0]
    mixed = dict(base, t=stacked["t"])
    with pytest.raises(NotImplementedError, match="only tangents and cotangents may be batched"):
        torch.func.vmap(lambda s: autodiff.cloudsc2(s, eta, dt, ext), in_dims=({n: 0 if n == "t" else None for n in NL_IN},))(mixed)
    with pytest.raises(NotImplementedError, match="only tangents and cotangents may be batched"):
        torch.func.vmap(lambda t: autodiff.saturation(base["ap"], t, ext))(stacked["t"])
    whole = {n: stacked["t"] if n == "t" else base[n].unsqueeze(0).expand(NMEM, *base[n].shape) for n in NL_IN}
    got = torch.func.vmap(lambda s: autodiff.cloudsc2(s, eta, dt, ext))(whole)
    assert _lib.last_kernel() == "cs2::nl_ens_kernel"
    for m in range(NMEM):
        want = autodiff.cloudsc2(dict(base, t=members[m]["t"]), eta, dt, ext)
        for n in NL_OUT:
            _close(f"only t differs {n}[{m}]", got[n][m], want[n], dtype)


@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_the_ensemble_function_backward_and_forward_ad(gpu, which):
    import torch
    import torch.autograd.forward_ad as fwad

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    dtype = np.float64
    f, names = _fn(which)
    fe = autodiff.cloudsc2_ensemble if which == "cloudsc2" else autodiff.cloudsc2_step_ensemble
    members, stacked, eta, dt, ext, w = _setup(gpu, dtype, names)
    states = dict(stacked, t=stacked["t"].clone().requires_grad_(True))
    out = fe(states, eta, dt, ext)
    assert _lib.last_kernel().startswith("cs2::nl_ens_kernel")
    ((out["tnd_t"] * w).sum()).backward()
    assert _lib.last_kernel() == ("cs2::ad_ens_kernel" if which == "cloudsc2" else "cs2::ad_ens_step_kernel")
    with fwad.dual_level():
        dual = dict(stacked, t=fwad.make_dual(stacked["t"], 0.01 * stacked["t"]))
        tangent = fwad.unpack_dual(fe(dual, eta, dt, ext)["tnd_t"]).tangent
        assert _lib.last_kernel() == ("cs2::tl_ens_kernel" if which == "cloudsc2" else "cs2::tl_ens_step_kernel")
    for m, mem in enumerate(members):
        t = mem["t"].detach().requires_grad_(True)      # the member's own storage: a clone would lose its level pitch
        (f(dict(mem, t=t), eta, dt, ext)["tnd_t"] * w).sum().backward()
        _close(f"{which}_ensemble grad t[{m}]", states["t"].grad[m], t.grad, dtype)
        with fwad.dual_level():
            want = fwad.unpack_dual(f(dict(mem, t=fwad.make_dual(mem["t"], 0.01 * mem["t"])), eta, dt, ext)["tnd_t"]).tangent
        _close(f"{which}_ensemble tangent[{m}]", tangent[m], want, dtype)
    if which == "cloudsc2_step":
        assert not out["qsat"].requires_grad


@pytest.mark.parametrize("which,flags", [("cloudsc2", dict(LEVAPLS2=True)), ("cloudsc2_step", dict(LPHYLIN=False))],
                         ids=["LEVAPLS2", "step without LPHYLIN"])
def test_what_has_no_ensemble_kernel_loops_over_the_members(gpu, which, flags):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    dtype = np.float64
    f, names = _fn(which)
    members, stacked, eta, dt, ext, w = _setup(gpu, dtype, names, **flags)
    rest = lambda s: {n: s[n] for n in names if n != "t"}  # noqa: E731
    cost = lambda t, others: (f({**others, "t": t}, eta, dt, ext)["tnd_t"] * w).sum()  # noqa: E731
    got = torch.func.vmap(torch.func.grad(cost))(stacked["t"], rest(stacked))
    assert "ens" not in _lib.last_kernel(), _lib.last_kernel()
    for m, mem in enumerate(members):
        _close(f"{which} {flags} grad t[{m}]", got[m], torch.func.grad(cost)(mem["t"], rest(mem)), dtype)


def test_a_batched_eta_and_members_times_directions_are_refused(gpu):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    dtype = np.float64
    members, stacked, eta, dt, ext, _ = _setup(gpu, dtype, NL_IN)
    etas = torch.stack([eta] * NMEM)
    with pytest.raises(NotImplementedError, match="eta"):
        torch.func.vmap(lambda e: autodiff.cloudsc2(members[0], e, dt, ext)["tnd_t"])(etas)
    rest = {n: stacked[n] for n in NL_IN if n != "t"}
    one = lambda t, others: autodiff.cloudsc2({**others, "t": t}, eta, dt, ext)["tnd_t"][:2, 0, :2]  # noqa: E731
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.vmap(torch.func.jacrev(one))(stacked["t"], rest)
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.vmap(torch.func.vmap(lambda t: autodiff.cloudsc2(dict(members[0], t=t), eta, dt, ext)["tnd_t"]))(
            torch.stack([stacked["t"]] * 2))
