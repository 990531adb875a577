"""Ensemble Jacobians through `torch.func`, opt-in (`autodiff.ENSEMBLE_JACOBIANS = True`): `vmap(jacrev(f))` and
`vmap(jacfwd(f))` over stacked states equal `jacrev(f)` / `jacfwd(f)` member by member - `assert_close` at its default, both
sides run the same level functions on the same words - and the cotangents of all members ran in the members-times-directions
kernel.  Three members of 63 columns, a 2 x 2 slice of one output as tests/test_autodiff_ensemble.py uses for the refusal:
two columns and two levels of `tnd_t`.  The refusal test takes the top two levels, where every derivative is zero; here the
two levels start where member 0's `tnd_t` is largest in those columns (`_level`), so that the Jacobians compared are not
all zero - member 0's is asserted not to be.
`vmap(jacfwd(f))` itself runs at two columns and five levels, where `t` has twelve elements and so twelve tangents (at 63 x
138 it would push 8 694 through a launch each); there every output is differentiated, and at least one member's Jacobian
is asserted not to be zero.  At the larger shape it is written out as what it is, `vmap(vmap(jvp))`, with two tangents the
members share.  The non-LPHYLIN step, which has no kernel of its own, loops over the members in both modes.
What stays refused still raises.  The flag is restored after every test."""
import numpy as np
import pytest

from derivative_support import SEED, STEP_IN
from helpers import NL_IN, assert_close, externals, nl_case, to_device

pytestmark = pytest.mark.gpu
NX, NZ, NMEM = 63, 137, 3
KERNEL = {"cloudsc2": "cs2::ad_mdirs_kernel", "cloudsc2_step": "cs2::ad_mdirs_step_kernel"}
TL_KERNEL = {"cloudsc2": "cs2::tl_ens_kernel", "cloudsc2_step": "cs2::tl_ens_step_kernel"}


@pytest.fixture()
def jacobians():
    """the module with `ENSEMBLE_JACOBIANS` set; it, `EVAP_ADJOINT` and `EVAP_ENSEMBLE` are what they were afterwards"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    before = (autodiff.ENSEMBLE_JACOBIANS, autodiff.EVAP_ADJOINT, autodiff.EVAP_ENSEMBLE)
    autodiff.ENSEMBLE_JACOBIANS = True
    yield autodiff
    autodiff.ENSEMBLE_JACOBIANS, autodiff.EVAP_ADJOINT, autodiff.EVAP_ENSEMBLE = before


def _setup(gpu, dtype, which, nx=NX, nz=NZ, **flags):
    """-> the differentiable call, members (per member {name: field}), stacked {name: (NMEM, NX, 1, NZ+1)}, eta (member
    0's: it is shared), dt, externals"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    f, names = {"cloudsc2": (autodiff.cloudsc2, NL_IN), "cloudsc2_step": (autodiff.cloudsc2_step, STEP_IN)}[which]
    ext = externals(NLEV=nz, **flags)
    cases = [nl_case(nx, nz, dtype=dtype, seed=SEED + 100 + m, ext=ext) for m in range(NMEM)]
    members = []
    for fields, _, _ in cases:
        dev = to_device(fields, gpu)
        members.append({n: dev["in_" + n] for n in names})
    stacked = {n: torch.stack([mem[n] for mem in members]) for n in names}
    return f, members, stacked, torch.as_tensor(cases[0][1], device=gpu), cases[0][2], ext


def _level(f, members, eta, dt, ext):
    """the first of the two levels of the output slice: where member 0's `tnd_t` is largest in the first two columns"""
    out = f(members[0], eta, dt, ext)["tnd_t"].detach()
    return min(int(out[:2, 0, :NZ].abs().sum(dim=0).argmax()), NZ - 2)


def _compare(what, got, members, jac, one, dtype):
    """`got`: (NMEM, 2, 2, NX, 1, NZ+1) against `jac(one)` on each member"""
    assert tuple(got.shape) == (NMEM, 2, 2, NX, 1, NZ + 1)
    for m, mem in enumerate(members):
        want = jac(one)(mem["t"], {n: f for n, f in mem.items() if n != "t"})
        a, b = got[m].detach().cpu().numpy(), want.detach().cpu().numpy()
        print(f"{what}[{m}]: largest entry of the member's own Jacobian {np.abs(b).max():.3e}")
        if m == 0:
            assert np.abs(b).max() > 0
        assert_close(f"{what}[{m}]", a[..., :NZ], b[..., :NZ], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_vmap_of_jacrev_equals_jacrev_per_member_in_one_launch(gpu, jacobians, which, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    f, members, stacked, eta, dt, ext = _setup(gpu, dtype, which)
    k = _level(f, members, eta, dt, ext)
    one = lambda t, others: f({**others, "t": t}, eta, dt, ext)["tnd_t"][:2, 0, k:k + 2]  # noqa: E731
    rest = {n: stacked[n] for n in stacked if n != "t"}
    got = torch.func.vmap(torch.func.jacrev(one))(stacked["t"], rest)
    assert _lib.last_kernel() == KERNEL[which]
    _compare(f"vmap(jacrev({which}))", got, members, torch.func.jacrev, one, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_vmap_of_vmap_of_jvp_equals_it_per_member_on_the_ensemble_kernels(gpu, jacobians, which, dtype):
    """what `vmap(jacfwd(f))` is, with two tangents shared by the members: 1 % of member 0's `t` and 2 % of member 1's"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    f, members, stacked, eta, dt, ext = _setup(gpu, dtype, which)
    k = _level(f, members, eta, dt, ext)
    one = lambda t, others: f({**others, "t": t}, eta, dt, ext)["tnd_t"][:2, 0, k:k + 2]  # noqa: E731
    tangents = torch.stack([0.01 * members[0]["t"], 0.02 * members[1]["t"]])

    def columns(t, others):      # the two columns of the Jacobian along the tangents: (2, 2, 2)
        return torch.func.vmap(lambda v: torch.func.jvp(lambda x: one(x, others), (t,), (v,))[1])(tangents)
    rest = {n: stacked[n] for n in stacked if n != "t"}
    got = torch.func.vmap(columns)(stacked["t"], rest)
    assert _lib.last_kernel() == TL_KERNEL[which]
    assert tuple(got.shape) == (NMEM, 2, 2, 2)
    for m, mem in enumerate(members):
        want = columns(mem["t"], {n: x for n, x in mem.items() if n != "t"})
        a, b = got[m].detach().cpu().numpy(), want.detach().cpu().numpy()
        print(f"vmap(vmap(jvp({which})))[{m}]: largest entry {np.abs(b).max():.3e}")
        if m == 0:
            assert np.abs(b).max() > 0
        assert_close(f"vmap(vmap(jvp({which})))[{m}]", a, b, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_vmap_of_jacfwd_equals_jacfwd_per_member_on_the_ensemble_kernels(gpu, jacobians, which, dtype):
    """the literal `vmap(jacfwd(f))`, all ten outputs with respect to every element of `t`: two columns, five levels"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_OUT

    nx, nz = 2, 5
    f, members, stacked, eta, dt, ext = _setup(gpu, dtype, which, nx, nz)

    def one(t, others):
        out = f({**others, "t": t}, eta, dt, ext)
        return torch.stack([out[n] for n in NL_OUT])
    rest = {n: stacked[n] for n in stacked if n != "t"}
    got = torch.func.vmap(torch.func.jacfwd(one))(stacked["t"], rest)
    assert _lib.last_kernel() == TL_KERNEL[which]
    assert tuple(got.shape) == (NMEM, len(NL_OUT), nx, 1, nz + 1, nx, 1, nz + 1)
    largest = []
    for m, mem in enumerate(members):
        want = torch.func.jacfwd(one)(mem["t"], {n: x for n, x in mem.items() if n != "t"})
        a, b = got[m].detach().cpu().numpy(), want.detach().cpu().numpy()
        largest.append(float(np.abs(b).max()))
        print(f"vmap(jacfwd({which}))[{m}]: largest entry of the member's own Jacobian {largest[-1]:.3e}")
        for i, n in enumerate(NL_OUT):      # per output: each has its own magnitude
            assert_close(f"vmap(jacfwd({which})) {n}[{m}]", a[i], b[i], dtype)
    assert max(largest) > 0


@pytest.mark.parametrize("mode", ["jacrev", "jvp"])
def test_the_step_without_lphylin_loops_over_the_members(gpu, jacobians, mode):
    """no fused kernel, no ensemble kernel: the multi-direction path of `cloudsc2_step`, member by member"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    dtype, which = np.float64, "cloudsc2_step"
    f, members, stacked, eta, dt, ext = _setup(gpu, dtype, which, LPHYLIN=False)
    k = _level(f, members, eta, dt, ext)
    one = lambda t, others: f({**others, "t": t}, eta, dt, ext)["tnd_t"][:2, 0, k:k + 2]  # noqa: E731
    rest = {n: stacked[n] for n in stacked if n != "t"}
    if mode == "jacrev":
        got = torch.func.vmap(torch.func.jacrev(one))(stacked["t"], rest)
        assert "mdirs" not in _lib.last_kernel() and "ens" not in _lib.last_kernel()
        _compare("vmap(jacrev(cloudsc2_step)) LPHYLIN=False", got, members, torch.func.jacrev, one, dtype)
        return
    tangents = torch.stack([0.01 * members[0]["t"], 0.02 * members[1]["t"]])

    def columns(t, others):
        return torch.func.vmap(lambda v: torch.func.jvp(lambda x: one(x, others), (t,), (v,))[1])(tangents)
    got = torch.func.vmap(columns)(stacked["t"], rest)
    assert "ens" not in _lib.last_kernel()
    for m, mem in enumerate(members):
        want = columns(mem["t"], {n: x for n, x in mem.items() if n != "t"})
        a, b = got[m].detach().cpu().numpy(), want.detach().cpu().numpy()
        if m == 0:
            assert np.abs(b).max() > 0
        assert_close(f"vmap(vmap(jvp(cloudsc2_step))) LPHYLIN=False [{m}]", a, b, dtype)


@pytest.mark.parametrize("mode", ["dense", "trajectory"])
@pytest.mark.parametrize("which", ["cloudsc2", "cloudsc2_step"])
def test_with_the_evaporation_switch_the_members_loop_and_no_new_kernel_runs(gpu, jacobians, which, mode):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    dtype = np.float64
    jacobians.EVAP_ADJOINT = mode
    f, members, stacked, eta, dt, ext = _setup(gpu, dtype, which, LEVAPLS2=True)
    k = _level(f, members, eta, dt, ext)
    one = lambda t, others: f({**others, "t": t}, eta, dt, ext)["tnd_t"][:2, 0, k:k + 2]  # noqa: E731
    rest = {n: stacked[n] for n in stacked if n != "t"}
    got = torch.func.vmap(torch.func.jacrev(one))(stacked["t"], rest)
    assert "mdirs" not in _lib.last_kernel()
    _compare(f"vmap(jacrev({which})) LEVAPLS2 {mode}", got, members, torch.func.jacrev, one, dtype)


def test_what_stays_refused_still_raises(gpu, jacobians):
    import torch

    autodiff = jacobians
    f, members, stacked, eta, dt, ext = _setup(gpu, np.float64, "cloudsc2")
    rest = {n: stacked[n] for n in NL_IN if n != "t"}
    one = lambda t, others: autodiff.cloudsc2({**others, "t": t}, eta, dt, ext)["tnd_t"][:2, 0, :2]  # noqa: E731
    # a batched eta
    etas = torch.stack([eta] * NMEM)
    with pytest.raises(NotImplementedError, match="eta"):
        torch.func.vmap(lambda e: autodiff.cloudsc2(members[0], e, dt, ext)["tnd_t"])(etas)
    # ... under the Jacobian of an ensemble too
    with pytest.raises(NotImplementedError, match="eta"):
        torch.func.vmap(torch.func.jacrev(
            lambda t, others, e: autodiff.cloudsc2({**others, "t": t}, e, dt, ext)["tnd_t"][:2, 0, :2]))(stacked["t"], rest, etas)
    # a state batched in part, under the Jacobian too
    shared = {n: members[0][n] for n in NL_IN if n != "t"}
    with pytest.raises(NotImplementedError, match="SOME fields"):
        torch.func.vmap(torch.func.jacrev(lambda t: one(t, shared)))(stacked["t"])
    # two batch levels over the state
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.vmap(torch.func.vmap(lambda t: autodiff.cloudsc2(dict(members[0], t=t), eta, dt, ext)["tnd_t"]))(
            torch.stack([stacked["t"]] * 2))
    # directions outer, members inner: `jacrev` applied outside the ensemble Function
    ens = lambda t: autodiff.cloudsc2_ensemble({**rest, "t": t}, eta, dt, ext)["tnd_t"][:, :2, 0, :2]  # noqa: E731
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.jacrev(ens)(stacked["t"])
    # two batch levels over the directions, the state plain
    _, vjp_fn = torch.func.vjp(lambda t: autodiff.cloudsc2(dict(members[0], t=t), eta, dt, ext)["tnd_t"], members[0]["t"])
    cots = torch.ones((2, 2, NX, 1, NZ + 1), dtype=torch.float64, device=gpu)
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.vmap(torch.func.vmap(lambda c: vjp_fn(c)[0]))(cots)

    # ... and with the state batched outside them: a third level

    def rows(t, others):
        _, pull = torch.func.vjp(lambda x: autodiff.cloudsc2({**others, "t": x}, eta, dt, ext)["tnd_t"], t)
        return torch.func.vmap(torch.func.vmap(lambda c: pull(c)[0]))(cots)
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.vmap(rows)(stacked["t"], rest)
    # `saturation` on its own under nesting
    sat = lambda t, ap: autodiff.saturation(ap, t, ext)[:2, 0, :2]  # noqa: E731
    with pytest.raises(NotImplementedError, match="members times directions"):
        torch.func.vmap(torch.func.jacrev(sat))(stacked["t"], stacked["ap"])
