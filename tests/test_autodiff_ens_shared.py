"""`cloudsc2_ensemble` / `cloudsc2_step_ensemble` and the thin ensemble calls with `shared=` and a per-member `eta`: values and
gradients equal the loop over the members through the single Functions under plain autograd - per-member gradients for the
members' own fields, the SUM over the members for a shared field - the launches are the shared-state entries', and no
shared field is copied once per member.  `assert_close` at its default: both sides run the same level functions on the same
words; the member sum of a shared field's gradient is formed in another order than autograd's accumulation, which the
default tolerance of the dtype covers (NMEM = 3 terms)."""
import numpy as np
import pytest

from derivative_support import SEED, STEP_IN
from helpers import NL_IN, assert_close, externals, from_device, nl_case, to_device

pytestmark = pytest.mark.gpu
NX, NZ, NMEM = 257, 12, 3
OWN = ("t", "q", "ql", "qi")


def _setup(gpu, dtype, names):
    """-> per member {name: field} (the shared fields are member 0's), stacked own fields, shared fields, eta, dt, ext, weight"""
    import torch

    ext = externals(NLEV=NZ)
    cases = [nl_case(NX, NZ, dtype=dtype, seed=SEED + 300 + m, ext=ext) for m in range(NMEM)]
    dev = [to_device(c[0], gpu) for c in cases]
    shared = {n: dev[0]["in_" + n] for n in names if n not in OWN}
    members = [{n: (shared[n] if n in shared else dev[m]["in_" + n]) for n in names} for m in range(NMEM)]
    own = {n: _stack([mem[n] for mem in members]) for n in OWN}
    w = torch.as_tensor(np.random.default_rng(7).standard_normal((NX, 1, NZ + 1)).astype(dtype), device=gpu)
    return members, own, shared, torch.as_tensor(cases[0][1], device=gpu), cases[0][2], ext, w


def _stack(fields):
    """the members' fields as ONE member-major batch in the `storage.zeros_batched` layout, the layout of the ensemble calls:
    nothing has to be re-laid inside a call (`torch.stack` would give row-major members, which every call copies first)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage

    out = storage.zeros_batched(len(fields), NX, NZ, fields[0].dtype, fields[0].device)
    for m, f in enumerate(fields):
        assert storage.field_geometry(out[m]) == storage.field_geometry(f)
        out[m].copy_(f)
    return out


def _close(what, got, want, dtype, nlev=NZ):
    assert_close(what, from_device(got.detach())[:nlev], from_device(want.detach())[:nlev], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [True, False], ids=["step", "nl"])
def test_backward_sums_the_members_for_shared_inputs(gpu, step, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    names = STEP_IN if step else NL_IN
    ens_fn, one_fn = (autodiff.cloudsc2_step_ensemble, autodiff.cloudsc2_step) if step else (autodiff.cloudsc2_ensemble, autodiff.cloudsc2)
    members, own, shared, eta, dt, ext, w = _setup(gpu, dtype, names)
    if not step:      # qsat belongs to a member: it follows the member's t
        own["qsat"] = _stack([m["qsat"] for m in members])
        shared.pop("qsat")
    diff_own = {n: own[n].clone().requires_grad_() for n in ("t", "q")}
    # `ap` in the call's layout; `lude` as a dense clone, another layout: it is copied ONCE, as one field
    diff_sh = {"ap": shared["ap"].detach().requires_grad_(), "lude": shared["lude"].clone().requires_grad_()}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = ens_fn({**own, **diff_own}, eta, dt, ext, shared={**shared, **diff_sh})
    grown = torch.cuda.memory_allocated() - before
    assert _lib.last_kernel() == ("cs2::nl_enss_kernel<saturation>" if step else "cs2::nl_enss_kernel")
    # the results (10 outputs, + qsat for the step) and nothing like a member-batch per shared field (11 of them)
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage

    field = storage.field_geometry(out["tnd_t"][0])[2] * (NZ + 1) * np.dtype(dtype).itemsize
    assert grown < (len(out) + 1) * NMEM * field, (grown, field)
    ((out["tnd_t"] * w).sum() + (out["tnd_q"] * w).sum()).backward()
    assert _lib.last_kernel() == ("cs2::ad_enss_step_kernel" if step else "cs2::ad_enss_kernel")
    want_sh = {n: 0 for n in diff_sh}
    for m, mem in enumerate(members):
        d = {n: mem[n].detach().requires_grad_() for n in ("t", "q", "ap", "lude")}     # leaves of their own, same layout
        state = {**mem, **d}
        o = one_fn(state, eta, dt, ext)
        for n in ("tnd_t", "clc"):
            _close(f"value {n}[{m}]", out[n][m], o[n], dtype)
        ((o["tnd_t"] * w).sum() + (o["tnd_q"] * w).sum()).backward()
        for n in ("t", "q"):
            _close(f"grad {n}[{m}]", diff_own[n].grad[m], d[n].grad, dtype)
        for n in want_sh:
            want_sh[n] = want_sh[n] + d[n].grad
    for n in want_sh:
        assert tuple(diff_sh[n].grad.shape) == (NX, 1, NZ + 1)
        _close(f"grad of shared {n}", diff_sh[n].grad, want_sh[n], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_thin_calls_take_shared_and_a_per_member_eta(gpu, dtype):
    """`tl_step_ens` / `ad_step_ens` with `shared=` and eta (nmem, nz+1): each member equals the single call on that member's
    state and level vector; the adjoints of shared inputs come back per member"""
    import torch

    from grid_support import eta_family

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage

    members, own, shared, _, dt, ext, _ = _setup(gpu, dtype, STEP_IN)
    fam = eta_family(NZ, dtype)
    etas = torch.as_tensor(np.stack([fam["uniform"], fam["no_window_above"], fam["nps_eq_klo"]]), device=gpu)
    pert = {"t": own["t"] * 0.01, "q": own["q"] * 0.01}
    nl, out_i = autodiff.tl_step_ens(own, pert, etas, dt, ext, want=("tnd_t", "tnd_q"), write_nl=True, shared=shared)
    assert _lib.last_kernel() == "cs2::tl_enss_step_kernel"
    adj = autodiff.ad_step_ens(own, out_i, etas, dt, ext, traj={n: nl[n] for n in ("fplsl", "fplsn")}, want=("t", "ap"),
                               shared=shared)
    assert _lib.last_kernel() == "cs2::ad_enss_step_kernel"
    assert tuple(adj["ap"].shape) == (NMEM, NX, 1, NZ + 1)
    for m, mem in enumerate(members):
        geo = storage.field_geometry(mem["t"])      # the member's perturbations as fields of the single call's layout
        nl1, o1 = autodiff.tl_step(mem, {n: autodiff._in_layout(f[m], mem["t"], geo) for n, f in pert.items()}, etas[m], dt, ext,
                                   want=("tnd_t", "tnd_q"), write_nl=True)
        a1 = autodiff.ad_step(mem, o1, etas[m], dt, ext, traj={n: nl1[n] for n in ("fplsl", "fplsn")}, want=("t", "ap"))
        for n in o1:
            torch.testing.assert_close(out_i[n][m][:, :, :NZ], o1[n][:, :, :NZ])
        for n in a1:
            torch.testing.assert_close(adj[n][m][:, :, :NZ], a1[n][:, :, :NZ])


def test_without_the_flag_vmap_over_part_of_the_state_and_over_eta_are_refused(gpu):
    """`SHARED_STATE` is False by default: a state batched in part and a batched `eta` raise what they always have"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    assert autodiff.SHARED_STATE is False
    members, own, shared, eta, dt, ext, _ = _setup(gpu, np.float64, STEP_IN)
    with pytest.raises(NotImplementedError, match="part of the state"):
        torch.func.vmap(lambda o: autodiff.cloudsc2_step({**shared, **o}, eta, dt, ext))(own)
    full = {**{n: f.unsqueeze(0).expand(NMEM, *f.shape) for n, f in shared.items()}, **own}
    with pytest.raises(NotImplementedError, match="`eta` is shared"):
        torch.func.vmap(lambda s, e: autodiff.cloudsc2_step(s, e, dt, ext))(full, eta.unsqueeze(0).expand(NMEM, -1))


def _batch(got, want, what, dtype):
    for m in range(NMEM):
        _close(f"{what}[{m}]", got[m], want[m], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["cloudsc2_step", "cloudsc2"])
def test_shared_state_under_vmap_equals_the_expanded_states(gpu, monkeypatch, which, dtype):
    """`SHARED_STATE = True`: `vmap(f)` with part of the state at in_dims=None, `vmap(grad(cost))` and `vmap(jvp)` against the
    same function on fully expanded states (every field batched: the plain ensemble launches); the launches are the
    shared-state entries' and the forward allocates no member-batch per shared field"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage

    step = which == "cloudsc2_step"
    f, names = (autodiff.cloudsc2_step, STEP_IN) if step else (autodiff.cloudsc2, NL_IN)
    members, own, shared, eta, dt, ext, w = _setup(gpu, dtype, names)
    if not step:
        own["qsat"] = _stack([m["qsat"] for m in members])
        shared.pop("qsat")
    full = {**{n: x.unsqueeze(0).expand(NMEM, *x.shape) for n, x in shared.items()}, **own}
    diff = {n: own[n] for n in ("t", "q")}
    rest = {n: x for n, x in own.items() if n not in diff}

    def cost(d, other):
        out = f({**other, **d}, eta, dt, ext)
        return (out["tnd_t"] * w).sum() + (out["tnd_q"] * w).sum()

    def push(d, td, other):
        return torch.func.jvp(lambda x: f({**other, **x}, eta, dt, ext)["tnd_t"], (d,), (td,))[1]

    tang = {n: x * 0.01 for n, x in diff.items()}
    frest = {n: x for n, x in full.items() if n not in diff}
    want = torch.func.vmap(lambda s: f(s, eta, dt, ext))(full)
    assert _lib.last_kernel() == ("cs2::nl_ens_kernel<saturation>" if step else "cs2::nl_ens_kernel")
    want_j = torch.func.vmap(push)(diff, tang, frest)

    monkeypatch.setattr(autodiff, "SHARED_STATE", True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = torch.func.vmap(lambda o: f({**shared, **o}, eta, dt, ext))(own)
    grown = torch.cuda.memory_allocated() - before
    assert _lib.last_kernel() == ("cs2::nl_enss_kernel<saturation>" if step else "cs2::nl_enss_kernel")
    field = storage.field_geometry(members[0]["t"])[2] * (NZ + 1) * np.dtype(dtype).itemsize
    # the results (10 outputs, + qsat for the step) plus less than one member-batch of one field: the own fields are in the
    # call's layout already, and no shared field is copied per member (11 of them: 11 member-batches on top)
    print(f"vmap({which}) {np.dtype(dtype).name}: allocated over the call {grown} B = {grown / (NMEM * field):.2f} member-batches, "
          f"{len(got)} results")
    assert grown < (len(got) + 1) * NMEM * field, (grown, field)
    for n in want:
        _batch(got[n], want[n], f"vmap({which}) {n}", dtype)
    got_g = torch.func.vmap(torch.func.grad(lambda d: cost(d, {**shared, **rest})))(diff)
    assert _lib.last_kernel() == ("cs2::ad_enss_step_kernel" if step else "cs2::ad_enss_kernel")
    got_j = torch.func.vmap(lambda d, td: push(d, td, {**shared, **rest}))(diff, tang)
    assert _lib.last_kernel() == ("cs2::tl_enss_step_kernel" if step else "cs2::tl_enss_kernel")
    _batch(got_j, want_j, f"vmap(jvp({which}))", dtype)
    monkeypatch.setattr(autodiff, "SHARED_STATE", False)
    want_g = torch.func.vmap(torch.func.grad(cost))(diff, frest)
    assert _lib.last_kernel() == ("cs2::ad_ens_step_kernel" if step else "cs2::ad_ens_kernel")
    for n in diff:
        _batch(got_g[n], want_g[n], f"vmap(grad({which})) {n}", dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batched_eta_under_vmap_and_grad_through_vmap(gpu, monkeypatch, dtype):
    """`SHARED_STATE = True`: `vmap` over the members' own fields AND `eta`, shared fields closed over, against the loop over
    the members; `grad` of a sum over that `vmap` gives per-member gradients for the own fields and the member sum for a
    shared one"""
    import torch

    from grid_support import eta_family

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    members, own, shared, _, dt, ext, w = _setup(gpu, dtype, STEP_IN)
    fam = eta_family(NZ, dtype)
    etas = torch.as_tensor(np.stack([fam["uniform"], fam["no_window_above"], fam["nps_eq_klo"]]), device=gpu)
    monkeypatch.setattr(autodiff, "SHARED_STATE", True)

    def total(t, ap):
        out = torch.func.vmap(lambda tm, o, e: autodiff.cloudsc2_step({**shared, "ap": ap, **o, "t": tm}, e, dt, ext))(
            t, {n: x for n, x in own.items() if n != "t"}, etas)
        return (out["tnd_t"] * w).sum(), out

    (g_t, g_ap), got = torch.func.grad(total, argnums=(0, 1), has_aux=True)(own["t"], shared["ap"])
    assert _lib.last_kernel() == "cs2::ad_enss_step_kernel"
    sum_ap = 0
    for m, mem in enumerate(members):
        d = {n: mem[n].detach().requires_grad_() for n in ("t", "ap")}
        o = autodiff.cloudsc2_step({**mem, **d}, etas[m], dt, ext)
        for n in ("tnd_t", "clc", "fplsl"):
            _close(f"batched eta {n}[{m}]", got[n][m], o[n], dtype)
        (o["tnd_t"] * w).sum().backward()
        _close(f"grad through vmap t[{m}]", g_t[m], d["t"].grad, dtype)
        sum_ap = sum_ap + d["ap"].grad
    assert tuple(g_ap.shape) == (NX, 1, NZ + 1)
    _close("grad through vmap, shared ap", g_ap, sum_ap, dtype)
    # only eta batched: every state field closed over
    got = torch.func.vmap(lambda e: autodiff.cloudsc2_step(members[0], e, dt, ext)["tnd_q"])(etas)
    for m in range(NMEM):
        _close(f"eta alone [{m}]", got[m], autodiff.cloudsc2_step(members[0], etas[m], dt, ext)["tnd_q"], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jvp_of_the_ensemble_function_with_a_shared_tangent(gpu, dtype):
    """forward mode through `cloudsc2_step_ensemble(..., shared=)`: a tangent on a member field and one on a SHARED field (a
    plain field, which every member sees) against `jvp` of `cloudsc2_step` member by member"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    members, own, shared, eta, dt, ext, _ = _setup(gpu, dtype, STEP_IN)
    rest = {n: f for n, f in shared.items() if n != "ap"}
    t_t, t_ap = own["t"] * 0.01, shared["ap"] * 0.001
    got = torch.func.jvp(lambda t, ap: autodiff.cloudsc2_step_ensemble({**own, "t": t}, eta, dt, ext, shared={**rest, "ap": ap})["tnd_t"],
                         (own["t"], shared["ap"]), (t_t, t_ap))[1]
    assert _lib.last_kernel() == "cs2::tl_enss_step_kernel"
    for m, mem in enumerate(members):
        want = torch.func.jvp(lambda t, ap: autodiff.cloudsc2_step({**mem, "t": t, "ap": ap}, eta, dt, ext)["tnd_t"],
                              (mem["t"], mem["ap"]), (autodiff._as_field(t_t[m]), t_ap))[1]
        _close(f"jvp shared tangent [{m}]", got[m], want, dtype)


def test_an_expanded_field_is_recognised_only_with_the_flag(gpu, monkeypatch):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    members, own, shared, eta, dt, ext, _ = _setup(gpu, np.float64, STEP_IN)
    full = {**{n: f.unsqueeze(0).expand(NMEM, *f.shape) for n, f in shared.items()}, **own}
    want = autodiff.cloudsc2_step_ensemble(full, eta, dt, ext)
    assert _lib.last_kernel() == "cs2::nl_ens_kernel<saturation>"
    monkeypatch.setattr(autodiff, "SHARED_STATE", True)
    got = autodiff.cloudsc2_step_ensemble(full, eta, dt, ext)
    assert _lib.last_kernel() == "cs2::nl_enss_kernel<saturation>"
    for n in want:
        assert torch.equal(got[n], want[n]), n
