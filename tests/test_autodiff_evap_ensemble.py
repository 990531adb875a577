"""`autodiff.EVAP_ENSEMBLE`, `ad_masked_evap_ens` and `ad_step_evap_ens` on the GPU: with `EVAP_ADJOINT = "trajectory"` and
`EVAP_ENSEMBLE = True` the backward of an ensemble under LEVAPLS2 is ONE launch of the cover kernels' ensemble form, and every
member's gradient is the single call's; in every other setting the members are looped as before.

The case is tests/test_evap_adjoint.py's (its builder asserts on the CPU that the evaporation block runs): 2 members x 63
columns x 137 levels in fp64, the functional that file differentiates (weights on the four tendencies and `covptot`), member
m's weighed by SCALE[m], so the two gradients differ.  `assert_close` at its default against the single call."""
import numpy as np
import pytest

import test_evap_adjoint as single
from derivative_support import STATE4, STEP_IN, Box
from helpers import NL_IN, assert_close, from_device

pytestmark = pytest.mark.gpu
DT, AD_OUT = single.DT, single.AD_OUT
DTYPE, NX, NZ = np.float64, 63, 137
SCALE = (1.0, 0.5)
COVER = {False: "cs2::ad_cover_kernel", True: "cs2::ad_cover_step_kernel"}
COVER_ENS = {False: "cs2::ad_cover_ens_kernel", True: "cs2::ad_cover_ens_step_kernel"}


def _setup(gpu, step):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    c = single.case(NX, NZ, DTYPE)
    box = Box(NX, NZ, DTYPE, gpu, False)
    names = STEP_IN if step else NL_IN
    eta = torch.as_tensor(c["eta"], device=gpu)
    w = {n: box.put(c["forcing"][n]) for n in AD_OUT}
    fns = (autodiff.cloudsc2_step, autodiff.cloudsc2_step_ensemble) if step else (autodiff.cloudsc2, autodiff.cloudsc2_ensemble)

    def members():
        st = {n: torch.stack([f, f]) for n, f in box.state(c["fields"], names).items()}
        for n in STATE4:
            st[n].requires_grad_(True)
        return st
    return c, box, names, eta, w, fns, members


def _ensemble_backward(fn, st, eta, ext, w):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    out = fn(st, eta, DT, ext)
    sum((out[n][m] * w[n]).sum() * SCALE[m] for n in AD_OUT for m in range(2)).backward()
    return _lib.last_kernel()


def _check(what, grads, ref):
    for n in STATE4:
        for m in range(2):
            assert_close(f"{what} member {m} grad {n}", from_device(grads[n][m])[:NZ], SCALE[m] * ref[n][:NZ], DTYPE)


@pytest.mark.parametrize("step", [False, True], ids=["cloudsc2", "cloudsc2_step"])
def test_the_ensemble_backward_is_one_launch_when_asked_for(gpu, step, monkeypatch):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    c, box, names, eta, w, (fn, fn_ens), members = _setup(gpu, step)
    assert autodiff.EVAP_ENSEMBLE is False and autodiff.EVAP_ADJOINT == "dense"
    monkeypatch.setattr(autodiff, "EVAP_ADJOINT", "trajectory")
    ref, kernel, _, _ = single._autodiff_run(gpu, fn, names, DTYPE, NX, NZ)
    assert kernel == COVER[step]
    # the default: looped, member by member, as before
    st = members()
    assert _ensemble_backward(fn_ens, st, eta, c["ext"], w) == COVER[step]
    _check("looped", {n: st[n].grad for n in STATE4}, ref)
    monkeypatch.setattr(autodiff, "EVAP_ENSEMBLE", True)
    st = members()
    assert _ensemble_backward(fn_ens, st, eta, c["ext"], w) == COVER_ENS[step]
    _check("ensemble backward", {n: st[n].grad for n in STATE4}, ref)
    # vmap(grad(cost)) over a whole stacked state, and grad through vmap
    scale = torch.tensor(SCALE, dtype=torch.float64, device=gpu)

    def cost(diff, rest, s):
        out = fn({**rest, **diff}, eta, DT, c["ext"])
        return sum((out[n] * w[n]).sum() for n in AD_OUT) * s

    st = {n: f.detach() for n, f in members().items()}
    diff, rest = {n: st[n] for n in STATE4}, {n: st[n] for n in names if n not in STATE4}
    per_member = torch.func.vmap(torch.func.grad(cost))(diff, rest, scale)
    assert _lib.last_kernel() == COVER_ENS[step]
    _check("vmap(grad)", per_member, ref)
    through = torch.func.grad(lambda d: torch.func.vmap(cost)(d, rest, scale).sum())(diff)
    assert _lib.last_kernel() == COVER_ENS[step]
    _check("grad(vmap)", through, ref)
    # the dense mode does not look at EVAP_ENSEMBLE
    monkeypatch.setattr(autodiff, "EVAP_ADJOINT", "dense")
    st = members()
    assert _ensemble_backward(fn_ens, st, eta, c["ext"], w) == ("cs2::saturation_ad_kernel" if step else "cs2::ad_kernel")


@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
def test_thin_calls_cover_round_trip_layouts_and_errors(gpu, step):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage

    c, box, names, eta, w, _, members = _setup(gpu, step)
    one, ens = (autodiff.ad_step_evap, autodiff.ad_step_evap_ens) if step else (autodiff.ad_masked_evap, autodiff.ad_masked_evap_ens)
    st1 = box.state(c["fields"], names)
    traj1 = box.nl_fluxes(box.state(c["fields"]), c["ext"], eta, DT)
    ref = {n: from_device(f) for n, f in one(st1, w, eta, DT, c["ext"], traj=traj1, want=STATE4).items()}
    st = {n: f.detach() for n, f in members().items()}
    traj = {n: torch.stack([f, f]) for n, f in traj1.items()}
    forcing = {n: torch.stack([f * s for s in SCALE]) for n, f in w.items()}
    cover = storage.zeros_batched(2, NX, NZ, torch.float64, gpu)
    cover.fill_(float("nan"))
    got = ens(st, forcing, eta, DT, c["ext"], traj=traj, want=STATE4, cover=cover)
    assert _lib.last_kernel() == COVER_ENS[step]
    _check("thin call", got, ref)
    cov = [from_device(cover[m]) for m in range(2)]
    assert not np.isnan(cov[0][:NZ]).any() and np.isnan(cov[0][NZ:]).all() and np.array_equal(cov[0], cov[1], equal_nan=True)
    again = ens(st, forcing, eta, DT, c["ext"], traj=traj, want=STATE4, cover=cover, cover_ready=True)
    for n in STATE4:
        assert torch.equal(again[n], got[n]), n
    assert all(np.array_equal(from_device(cover[m]), cov[m], equal_nan=True) for m in range(2))
    assert set(ens(st, forcing, eta, DT, c["ext"], traj=traj, want=("t",))) == {"t"}          # a cover of the call's own
    # tensors in another layout - a level-fastest state field, a cover with a gap between its members - go through one copy
    odd = dict(st, q=torch.empty((2, NX, 1, NZ + 1), dtype=torch.float64, device=gpu).copy_(st["q"]))
    assert odd["q"].stride(-1) == 1
    wide = torch.full((2, 2 * (NZ + 1) * box.pitch), float("nan"), dtype=torch.float64, device=gpu)
    gapped = wide[:, :(NZ + 1) * box.pitch].view(2, NZ + 1, box.pitch)[:, :, :NX].unsqueeze(2).permute(0, 3, 2, 1)
    other = ens(odd, forcing, eta, DT, c["ext"], traj=traj, want=STATE4, cover=gapped)
    for n in STATE4:
        assert torch.equal(other[n], got[n]), n
    assert all(np.array_equal(from_device(gapped[m])[:NZ], cov[m][:NZ]) for m in range(2))       # handed back
    assert bool(wide[:, (NZ + 1) * box.pitch:].isnan().all())
    with pytest.raises(ValueError, match="cover_ready without a `cover`"):
        ens(st, forcing, eta, DT, c["ext"], traj=traj, want=STATE4, cover_ready=True)
    with pytest.raises(ValueError, match="cover must be a tensor of shape"):
        ens(st, forcing, eta, DT, c["ext"], traj=traj, want=STATE4, cover=cover[0])
    with pytest.raises(ValueError, match="cover must be a tensor of shape"):
        ens(st, forcing, eta, DT, c["ext"], traj=traj, want=STATE4, cover=storage.zeros_batched(3, NX, NZ, torch.float64, gpu))
    with pytest.raises(ValueError, match="tnd_t must be a tensor of shape"):
        ens(st, dict(forcing, tnd_t=w["tnd_t"]), eta, DT, c["ext"], traj=traj, want=STATE4)
    with pytest.raises(ValueError, match="neither LEVAPLS2 nor LDRAIN1D"):
        ens(st, forcing, eta, DT, dict(c["ext"], LEVAPLS2=False), traj=traj, want=STATE4)
