"""The checker of `saturation`'s derivative, shared by tests/test_saturation_grad.py and tests/test_step_grad.py: the formula
of common/_stencils/saturation.py:23-42 + fcttre.py:22-57 written as PyTorch operations on CPU float64 tensors and
differentiated by `torch.autograd` - nothing of the code under test is involved.  `min` / `max` / `clamp` pass the gradient
to the branch that was taken, so a clamped branch has derivative 0."""
import numpy as np
import torch

from helpers import oracle


def qsat_torch(ap: torch.Tensor, t: torch.Tensor, e) -> torch.Tensor:
    """qsat of float64 tensors `ap`, `t` (any shape); all three forms (LPHYLIN; KFLAG == 1 / other)"""
    cu = (not e["LPHYLIN"]) and e["KFLAG"] == 1
    ti, ri = (e["RTICECU"], e["RTWAT_RTICECU_R"]) if cu else (e["RTICE"], e["RTWAT_RTICE_R"])
    alfa = torch.clamp(((torch.clamp(t, min=ti, max=e["RTWAT"]) - ti) * ri) ** 2.0, max=1.0)
    el = e["R2ES"] * torch.exp(e["R3LES"] * (t - e["RTT"]) / (t - e["R4LES"]))
    ei = e["R2ES"] * torch.exp(e["R3IES"] * (t - e["RTT"]) / (t - e["R4IES"]))
    ew = alfa * el + (1.0 - alfa) * ei
    qs = torch.clamp(ew / ap, max=e["QMAX"])
    return qs / (1.0 - e["RETV"] * qs)


def ew_numpy(t: np.ndarray, e) -> np.ndarray:
    """the saturation vapour pressure `ew` (what `ap` is set to for a point clipped at QMAX)"""
    one = torch.ones(t.shape, dtype=torch.float64)
    big = dict(e, QMAX=1e300, RETV=0.0)
    return qsat_torch(one, torch.as_tensor(t.astype(np.float64)), big).numpy()


def saturation_derivative(in_ap: np.ndarray, in_t: np.ndarray, e):
    """(qsat, g_t, g_ap, clipped) as float64 (nz+1, nx) arrays for (nz+1, nx) inputs of any float type; level nz is 0 (it is
    outside `saturation`'s domain).  Asserts that the value is the NumPy oracle's to 1e-14 relative."""
    nz = in_ap.shape[0] - 1
    ap = torch.tensor(in_ap[:nz].astype(np.float64), requires_grad=True)
    t = torch.tensor(in_t[:nz].astype(np.float64), requires_grad=True)
    q = qsat_torch(ap, t, e)
    g_ap, g_t = torch.autograd.grad(q.sum(), [ap, t])
    want = np.zeros((nz + 1,) + in_ap.shape[1:])
    oracle.saturation(in_ap.astype(np.float64), in_t.astype(np.float64), want, e)
    got = q.detach().numpy()
    assert np.all(np.abs(got - want[:nz]) <= 1e-14 * np.abs(want[:nz])), float(np.max(np.abs(got / want[:nz] - 1.0)))
    pad = lambda a: np.concatenate([a, np.zeros((1,) + a.shape[1:])])  # noqa: E731
    with torch.no_grad():
        clipped = (qsat_torch(ap, t, dict(e, QMAX=1e300)) != q).numpy()
    return pad(got), pad(g_t.numpy()), pad(g_ap.numpy()), pad(clipped).astype(bool)
