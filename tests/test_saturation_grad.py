"""The derivative of `saturation` on the GPU (C ABI `cloudsc2_saturation_tl_*` / `_ad_*`, `autodiff.saturation`) against the
analytic derivative of the reference's formula, taken by `torch.autograd` on CPU float64 (tests/saturation_oracle.py).

One column is set by hand so that every branch of the rule is present, a whole kelvin from each kink: t = TI - 1, TI + 1,
RTWAT - 1, RTWAT + 1, and a point clipped at QMAX (ap = ew).  No point is excluded from any comparison.

Tolerance: `helpers.assert_close` at its default (rtol_mul = 1), the bound `saturation`'s value is held to, for both
precisions.  (Expected beforehand: the derivative is a few more roundings of the same primitives - about 1e-15 relative in
float64 and 1e-6 in float32, where the exponent's argument of up to 20 is rounded to 6e-8 relative - against bounds of 1e-9 and
5e-4; no wider multiplier is used.  Measured against the CPU oracle on these inputs, as a fraction of the field's largest
value: 3.7e-16 / 3.0e-7 for `qsat_i`, 2.8e-16 / 2.5e-7 for the `t` adjoint, 1.0e-16 / 6.0e-7 for the `ap` adjoint.)"""
import ctypes

import numpy as np
import pytest

from derivative_support import Box
from helpers import assert_close, externals, from_device, nl_case
from saturation_oracle import ew_numpy, saturation_derivative

NX, NZ, COL = 130, 5, 77       # two waves and a ragged third; COL: the hand-set column
FORMS = {"lphylin": dict(LPHYLIN=True), "kflag1": dict(LPHYLIN=False, KFLAG=1), "kflag0": dict(LPHYLIN=False, KFLAG=0)}
_cases = {}


def _case(dtype, form):
    """host inputs, perturbations, forcing and the oracle's derivative: built once per (dtype, form), never modified"""
    key = (np.dtype(dtype), form)
    if key not in _cases:
        ext = externals(**FORMS[form])
        fields, _, _ = nl_case(NX, NZ, dtype=dtype)
        ap, t = fields["in_ap"].copy(), fields["in_t"].copy()
        ti = ext["RTICECU"] if form == "kflag1" else ext["RTICE"]
        t[:NZ, COL] = np.array([ti - 1.0, ti + 1.0, ext["RTWAT"] - 1.0, ext["RTWAT"] + 1.0, 280.0], dtype=dtype)
        ap[NZ - 1, COL] = ew_numpy(t[NZ - 1:NZ, COL], ext)[0]          # ew / ap = 1 > QMAX: clipped
        rng = np.random.default_rng(11)
        t_i = rng.standard_normal(t.shape).astype(dtype)
        ap_i = (0.01 * ap * rng.standard_normal(t.shape)).astype(dtype)
        q_adj = rng.standard_normal(t.shape).astype(dtype)
        prev = {n: rng.standard_normal(t.shape).astype(dtype) for n in ("ap", "t")}
        qsat, g_t, g_ap, clipped = saturation_derivative(ap, t, ext)
        t64 = t[:NZ].astype(np.float64)
        regimes = {"t = TI - 1": t64[0, COL] == np.float64(dtype(ti - 1.0)), "t = TI + 1": t64[1, COL] == np.float64(dtype(ti + 1.0)),
                   "t = RTWAT - 1": t64[2, COL] == np.float64(dtype(ext["RTWAT"] - 1.0)),
                   "t = RTWAT + 1": t64[3, COL] == np.float64(dtype(ext["RTWAT"] + 1.0)),
                   "below TI": int((t64 < ti).sum()), "between": int(((t64 > ti) & (t64 < ext["RTWAT"])).sum()),
                   "above RTWAT": int((t64 > ext["RTWAT"]).sum()), "clipped at QMAX": int(clipped.sum()),
                   "not clipped": int((~clipped[:NZ]).sum())}
        assert all(int(v) > 0 for v in regimes.values()), regimes
        # (`saturation_derivative` has asserted that its value is the NumPy oracle's to 1e-14 relative)
        assert clipped[NZ - 1, COL] and g_t[NZ - 1, COL] == 0.0 and g_ap[NZ - 1, COL] == 0.0 and qsat[NZ].max() == 0.0
        assert g_t[0, COL] > 0 and g_t[3, COL] > 0 and g_ap[1, COL] < 0
        _cases[key] = dict(ext=ext, ap=ap, t=t, t_i=t_i, ap_i=ap_i, q_adj=q_adj, prev=prev, qsat=qsat, g_t=g_t, g_ap=g_ap,
                           clipped=clipped)
    return _cases[key]


class Dev(Box):
    """the `Box` of the case's geometry, and the pointwise C entries (field pointers, no pointer arrays) on its fields"""

    def __init__(self, gpu, dtype, window):
        super().__init__(NX, NZ, dtype, gpu, window)

    def call(self, name, ext, *args):
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

        p = autodiff._params(ext, NZ)
        ptr = [a.data_ptr() if isinstance(a, self.torch.Tensor) else a for a in args]
        rc = getattr(_lib.load(), f"cloudsc2_{name}_{self.sfx}")(
            ctypes.byref(p), NX, NZ, self.pitch, *ptr, int(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, name)
        return _lib.last_kernel()


def _levels(f):
    a = from_device(f)
    return a[:NZ], a[NZ:]


SHAPES = pytest.mark.parametrize("window", [False, True], ids=["dense", "window"])
CASES = [pytest.mark.parametrize("form", list(FORMS)), pytest.mark.parametrize("dtype", [np.float64, np.float32]), SHAPES]


def _all(marks):
    def deco(fn):
        for m in marks:
            fn = m(fn)
        return pytest.mark.gpu(fn)
    return deco


@_all(CASES)
def test_saturation_tl_is_the_oracles_jvp(gpu, window, dtype, form):
    c, d = _case(dtype, form), Dev(gpu, dtype, window)
    ap, t, ap_i, t_i = (d.put(c[n]) for n in ("ap", "t", "ap_i", "t_i"))
    qsat, qsat_i, ref = d.nan(), d.nan(), d.nan()
    assert d.call("saturation_tl", c["ext"], ap, t, ap_i, t_i, qsat, qsat_i) == "cs2::saturation_tl_kernel"
    d.call("saturation", c["ext"], ap, t, ref)
    d.torch.cuda.synchronize()
    want = c["g_t"] * c["t_i"].astype(np.float64) + c["g_ap"] * c["ap_i"].astype(np.float64)
    got, pad = _levels(qsat_i)
    worst = assert_close("qsat_i", got, want[:NZ].astype(dtype), dtype)
    print(f"saturation_tl {np.dtype(dtype).name} {form}: max scaled error {worst:.2e}")
    assert np.isnan(pad).all() and np.isnan(_levels(qsat)[1]).all(), "level nz written"
    assert (got[c["clipped"][:NZ]] == 0.0).all(), "a point clipped at QMAX has a derivative"
    assert np.array_equal(_levels(qsat)[0], _levels(ref)[0]), "the value is not saturation's bit for bit"
    # absent pointers: the dense call with an explicit zero field, bit for bit; an absent qsat is not written
    zero = d.put(np.zeros_like(c["t"]))
    for a_i, t_ii, a_ptr, t_ptr in ((zero, t_i, None, t_i), (ap_i, zero, ap_i, None)):
        dense, masked, noq = d.nan(), d.nan(), d.nan()
        d.call("saturation_tl", c["ext"], ap, t, a_i, t_ii, qsat, dense)
        d.call("saturation_tl", c["ext"], ap, t, a_ptr, t_ptr, None, masked)
        d.torch.cuda.synchronize()
        assert np.array_equal(_levels(dense)[0], _levels(masked)[0]) and np.isnan(_levels(masked)[1]).all()
    d.call("saturation_tl", c["ext"], ap, t, ap_i, t_i, None, noq)
    d.torch.cuda.synchronize()
    assert np.array_equal(_levels(noq)[0], got)


@_all(CASES)
def test_saturation_ad_is_the_oracles_vjp(gpu, window, dtype, form):
    c, d = _case(dtype, form), Dev(gpu, dtype, window)
    ap, t, q_adj = (d.put(c[n]) for n in ("ap", "t", "q_adj"))
    ap_adj, t_adj = d.nan(), d.nan()
    assert d.call("saturation_ad", c["ext"], ap, t, q_adj, ap_adj, t_adj, 0) == "cs2::saturation_ad_kernel"
    acc = {n: d.put(c["prev"][n]) for n in ("ap", "t")}
    d.call("saturation_ad", c["ext"], ap, t, q_adj, acc["ap"], acc["t"], 1)
    only_t, only_ap, acc_t = d.nan(), d.nan(), d.put(c["prev"]["t"])
    d.call("saturation_ad", c["ext"], ap, t, q_adj, None, only_t, 0)
    d.call("saturation_ad", c["ext"], ap, t, q_adj, only_ap, None, 0)
    d.call("saturation_ad", c["ext"], ap, t, q_adj, None, acc_t, 1)
    d.torch.cuda.synchronize()
    qa = c["q_adj"].astype(np.float64)
    for n, g, got_f, acc_f in (("ap", c["g_ap"], ap_adj, acc["ap"]), ("t", c["g_t"], t_adj, acc["t"])):
        got, pad = _levels(got_f)
        worst = assert_close(n + "_adj", got, (g * qa)[:NZ].astype(dtype), dtype)
        print(f"saturation_ad {np.dtype(dtype).name} {form} {n}: max scaled error {worst:.2e}")
        assert np.isnan(pad).all(), "level nz written"
        assert (got[c["clipped"][:NZ]] == 0.0).all(), "a point clipped at QMAX has a derivative"
        got_acc, pad_acc = _levels(acc_f)
        assert_close(n + "_adj accumulated", got_acc, (c["prev"][n].astype(np.float64) + g * qa)[:NZ].astype(dtype), dtype)
        assert np.array_equal(pad_acc, c["prev"][n][NZ:]), "level nz touched by the accumulation"
    assert np.array_equal(_levels(only_t)[0], _levels(t_adj)[0]) and np.isnan(_levels(only_t)[1]).all()
    assert np.array_equal(_levels(only_ap)[0], _levels(ap_adj)[0]) and np.isnan(_levels(only_ap)[1]).all()
    assert np.array_equal(_levels(acc_t)[0], _levels(acc["t"])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_autograd_through_saturation_gives_the_same_numbers(gpu, dtype, form):
    import torch
    import torch.autograd.forward_ad as fwad

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, saturation
    from helpers import to_device

    c = _case(dtype, form)
    dev = to_device({n: c[n] for n in ("ap", "t", "ap_i", "t_i", "q_adj")}, gpu)
    ap, t = dev["ap"].requires_grad_(True), dev["t"].requires_grad_(True)
    qsat = saturation(ap, t, c["ext"])
    g_ap, g_t = torch.autograd.grad(qsat, [ap, t], dev["q_adj"])
    assert _lib.last_kernel() == "cs2::saturation_ad_kernel"
    g_t_only, = torch.autograd.grad(saturation(ap.detach(), t, c["ext"]).sum(), [t])
    with fwad.dual_level():
        out = saturation(fwad.make_dual(ap.detach(), dev["ap_i"]), fwad.make_dual(t.detach(), dev["t_i"]), c["ext"])
        tangent = fwad.unpack_dual(out).tangent
    assert _lib.last_kernel() == "cs2::saturation_tl_kernel"
    torch.cuda.synchronize()
    qa = c["q_adj"].astype(np.float64)
    assert_close("qsat", from_device(qsat.detach())[:NZ], c["qsat"][:NZ].astype(dtype), dtype)
    assert_close("grad ap", from_device(g_ap)[:NZ], (c["g_ap"] * qa)[:NZ].astype(dtype), dtype)
    assert_close("grad t", from_device(g_t)[:NZ], (c["g_t"] * qa)[:NZ].astype(dtype), dtype)
    assert_close("grad t of sum", from_device(g_t_only)[:NZ], c["g_t"][:NZ].astype(dtype), dtype)
    want_i = c["g_t"] * c["t_i"].astype(np.float64) + c["g_ap"] * c["ap_i"].astype(np.float64)
    assert_close("jvp", from_device(tangent)[:NZ], want_i[:NZ].astype(dtype), dtype)
    for f in (qsat.detach(), g_ap, g_t, tangent):
        assert not from_device(f)[NZ:].any(), "level nz carries a value"
