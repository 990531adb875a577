"""The ensemble kernels on the GPU (C ABI `cloudsc2_{nl,nl_fused,tl,tl_step,ad,ad_step}_ens_*`): every member of every
written field equals what the single launch gives for that member alone - `assert_close` at its default for the dtype, and
whether it was bit-equal is printed, not asserted - and nothing else is touched: the padding level, the gap between members
of a padded member stride and every other slot stay NaN.

Every member is a DIFFERENT seeded case (`nl_case` with seed SEED + 100 + m), so a wrong member base shows; `eta`, which
an ensemble shares, is member 0's.  Perturbations
are the 1 % `increments` of the member's state; the adjoint forcing of a member is the ten perturbed outputs of the single
tangent-linear launch on it, its trajectory fluxes that launch's NL outputs (as tests/test_hip_ad_multi.py).

Bounds: `assert_close` at its default against the single launches; |norm1 - norm2| / (eps |norm2|) < 1e4 per column and
member for the transpose identity (tests/test_hip_ad_multi.py); against the NumPy oracle `assert_close` at its default for
the NL outputs and 100 x for the TL outputs and the adjoints (tests/test_hip_masked.py, tests/test_hip_ad_multi.py), for the
step chained with the analytic derivative of `saturation` (tests/saturation_oracle.py)."""
import numpy as np
import pytest

from derivative_support import SEED, STATE4, STEP_IN, TND4, Box, Ens, ens_ad, ens_nl, ens_tl
from helpers import (NL_IN, NL_OUT, adjoint_nlev_of, assert_close, externals, from_device, increments, nl_case, nlev_of,
                     run_oracle_ad, run_oracle_nl, run_oracle_tl)
from saturation_oracle import saturation_derivative

pytestmark = pytest.mark.gpu

#: (nmem, nx, nz, window, gap): one member and a partial wave; 6 blocks (identity mapping, the last block of each member
#: nearly empty); 8 blocks (XCD remap active); many one-column members; windows of wider allocations (lev_stride > nx);
#: a member stride beyond (nz+1) * lev_stride
SHAPES = [(1, 63, 137, False, 0), (3, 257, 137, False, 0), (4, 300, 137, False, 0), (16, 1, 5, False, 0),
          (2, 130, 40, True, 0), (3, 63, 137, False, 1000)]
_cases = {}


def _members(nmem, nx, nz, dtype):
    """per member: host fields, eta, dt - member m drawn with seed SEED + 100 + m; computed once"""
    key = (nmem, nx, nz, np.dtype(dtype))
    if key not in _cases:
        _cases[key] = [nl_case(nx, nz, dtype=dtype, seed=SEED + 100 + m) for m in range(nmem)]
    return _cases[key]


def compare_members(what, got, rows, names, nz, dtype, levels, ens):
    """member by member against the single launches; the padding level and the gaps between members stay NaN"""
    equal = True
    for n in names:
        k = levels(n, nz)
        for m, row in enumerate(rows):
            a, b = from_device(got[n][m]), row[n]
            assert not np.isnan(a[:k]).any(), (what, n, m)
            assert_close(f"{what} {n}[{m}]", a[:k], b[:k], dtype)
            assert np.isnan(a[k:]).all(), f"{what} {n}[{m}]: padding level written"
            equal = equal and np.array_equal(a[:k], b[:k])
    assert ens.gaps_untouched(), f"{what}: the gap between members was written"
    print(f"{what} nmem={len(rows)} {np.dtype(dtype).name}: bit-equal to the single launches: {equal}")


def _setup(gpu, nmem, nx, nz, window, gap, dtype, **flags):
    import torch

    cases = _members(nmem, nx, nz, dtype)
    box = Box(nx, nz, dtype, gpu, window)
    ext = externals(NLEV=nz, **flags)
    eta, dt = torch.as_tensor(cases[0][1], device=gpu), cases[0][2]
    return cases, box, Ens(box, nmem, gap), ext, eta, dt


def _singles(box, cases, ext, eta, dt, step, have_tl=NL_IN, want_tl=NL_OUT, have_ad=NL_OUT, want_ad=None):
    """the single launches on each member alone -> per member: NL outputs (+ qsat for the step), perturbed outputs,
    host forcing, adjoints - and the kernels that ran"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    names = STEP_IN if step else NL_IN
    tl, ad = (autodiff.tl_step, autodiff.ad_step) if step else (autodiff.tl_masked, autodiff.ad_masked)
    want_ad = names if want_ad is None else tuple(n for n in want_ad if n in names)
    rows = []
    for fields, _, _ in cases:
        st = box.state(fields, names)
        inc = increments(fields, 0.01)
        pert = {n: box.put(inc["in_" + n + "_i"]) for n in have_tl if n in names}
        nl, out_i = tl(st, pert, eta, dt, ext, want=want_tl, write_nl=True)
        assert _lib.last_kernel() == ("cs2::tl_step_kernel" if step else "cs2::tl_masked_kernel")
        full = out_i if set(want_tl) == set(NL_OUT) else tl(
            st, {n: box.put(inc["in_" + n + "_i"]) for n in names}, eta, dt, ext, want=NL_OUT)[1]
        forcing = {n: from_device(full[n]) for n in NL_OUT}
        adj = ad(st, {n: full[n] for n in have_ad}, eta, dt, ext, traj={"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]},
                 want=want_ad)
        assert _lib.last_kernel() == ("cs2::ad_step_kernel" if step else "cs2::ad_masked_kernel")
        rows.append(dict(nl={n: from_device(nl[n]) for n in NL_OUT}, tl={n: from_device(out_i[n]) for n in want_tl},
                         forcing=forcing, ad={n: from_device(adj[n]) for n in want_ad}, inc=inc))
    return names, want_ad, rows


def _run_family(gpu, shape, dtype, step, flags=None, have_tl=NL_IN, want_tl=NL_OUT, have_ad=NL_OUT, want_ad=None):
    """TL and AD ensemble launches of one family against the singles -> (rows, perturbed outputs, adjoints, names)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nmem, nx, nz, window, gap = shape
    cases, box, ens, ext, eta, dt = _setup(gpu, nmem, nx, nz, window, gap, dtype, **(flags or {}))
    names, want_ad, rows = _singles(box, cases, ext, eta, dt, step, have_tl, want_tl, have_ad, want_ad)
    state = {n: ens.put([c[0]["in_" + n] for c in cases]) for n in names}
    pert = {n: ens.put([r["inc"]["in_" + n + "_i"] for r in rows]) for n in have_tl if n in names}
    out, out_i = {n: ens.nan() for n in NL_OUT}, {n: ens.nan() for n in want_tl}
    tag = f"{'step' if step else 'masked'} {shape} {flags or ''}"
    ens_tl("tl_step_ens" if step else "tl_ens", ens, ext, state, pert, eta, dt, out, out_i)
    assert _lib.last_kernel() == ("cs2::tl_ens_step_kernel" if step else "cs2::tl_ens_kernel")
    compare_members(f"tl_ens {tag} out_i", out_i, [r["tl"] for r in rows], want_tl, nz, dtype, nlev_of, ens)
    compare_members(f"tl_ens {tag} out", out, [r["nl"] for r in rows], NL_OUT, nz, dtype, nlev_of, ens)
    forcing = {n: ens.put([r["forcing"][n] for r in rows]) for n in have_ad}
    traj = {n: out[n] for n in ("fplsl", "fplsn")}
    out_adj = {n: ens.nan() for n in want_ad}
    ens_ad("ad_step_ens" if step else "ad_ens", ens, ext, state, forcing, eta, dt, traj, out_adj)
    assert _lib.last_kernel() == ("cs2::ad_ens_step_kernel" if step else "cs2::ad_ens_kernel")
    compare_members(f"ad_ens {tag}", out_adj, [r["ad"] for r in rows], want_ad, nz, dtype, adjoint_nlev_of, ens)
    return rows, out_i, out_adj, names


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_tl_and_ad_every_member_equals_the_single_launch(gpu, shape, step, dtype):
    _run_family(gpu, shape, dtype, step)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_nl_every_member_equals_the_single_launch(gpu, shape, dtype):
    """`cloudsc2_nl_ens` against `cloudsc2_nl`, `cloudsc2_nl_fused_ens` against `cloudsc2_nl_saturation` (qsat included)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nmem, nx, nz, window, gap = shape
    cases, box, ens, ext, eta, dt = _setup(gpu, nmem, nx, nz, window, gap, dtype)
    plain, fused = [], []
    for fields, _, _ in cases:
        st = box.state(fields)
        outs = {n: box.nan() for n in NL_OUT}
        box.stencil("cloudsc2_nl", ext, eta, dt, **{"in_" + n: f for n, f in st.items()}, **{"out_" + n: f for n, f in outs.items()})
        plain.append({n: from_device(outs[n]) for n in NL_OUT})
        outs, qsat = {n: box.nan() for n in NL_OUT}, box.nan()
        box.stencil("cloudsc2_nl_saturation", ext, eta, dt, **{"in_" + n: f for n, f in st.items() if n != "qsat"}, out_qsat=qsat,
                    **{"out_" + n: f for n, f in outs.items()})
        fused.append(dict({n: from_device(outs[n]) for n in NL_OUT}, qsat=from_device(qsat)))
    state = {n: ens.put([c[0]["in_" + n] for c in cases]) for n in NL_IN}
    out = {n: ens.nan() for n in NL_OUT}
    ens_nl(ens, ext, state, eta, dt, out)
    assert _lib.last_kernel() == "cs2::nl_ens_kernel"
    compare_members(f"nl_ens {shape}", out, plain, NL_OUT, nz, dtype, nlev_of, ens)
    out, qsat = {n: ens.nan() for n in NL_OUT}, ens.nan()
    ens_nl(ens, ext, {n: f for n, f in state.items() if n != "qsat"}, eta, dt, out, qsat)
    assert _lib.last_kernel() == "cs2::nl_ens_kernel<saturation>"
    compare_members(f"nl_fused_ens {shape}", dict(out, qsat=qsat), fused, NL_OUT + ("qsat",), nz, dtype, nlev_of, ens)


#: name -> (perturbations present, perturbed outputs wanted, forcing present, adjoints wanted)
MASKS = {"4dvar": (STATE4, TND4, TND4, STATE4), "single field": (("t",), ("tnd_q",), ("fplsl",), ("aph",))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_masks(gpu, mask, step, dtype):
    """absent inputs are read from the zero line by every member (they behave as zeros: the single launch's result),
    unwanted outputs are not written"""
    have_tl, want_tl, have_ad, want_ad = MASKS[mask]
    _run_family(gpu, (3, 257, 137, False, 0), dtype, step, None, have_tl, want_tl, have_ad, want_ad)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("flags", [dict(AD_TRAJ_FIX=0), dict(AD_TRAJ_FIX=1), dict(LREGCL=False)], ids=["FIX0", "FIX1", "noLREGCL"])
def test_other_switches(gpu, flags, step, dtype):
    _run_family(gpu, (3, 63, 137, False, 0), dtype, step, flags)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
def test_ad_ens_is_the_transpose_of_tl_ens(gpu, step, dtype):
    """<J u, J u> == <u, J^T (J u)> per column and member (AD_TRAJ_FIX = 1); `supsat` is not perturbed, as in
    tests/test_hip_ad_multi.py (its adjoint is the reference's literal dt x the q adjoint, not the transpose)"""
    shape = (3, 63, 137, False, 0)
    names = tuple(n for n in (STEP_IN if step else NL_IN) if n != "supsat")
    rows, w, adj, _ = _run_family(gpu, shape, dtype, step, dict(AD_TRAJ_FIX=1), have_tl=names, want_ad=names)
    for m, r in enumerate(rows):
        # the levels a launch writes: the padding level of these buffers is still NaN
        norm1 = sum((from_device(w[n][m])[:nlev_of(n, 137)].astype(np.float64) ** 2).sum(axis=0) for n in NL_OUT)
        norm2 = sum((r["inc"]["in_" + n + "_i"][:adjoint_nlev_of(n, 137)].astype(np.float64)
                     * from_device(adj[n][m])[:adjoint_nlev_of(n, 137)].astype(np.float64)).sum(axis=0) for n in names)
        assert (norm2 != 0).all()
        norm3 = np.abs(norm1 - norm2) / (np.finfo(dtype).eps * np.abs(norm2))
        print(f"ens transpose identity step={step} {np.dtype(dtype).name} member {m}: max {norm3.max():.3e} x eps")
        assert (norm3 < 1e4).all(), (m, float(norm3.max()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
def test_members_equal_the_oracle(gpu, step, dtype):
    """NL outputs, perturbed outputs and adjoints of every member held directly against the NumPy oracle (for the step
    chained with saturation's analytic derivative), so that "equals the single launch" does not rest on the product alone"""
    shape = (2, 63, 137, False, 0)
    nmem, nx, nz, _, _ = shape
    ext = externals(NLEV=nz, AD_TRAJ_FIX=1)
    cases, box, ens, _, eta, dt = _setup(gpu, nmem, nx, nz, False, 0, dtype, AD_TRAJ_FIX=1)
    names = STEP_IN if step else NL_IN
    want = []
    eta_h, dt_h = cases[0][1], cases[0][2]      # `eta` is shared by the members: member 0's
    for fields, _, _ in cases:
        inc = increments(fields, 0.01)
        _, g_t, g_ap, _ = saturation_derivative(fields["in_ap"], fields["in_t"], ext)
        if step:       # the qsat perturbation is saturation's derivative applied to those of t and ap
            inc = dict(inc, in_qsat_i=(g_t * inc["in_t_i"].astype(np.float64) + g_ap * inc["in_ap_i"].astype(np.float64)).astype(dtype))
        nl0 = run_oracle_nl(fields, eta_h, dt_h, ext)
        tl_i = run_oracle_tl(fields, inc, eta_h, dt_h, ext)[1]
        adj = dict(run_oracle_ad(fields, tl_i, eta_h, dt_h, ext, traj=nl0)[1])
        if step:
            adj["t"] = (adj["t"].astype(np.float64) + g_t * adj["qsat"].astype(np.float64)).astype(dtype)
            adj["ap"] = (adj["ap"].astype(np.float64) + g_ap * adj["qsat"].astype(np.float64)).astype(dtype)
        want.append(dict(nl=nl0, tl=tl_i, ad=adj, inc=increments(fields, 0.01)))
    state = {n: ens.put([c[0]["in_" + n] for c in cases]) for n in names}
    pert = {n: ens.put([w["inc"]["in_" + n + "_i"] for w in want]) for n in names}
    out, out_i = {n: ens.nan() for n in NL_OUT}, {n: ens.nan() for n in NL_OUT}
    ens_tl("tl_step_ens" if step else "tl_ens", ens, ext, state, pert, eta, dt, out, out_i)
    forcing = {n: ens.put([w["tl"][n] for w in want]) for n in NL_OUT}
    out_adj = {n: ens.nan() for n in names}
    ens_ad("ad_step_ens" if step else "ad_ens", ens, ext, state, forcing, eta, dt, {n: out[n] for n in ("fplsl", "fplsn")}, out_adj)
    nl_out = {n: ens.nan() for n in NL_OUT}
    if step:
        ens_nl(ens, ext, state, eta, dt, nl_out, ens.nan())
    else:
        ens_nl(ens, ext, state, eta, dt, nl_out)
    failures = []
    for m, w in enumerate(want):
        for what, got, ref, lev, mul in (("nl", nl_out, w["nl"], nlev_of, 1.0), ("tl", out_i, w["tl"], nlev_of, 100.0),
                                        ("ad", out_adj, w["ad"], adjoint_nlev_of, 100.0)):
            for n in got:
                k = lev(n, nz)
                try:
                    assert_close(f"{what}_ens vs oracle {n}[{m}]", from_device(got[n][m])[:k], ref[n][:k], dtype, rtol_mul=mul)
                except AssertionError as exc:
                    failures.append(str(exc))
    assert not failures, "\n".join(failures)
