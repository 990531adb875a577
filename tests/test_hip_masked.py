"""The masked TL / AD kernels on the GPU (`autodiff.tl_masked` / `ad_masked`, C ABI `cloudsc2_*_masked_*`): a field that is
written equals what the dense kernel writes for the same inputs with zeros in place of the absent fields - AD bit for bit
(the arithmetic of `cloudsc2_ad_from_trajectory`), TL to rounding - and a field that is absent is not touched.

Comparisons with the NumPy oracle use `assert_close` with the factors the suite already holds these fields to
(tests/test_hip_tl_ad.py: 100 x for TL perturbations, 1000 x for adjoints - both are differences of nearly equal terms)."""
import numpy as np
import pytest

from derivative_support import (SHAPES, STATE4, TND4, Box, host_case, host_increments, oracle_nl, oracle_tl_i, raw_ad,
                                raw_tl)
from helpers import (NL_IN, NL_OUT, assert_close, externals, from_device, increments, nl_case, nlev_of, run_oracle_ad,
                     run_oracle_tl)

pytestmark = pytest.mark.gpu


def _setup(gpu, nx, nz, window, dtype, **flags):
    import torch

    fields, eta, dt = host_case(nx, nz, dtype)
    box = Box(nx, nz, dtype, gpu, window)
    ext = externals(NLEV=nz, **flags)
    return box, ext, fields, torch.as_tensor(eta, device=gpu), dt, host_increments(nx, nz, dtype), box.state(fields)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("nx,nz,window", SHAPES)
def test_full_mask_ad_is_bit_equal_to_the_trajectory_kernel(gpu, nx, nz, window, fix, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    box, ext, fields, eta, dt, fi, state = _setup(gpu, nx, nz, window, dtype, AD_TRAJ_FIX=fix)
    traj = box.nl_fluxes(state, ext, eta, dt)
    tl_i = oracle_tl_i(nx, nz, dtype)
    forcing = {n: box.put(tl_i[n]) for n in NL_OUT}
    want = box.dense_ad_traj(state, forcing, traj, ext, eta, dt)
    assert _lib.last_kernel() == "cs2::ad_kernel<trajectory>"
    got = autodiff.ad_masked(state, forcing, eta, dt, ext, traj=traj, want=NL_IN)
    assert _lib.last_kernel() == "cs2::ad_masked_kernel"
    torch.cuda.synchronize()
    for n in NL_IN:
        k = nz + 1 if n in ("aph", "lu") else nz
        a, b = from_device(got[n])[:k], from_device(want[n])[:k]
        assert not np.isnan(a).any(), n
        assert np.array_equal(a, b), (n, float(np.abs(a - b).max()))
        assert not from_device(got[n])[k:].any(), f"{n}: padding level written"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nx,nz,window", SHAPES)
def test_full_mask_tl_agrees_with_the_dense_kernel(gpu, nx, nz, window, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    box, ext, fields, eta, dt, fi, state = _setup(gpu, nx, nz, window, dtype)
    pert = {n: box.put(fi["in_" + n + "_i"]) for n in NL_IN}
    want, want_i = box.dense_tl(state, pert, ext, eta, dt)
    got, got_i = autodiff.tl_masked(state, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    assert _lib.last_kernel() == "cs2::tl_masked_kernel"
    torch.cuda.synchronize()
    for n in NL_OUT:
        k = nlev_of(n, nz)
        assert_close(f"tl_masked out_{n}", from_device(got[n])[:k], from_device(want[n])[:k], dtype)
        assert_close(f"tl_masked out_{n}_i", from_device(got_i[n])[:k], from_device(want_i[n])[:k], dtype, rtol_mul=100.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("nx,nz,window", [(200, 137, False), (333, 137, True)])
def test_4dvar_mask_ad_is_bit_equal_to_dense_with_explicit_zeros(gpu, nx, nz, window, fix, dtype):
    import torch

    box, ext, fields, eta, dt, fi, state = _setup(gpu, nx, nz, window, dtype, AD_TRAJ_FIX=fix)
    traj = box.nl_fluxes(state, ext, eta, dt)
    tl_i = oracle_tl_i(nx, nz, dtype)
    forcing = {n: box.put(tl_i[n]) for n in TND4}
    want = box.dense_ad_traj(state, {n: forcing.get(n) if n in forcing else box.zeros() for n in NL_OUT}, traj, ext, eta, dt)
    bufs = {n: box.nan() for n in NL_IN}                   # every buffer NaN-prefilled; only the wanted four are passed
    raw_ad("cloudsc2_ad_masked", box, ext, state, forcing, eta, dt, traj, {n: bufs[n] for n in STATE4})
    torch.cuda.synchronize()
    for n in NL_IN:
        a = from_device(bufs[n])
        if n in STATE4:
            assert np.array_equal(a[:nz], from_device(want[n])[:nz]), n
            assert np.isnan(a[nz:]).all(), f"{n}: padding level written"
        else:
            assert np.isnan(a).all(), f"{n}: an absent output was written"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nx,nz,window", [(200, 137, False), (333, 137, True)])
def test_4dvar_mask_tl_matches_the_oracle_fed_explicit_zeros(gpu, nx, nz, window, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    box, ext, fields, eta, dt, fi, state = _setup(gpu, nx, nz, window, dtype)
    zeros_i = {k: (v if k[3:-2] in STATE4 else np.zeros_like(v)) for k, v in fi.items()}
    _, want_i = run_oracle_tl(fields, zeros_i, host_case(nx, nz, dtype)[1], dt, ext)
    pert = {n: box.put(fi["in_" + n + "_i"]) for n in STATE4}
    out, got_i = autodiff.tl_masked(state, pert, eta, dt, ext, want=TND4)
    # and the entry itself on NaN-prefilled buffers: the six absent `out_i` and the ten absent `out` must stay untouched
    bufs, nl_bufs = {n: box.nan() for n in NL_OUT}, {n: box.nan() for n in NL_OUT}
    raw_tl("cloudsc2_tl_masked", box, ext, state, pert, eta, dt, None, {n: bufs[n] for n in TND4})
    torch.cuda.synchronize()
    assert out is None and sorted(got_i) == sorted(TND4)
    for n in TND4:
        assert_close(f"tl_masked 4dvar out_{n}_i", from_device(got_i[n])[:nz], want_i[n][:nz], dtype, rtol_mul=100.0)
        assert not from_device(got_i[n])[nz:].any()
    for n in NL_OUT:
        a = from_device(bufs[n])
        if n in TND4:
            assert np.array_equal(a[:nz], from_device(got_i[n])[:nz]), n
            assert np.isnan(a[nz:]).all(), f"{n}: padding level written"
        else:
            assert np.isnan(a).all(), f"out_{n}_i: an absent output was written"
        assert np.isnan(from_device(nl_bufs[n])).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NL_OUT)
def test_each_forcing_alone_matches_the_oracle_adjoint(gpu, name, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    nx, nz = 200, 137
    box, ext, fields, eta, dt, fi, state = _setup(gpu, nx, nz, False, dtype, AD_TRAJ_FIX=1)
    nl0 = oracle_nl(nx, nz, dtype)
    tl_i = oracle_tl_i(nx, nz, dtype)
    forcing = {n: (tl_i[n] if n == name else np.zeros_like(tl_i[n])) for n in NL_OUT}
    _, want = run_oracle_ad(fields, forcing, host_case(nx, nz, dtype)[1], dt, ext, traj=nl0)
    traj = box.nl_fluxes(state, ext, eta, dt)
    got = autodiff.ad_masked(state, {name: box.put(tl_i[name])}, eta, dt, ext, traj=traj, want=NL_IN)
    torch.cuda.synchronize()
    for n in NL_IN:
        k = nz + 1 if n in ("aph", "lu") else nz
        assert_close(f"ad_masked[{name}] out_{n}_i", from_device(got[n])[:k], want[n][:k], dtype, rtol_mul=1000.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NL_IN)
def test_each_perturbation_alone_matches_the_oracle_tl(gpu, name, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    nx, nz = 200, 137
    box, ext, fields, eta, dt, fi, state = _setup(gpu, nx, nz, False, dtype)
    one = {k: (v if k == "in_" + name + "_i" else np.zeros_like(v)) for k, v in fi.items()}
    _, want_i = run_oracle_tl(fields, one, host_case(nx, nz, dtype)[1], dt, ext)
    _, got_i = autodiff.tl_masked(state, {name: box.put(fi["in_" + name + "_i"])}, eta, dt, ext, want=NL_OUT)
    torch.cuda.synchronize()
    for n in NL_OUT:
        k = nlev_of(n, nz)
        assert_close(f"tl_masked[{name}] out_{n}_i", from_device(got_i[n])[:k], want_i[n][:k], dtype, rtol_mul=100.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nx,nz,window,seed", [(200, 137, False, 20240807), (333, 137, True, 7), (130, 40, False, 11)])
def test_dot_product_identity_on_masked_sets(gpu, nx, nz, window, seed, dtype):
    """<TL h, TL h> == <h, AD TL h> per column, perturbing t, q, ql, qi by 1 % and forcing with the TL tendencies only - the
    reference's symmetry rule (|norm1 - norm2| / (eps norm2) < 1e4 per column), AD_TRAJ_FIX = 1."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    fields, eta_h, dt = nl_case(nx, nz, dtype=dtype, seed=seed)
    fi = increments(fields, 0.01)
    box = Box(nx, nz, dtype, gpu, window)
    ext = externals(NLEV=nz, AD_TRAJ_FIX=1)
    eta = torch.as_tensor(eta_h, device=gpu)
    state = box.state(fields)
    pert = {n: box.put(fi["in_" + n + "_i"]) for n in STATE4}
    nl, tl_i = autodiff.tl_masked(state, pert, eta, dt, ext, want=TND4, write_nl=True)
    adj = autodiff.ad_masked(state, tl_i, eta, dt, ext, traj={"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}, want=STATE4)
    torch.cuda.synchronize()
    norm1 = sum((from_device(tl_i[n]).astype(np.float64)[:nz] ** 2).sum(axis=0) for n in TND4)
    norm2 = sum((fi["in_" + n + "_i"].astype(np.float64)[:nz] * from_device(adj[n]).astype(np.float64)[:nz]).sum(axis=0)
                for n in STATE4)
    assert (norm2 != 0).all()
    norm3 = np.abs(norm1 - norm2) / (np.finfo(dtype).eps * np.abs(norm2))
    print(f"masked symmetry nx={nx} nz={nz} {np.dtype(dtype).name}: max {norm3.max():.3e} x eps")
    assert (norm3 < 1e4).all(), (int((norm3 >= 1e4).sum()), float(norm3.max()))
