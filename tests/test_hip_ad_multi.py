"""The multi-direction adjoint kernels on the GPU (C ABI `cloudsc2_ad_multi_*` / `cloudsc2_ad_multi_step_*`,
`autodiff.ad_multi` / `ad_step_multi`): every direction of every wanted adjoint equals what the single-direction launch
(`ad_masked` / `ad_step`) gives for that cotangent alone - `assert_close` at its default, and whether it was bit-equal is
printed - and nothing else is touched.

Directions are independent: direction d is the `helpers.increments` of a state drawn with another seed, with factor
0.01 (d + 1), as in tests/test_hip_tl_multi.py; the adjoint forcing of direction d is the ten perturbed outputs of the
single tangent-linear launch (`tl_masked` / `tl_step`) on direction d, which keeps the magnitudes physical.  The trajectory
fluxes are that launch's NL outputs.

Bounds: |norm1 - norm2| / (eps |norm2|) < 1e4 per column and direction for the transpose identity against `tl_multi`
(tests/test_step_grad.py); 100 x `assert_close` against the NumPy oracle, for the step family chained with the analytic
derivative of `saturation` (tests/saturation_oracle.py) as tests/test_step_grad.py does."""
import numpy as np
import pytest

from derivative_support import SHAPES, STATE4, STEP_IN, TND4, Box, compare_directions, direction_case, raw_ad, singles
from helpers import (NL_IN, NL_OUT, adjoint_nlev_of, assert_close, externals, from_device, run_oracle_ad, run_oracle_nl,
                     run_oracle_tl)
from saturation_oracle import saturation_derivative

pytestmark = pytest.mark.gpu

#: family -> (C entry, single AD call, its kernel, multi kernel, input names, single TL call, multi TL call)
FAMILIES = {"multi": ("cloudsc2_ad_multi", "ad_masked", "cs2::ad_masked_kernel", "cs2::ad_dirs_kernel", NL_IN, "tl_masked",
                      "tl_multi"),
            "step": ("cloudsc2_ad_multi_step", "ad_step", "cs2::ad_step_kernel", "cs2::ad_dirs_step_kernel", STEP_IN, "tl_step",
                     "tl_step_multi")}


def _max_dirs():
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    return _lib.AD_MAX_DIRS


def _setup(gpu, family, nx, nz, window, dtype, ndir, **flags):
    """-> box, externals, eta, dt, dirs, the family's state, its trajectory fluxes, per direction the host forcing
    {NL_OUT name: [level][column]} = the single tangent-linear launch's perturbed outputs for direction d"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    fields, eta, dt, dirs = direction_case(nx, nz, dtype, ndir)
    box = Box(nx, nz, dtype, gpu, window)
    names = FAMILIES[family][4]
    st = box.state(fields, names)
    ext = externals(NLEV=nz, **flags)
    eta = torch.as_tensor(eta, device=gpu)
    tl = getattr(autodiff, FAMILIES[family][5])
    traj, forcing = None, []
    for d, u in enumerate(dirs):
        nl, out_i = tl(st, {n: box.put(u[n]) for n in names}, eta, dt, ext, want=NL_OUT, write_nl=d == 0)
        if d == 0:
            traj = {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}
        forcing.append({n: from_device(out_i[n]) for n in NL_OUT})
    return box, ext, eta, dt, dirs, st, traj, forcing


def _singles(family, state, forcing, eta, dt, ext, traj, want, ndir):
    """the single-direction launch for each cotangent alone -> per direction {name: host array}"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    return singles(getattr(autodiff, FAMILIES[family][1]), FAMILIES[family][2], state, forcing, eta, dt, ext, want, ndir,
                   traj=traj)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nx,nz,window", SHAPES)
def test_full_mask_every_direction_equals_the_single_launch(gpu, nx, nz, window, family, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    entry, _, _, kernel, names, _, _ = FAMILIES[family]
    top = _max_dirs()
    box, ext, eta, dt, dirs, st, traj, w = _setup(gpu, family, nx, nz, window, dtype, top)
    forcing = {n: box.batch([w[d][n] for d in range(top)]) for n in NL_OUT}
    rows = _singles(family, st, forcing, eta, dt, ext, traj, names, top)
    assert all(r["t"][:nz].any() and r["aph"].any() for r in rows)
    for ndir in (1, 2, 3, top):
        out_adj = {n: box.nan(top + 1) for n in names}
        raw_ad(entry, box, ext, st, forcing, eta, dt, traj, out_adj, ndir)
        assert _lib.last_kernel() == kernel
        torch.cuda.synchronize()
        compare_directions(f"{entry} {nx}x{nz}", out_adj, rows, names, nz, dtype, ndir, levels=adjoint_nlev_of)


#: name -> (forcing present, adjoints wanted)
MASKS = {"4dvar": (TND4, STATE4), "fplsl alone": (("fplsl",), NL_IN), "aph alone": (NL_OUT, ("aph",)), "lu alone": (NL_OUT, ("lu",))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("nx,nz,window", [(63, 137, False), (333, 137, True)])
def test_masks(gpu, nx, nz, window, mask, family, dtype):
    """absent forcing (read from the zero line for every direction) and unwanted adjoints (not written).  `fplsl` enters
    one level down; `aph` alone exercises the carry and the per-direction store of the top half level, whose value is the
    single launch's daph_i - dp_i; the top half level of `lu` is zero in every direction"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    entry, _, _, kernel, names, _, _ = FAMILIES[family]
    have, want = MASKS[mask]
    want = tuple(n for n in want if n in names)
    ndir = 3
    box, ext, eta, dt, dirs, st, traj, w = _setup(gpu, family, nx, nz, window, dtype, ndir)
    forcing = {n: box.batch([w[d][n] for d in range(ndir)]) for n in have}
    rows = _singles(family, st, forcing, eta, dt, ext, traj, want, ndir)
    out_adj = {n: box.nan(ndir + 1) for n in want}
    raw_ad(entry, box, ext, st, forcing, eta, dt, traj, out_adj, ndir)
    assert _lib.last_kernel() == kernel
    torch.cuda.synchronize()
    compare_directions(f"{entry} [{mask}]", out_adj, rows, want, nz, dtype, ndir, levels=adjoint_nlev_of)
    for d in range(ndir):
        if "aph" in want:
            top = from_device(out_adj["aph"][d])[0]
            assert_close(f"{entry} [{mask}] top half level of aph[{d}]", top, rows[d]["aph"][0], dtype,
                         scale=float(np.abs(rows[d]["aph"]).max()))
        if "lu" in want:
            assert not from_device(out_adj["lu"][d])[0].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("flags", [dict(AD_TRAJ_FIX=0), dict(AD_TRAJ_FIX=1), dict(LREGCL=False)],
                         ids=["FIX0", "FIX1", "noLREGCL"])
def test_other_switches(gpu, flags, family, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nx, nz, ndir = 63, 137, 3
    entry, _, _, kernel, names, _, _ = FAMILIES[family]
    box, ext, eta, dt, dirs, st, traj, w = _setup(gpu, family, nx, nz, False, dtype, ndir, **flags)
    forcing = {n: box.batch([w[d][n] for d in range(ndir)]) for n in NL_OUT}
    rows = _singles(family, st, forcing, eta, dt, ext, traj, names, ndir)
    out_adj = {n: box.nan(ndir) for n in names}
    raw_ad(entry, box, ext, st, forcing, eta, dt, traj, out_adj, ndir)
    assert _lib.last_kernel() == kernel
    torch.cuda.synchronize()
    compare_directions(f"{entry} {flags}", out_adj, rows, names, nz, dtype, ndir, levels=adjoint_nlev_of)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nx,nz,window", [(200, 137, False), (333, 137, True)])
def test_python_layer_serves_eleven_directions_in_chunks(gpu, nx, nz, window, family, dtype):
    """`ad_multi` / `ad_step_multi` with 11 cotangents at the full width: a full chunk and a ragged one; at width 5: two
    chunks and a single launch.  The 4D-Var mask; one forcing arrives in another layout and is copied."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    entry, _, single_kernel, kernel, names, _, _ = FAMILIES[family]
    ndir = 11
    box, ext, eta, dt, dirs, st, traj, w = _setup(gpu, family, nx, nz, window, dtype, ndir)
    forcing = {n: box.batch([w[d][n] for d in range(ndir)]) for n in TND4}
    rows = _singles(family, st, forcing, eta, dt, ext, traj, STATE4, ndir)
    given = dict(forcing, tnd_q=torch.as_tensor(np.stack([w[d]["tnd_q"].T[:, None, :] for d in range(ndir)]), device=gpu))  # packed
    call = autodiff.ad_multi if family == "multi" else autodiff.ad_step_multi
    for width, last in ((_max_dirs(), kernel), (5, single_kernel)):
        adj = call(st, given, eta, dt, ext, traj=traj, want=STATE4, width=width)
        assert _lib.last_kernel() == last
        torch.cuda.synchronize()
        assert sorted(adj) == sorted(STATE4)
        for n in STATE4:
            assert tuple(adj[n].shape) == (ndir, nx, 1, nz + 1)
            for d in range(ndir):
                a = from_device(adj[n][d])
                assert_close(f"{entry} width {width} out_{n}_i[{d}]", a[:nz], rows[d][n][:nz], dtype)
                assert not a[nz:].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ad_multi_is_the_transpose_of_tl_multi(gpu, family, dtype):
    """<J u_d, J u_d> == <u_d, J^T (J u_d)> per column and direction, J u_d from the multi-direction tangent-linear,
    J^T from the multi-direction adjoint (AD_TRAJ_FIX = 1: the adjoint is the exact transpose).  `supsat` is not perturbed,
    as in the reference's symmetry test and in tests/test_hip_tl_ad.py: its adjoint is the reference's literal dt x the q
    adjoint (quirk Q7), not the transpose, and a column with supsat != 0 misses the identity by 1e14 x eps with it."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    nx, nz, ndir = 63, 137, 3
    entry, _, _, kernel, names, _, tl_multi = FAMILIES[family]
    fields, eta, dt, dirs = direction_case(nx, nz, dtype, ndir)
    box = Box(nx, nz, dtype, gpu, False)
    st = {n: box.put(fields["in_" + n]) for n in names}
    ext = externals(NLEV=nz, AD_TRAJ_FIX=1)
    eta = torch.as_tensor(eta, device=gpu)
    names = tuple(n for n in names if n != "supsat")
    pert = {n: box.batch([u[n] for u in dirs]) for n in names}
    nl, w = getattr(autodiff, tl_multi)(st, pert, eta, dt, ext, want=NL_OUT, write_nl=True, width=_lib.TL_MAX_DIRS)
    call = autodiff.ad_multi if family == "multi" else autodiff.ad_step_multi
    adj = call(st, w, eta, dt, ext, traj={"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}, want=names, width=_max_dirs())
    assert _lib.last_kernel() == kernel
    torch.cuda.synchronize()
    for d, u in enumerate(dirs):
        norm1 = sum((from_device(w[n][d]).astype(np.float64) ** 2).sum(axis=0) for n in NL_OUT)
        norm2 = sum((u[n].astype(np.float64) * from_device(adj[n][d]).astype(np.float64)).sum(axis=0) for n in names)
        assert (norm2 != 0).all()
        norm3 = np.abs(norm1 - norm2) / (np.finfo(dtype).eps * np.abs(norm2))
        print(f"{entry} transpose identity {np.dtype(dtype).name} direction {d}: max {norm3.max():.3e} x eps")
        assert (norm3 < 1e4).all(), (d, float(norm3.max()))


_oracle = {}


def _oracle_case(dtype, ndir):
    """host forcing (the oracle's TL outputs of each direction) and the oracle's adjoints for it, on the oracle's own
    trajectory fluxes, with the chain through `saturation` for the step family: computed once per precision"""
    key = np.dtype(dtype)
    if key not in _oracle:
        nx, nz = 63, 137
        fields, eta, dt, dirs = direction_case(nx, nz, dtype, ndir)
        ext = externals(NLEV=nz, AD_TRAJ_FIX=1)
        nl0 = run_oracle_nl(fields, eta, dt, ext)
        _, g_t, g_ap, _ = saturation_derivative(fields["in_ap"], fields["in_t"], ext)
        forcing, want = [], []
        for u in dirs:
            tl_i = run_oracle_tl(fields, {"in_" + n + "_i": u[n] for n in NL_IN}, eta, dt, ext)[1]
            adj = run_oracle_ad(fields, tl_i, eta, dt, ext, traj=nl0)[1]
            step = dict(adj)
            step["t"] = (adj["t"].astype(np.float64) + g_t * adj["qsat"].astype(np.float64)).astype(dtype)
            step["ap"] = (adj["ap"].astype(np.float64) + g_ap * adj["qsat"].astype(np.float64)).astype(dtype)
            forcing.append(tl_i)
            want.append({"multi": adj, "step": step})
        _oracle[key] = (forcing, want)
    return _oracle[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_directions_equal_the_oracle(gpu, family, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    nx, nz, ndir = 63, 137, 2
    entry, _, _, kernel, names, tl_single, _ = FAMILIES[family]
    w, want = _oracle_case(dtype, ndir)
    fields, eta, dt, dirs = direction_case(nx, nz, dtype, ndir)
    box = Box(nx, nz, dtype, gpu, False)
    st = {n: box.put(fields["in_" + n]) for n in names}
    ext = externals(NLEV=nz, AD_TRAJ_FIX=1)
    eta = torch.as_tensor(eta, device=gpu)
    # the trajectory fluxes are the device's own NL outputs (written by a tangent-linear launch on direction 0)
    nl, _ = getattr(autodiff, tl_single)(st, {"t": box.put(dirs[0]["t"])}, eta, dt, ext, want=("tnd_t",), write_nl=True)
    forcing = {n: box.batch([w[d][n] for d in range(ndir)]) for n in NL_OUT}
    out_adj = {n: box.nan(ndir) for n in names}
    raw_ad(entry, box, ext, st, forcing, eta, dt, {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}, out_adj, ndir)
    torch.cuda.synchronize()
    failures = []
    for d in range(ndir):
        for n in names:
            k = adjoint_nlev_of(n, nz)
            a, b = from_device(out_adj[n][d])[:k], want[d][family][n][:k]
            scale = float(np.abs(b).max())
            print(f"{entry} vs oracle {np.dtype(dtype).name} out_{n}_i[{d}]: max |err| / scale "
                  f"{float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / scale if scale else 0.0:.3e}")
            try:
                assert_close(f"{entry} vs oracle out_{n}_i[{d}]", a, b, dtype, rtol_mul=100.0)
            except AssertionError as exc:
                failures.append(str(exc))
    assert not failures, "\n".join(failures)
