"""The multi-direction tangent-linear kernels on the GPU (C ABI `cloudsc2_tl_multi_*` / `cloudsc2_tl_multi_step_*`,
`autodiff.tl_multi` / `tl_step_multi`): every direction of every wanted output equals what the single-direction launch
(`tl_masked` / `tl_step`) gives for that direction alone - `assert_close` at its default, and whether it was bit-equal is
printed - the NL outputs are written once and equal `cloudsc2_nl`'s, and nothing else is touched.

Directions are independent: direction d is the `helpers.increments` of a state drawn with another seed, with factor
0.01 (d + 1).  Against the NumPy oracle the perturbations are held to 100 x `assert_close`, as everywhere in the suite
(tests/test_hip_tl_ad.py, tests/test_step_grad.py); for the step family the oracle's TL is chained with the analytic
derivative of `saturation` (tests/saturation_oracle.py), as tests/test_step_grad.py does."""
import numpy as np
import pytest

from derivative_support import SHAPES, STATE4, STEP_IN, TND4, Box, compare_directions, direction_case, raw_tl, singles
from helpers import NL_IN, NL_OUT, assert_close, externals, from_device, nlev_of, run_oracle_tl
from saturation_oracle import saturation_derivative

pytestmark = pytest.mark.gpu

FAMILIES = {"multi": ("cloudsc2_tl_multi", "tl_masked", "cs2::tl_dirs_kernel", NL_IN),
            "step": ("cloudsc2_tl_multi_step", "tl_step", "cs2::tl_dirs_step_kernel", STEP_IN)}


def _max_dirs():
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    return _lib.TL_MAX_DIRS


def _setup(gpu, nx, nz, window, dtype, ndir, **flags):
    import torch

    fields, eta, dt, dirs = direction_case(nx, nz, dtype, ndir)
    box = Box(nx, nz, dtype, gpu, window)
    return box, externals(NLEV=nz, **flags), fields, torch.as_tensor(eta, device=gpu), dt, dirs, box.state(fields)


def _singles(family, state, names, pert, eta, dt, ext, want, ndir):
    """the single-direction launch for each direction alone -> per direction {name: host array}"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    single = FAMILIES[family][1]
    return singles(getattr(autodiff, single), "cs2::" + single + "_kernel", {n: state[n] for n in names}, pert, eta, dt, ext,
                   want, ndir)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nx,nz,window", SHAPES)
def test_full_mask_every_direction_equals_the_single_launch(gpu, nx, nz, window, family, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

    entry, _, kernel, names = FAMILIES[family]
    top = _max_dirs()
    box, ext, fields, eta, dt, dirs, state = _setup(gpu, nx, nz, window, dtype, top)
    pert = {n: box.batch([u[n] for u in dirs]) for n in names}
    rows = _singles(family, state, names, pert, eta, dt, ext, NL_OUT, top)
    for ndir in (1, 2, 3, top):
        out_i = {n: box.nan(top + 1) for n in NL_OUT}
        out = {n: box.nan() for n in NL_OUT} if ndir == 3 else None
        raw_tl(entry, box, ext, state, pert, eta, dt, out, out_i, ndir)
        assert _lib.last_kernel() == kernel
        torch.cuda.synchronize()
        compare_directions(f"{entry} {nx}x{nz}", out_i, rows, NL_OUT, nz, dtype, ndir)
        if out is not None:                       # write_nl: the NL outputs are cloudsc2_nl's (on the step's own qsat)
            nl = {n: box.nan() for n in NL_OUT}
            ins = {"in_" + n: f for n, f in state.items()}
            if family == "step":
                ins["in_qsat"] = box.nan()
                compile_stencil("saturation", ext)(in_ap=state["ap"], in_t=state["t"], out_qsat=ins["in_qsat"],
                                                    origin=(0, 0, 0), domain=(nx, 1, nz), validate_args=True, exec_info=None)
            compile_stencil("cloudsc2_nl", ext)(**ins, **{"out_" + n: f for n, f in nl.items()}, in_eta=eta, dt=dt,
                                                 origin=(0, 0, 0), domain=(nx, 1, nz + 1), validate_args=True, exec_info=None)
            torch.cuda.synchronize()
            for n in NL_OUT:
                k = nlev_of(n, nz)
                assert_close(f"{entry} NL out_{n}", from_device(out[n])[:k], from_device(nl[n])[:k], dtype)


MASKS = {"4dvar": (STATE4, TND4), "aph alone": (("aph",), NL_OUT), "fplsl alone": (NL_IN, ("fplsl",))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("nx,nz,window", [(63, 137, False), (333, 137, True)])
def test_masks(gpu, nx, nz, window, mask, family, dtype):
    """absent perturbations (read from the zero line for every direction) and absent outputs (not written); `aph` feeds the
    carry, `fplsl` is stored one level down and zeroed at the top level"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    entry, _, kernel, names = FAMILIES[family]
    have, want = MASKS[mask]
    have = tuple(n for n in have if n in names)
    ndir = 3
    box, ext, fields, eta, dt, dirs, state = _setup(gpu, nx, nz, window, dtype, ndir)
    pert = {n: box.batch([u[n] for u in dirs]) for n in have}
    rows = _singles(family, state, names, pert, eta, dt, ext, want, ndir)
    out_i = {n: box.nan(ndir + 1) for n in want}
    raw_tl(entry, box, ext, state, pert, eta, dt, None, out_i, ndir)
    assert _lib.last_kernel() == kernel
    torch.cuda.synchronize()
    compare_directions(f"{entry} [{mask}]", out_i, rows, want, nz, dtype, ndir)
    if "fplsl" in want:
        for d in range(ndir):
            assert not from_device(out_i["fplsl"][d])[0].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("flags", [dict(LEVAPLS2=True), dict(LREGCL=False)], ids=["LEVAPLS2", "noLREGCL"])
def test_other_switches(gpu, flags, family, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nx, nz, ndir = 63, 137, 3
    entry, _, kernel, names = FAMILIES[family]
    box, ext, fields, eta, dt, dirs, state = _setup(gpu, nx, nz, False, dtype, ndir, **flags)
    if flags.get("LEVAPLS2"):
        # as everywhere in the suite (tests/test_hip_tl_ad.py): at the drivers' 3600 s the evaporation block's recurrence
        # amplifies by ~3600 per level (the reference's dt**2 quirk) - the oracle's perturbations reach 1e38 for these
        # increments, which no fp32 implementation can hold (single launch and oracle overflow alike); at 60 s they are O(1)
        dt = 60.0
    pert = {n: box.batch([u[n] for u in dirs]) for n in names}
    rows = _singles(family, state, names, pert, eta, dt, ext, NL_OUT, ndir)
    if flags.get("LEVAPLS2"):                     # the block is exercised: the evaporation's cover perturbation is there
        assert all(np.isfinite(r[n]).all() for r in rows for n in NL_OUT) and all(r["covptot"].any() for r in rows)
    out_i = {n: box.nan(ndir) for n in NL_OUT}
    raw_tl(entry, box, ext, state, pert, eta, dt, None, out_i, ndir)
    assert _lib.last_kernel() == kernel
    torch.cuda.synchronize()
    compare_directions(f"{entry} {flags}", out_i, rows, NL_OUT, nz, dtype, ndir)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nx,nz,window", [(200, 137, False), (333, 137, True)])
def test_python_layer_serves_eleven_directions_in_chunks(gpu, nx, nz, window, family, dtype):
    """`tl_multi` / `tl_step_multi` with 11 directions at the full width: a full chunk and a ragged one; at width 5: two
    chunks and a single launch.  The 4D-Var mask; one perturbation arrives in another layout and is copied."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    entry, _, kernel, names = FAMILIES[family]
    ndir = 11
    box, ext, fields, eta, dt, dirs, state = _setup(gpu, nx, nz, window, dtype, ndir)
    st = {n: state[n] for n in names}
    pert = {n: box.batch([u[n] for u in dirs]) for n in STATE4}
    rows = _singles(family, state, names, pert, eta, dt, ext, TND4, ndir)
    given = dict(pert, q=torch.as_tensor(np.stack([u["q"].T[:, None, :] for u in dirs]), device=gpu))   # (ndir, nx, 1, nlev), packed
    call = autodiff.tl_multi if family == "multi" else autodiff.tl_step_multi
    for width, last in ((_max_dirs(), kernel), (5, "cs2::" + FAMILIES[family][1] + "_kernel")):
        nl, out_i = call(st, given, eta, dt, ext, want=TND4, write_nl=True, width=width)
        assert _lib.last_kernel() == last
        torch.cuda.synchronize()
        assert sorted(out_i) == sorted(TND4) and sorted(nl) == sorted(NL_OUT)
        for n in TND4:
            assert tuple(out_i[n].shape) == (ndir, nx, 1, nz + 1)
            for d in range(ndir):
                a = from_device(out_i[n][d])
                assert_close(f"{entry} width {width} out_{n}_i[{d}]", a[:nz], rows[d][n][:nz], dtype)
                assert not a[nz:].any()
        assert not np.isnan(from_device(nl["tnd_t"])[:nz]).any() and from_device(nl["tnd_t"])[:nz].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_directions_equal_the_oracle(gpu, family, dtype):
    import torch

    nx, nz, ndir = 63, 137, 2
    entry, _, kernel, names = FAMILIES[family]
    box, ext, fields, eta, dt, dirs, state = _setup(gpu, nx, nz, False, dtype, ndir)
    pert = {n: box.batch([u[n] for u in dirs]) for n in names}
    out_i = {n: box.nan(ndir) for n in NL_OUT}
    raw_tl(entry, box, ext, state, pert, eta, dt, None, out_i, ndir)
    torch.cuda.synchronize()
    _, g_t, g_ap, _ = saturation_derivative(fields["in_ap"], fields["in_t"], ext)
    for d, u in enumerate(dirs):
        fi = {"in_" + n + "_i": u[n] for n in NL_IN}
        if family == "step":
            fi["in_qsat_i"] = (g_t * u["t"].astype(np.float64) + g_ap * u["ap"].astype(np.float64)).astype(dtype)
        want_i = run_oracle_tl(fields, fi, np.asarray(eta.cpu()), dt, ext)[1]
        for n in NL_OUT:
            k = nlev_of(n, nz)
            assert_close(f"{entry} vs oracle out_{n}_i[{d}]", from_device(out_i[n][d])[:k], want_i[n][:k], dtype, rtol_mul=100.0)
