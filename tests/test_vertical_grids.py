"""NL / TL / AD on vertical grids other than the synthetic one.

`synthetic.eta_levels` is the same for every seed (the seed moves the surface pressure only, which cancels in
ap / aph[nz]), and no other test passes an `eta` of its own - so the tropopause logic, which depends on nothing but `eta`
(`build_level_table`, `trpaus_prescan`, `trpaus_prescan_multi`, the overlapped pre-scan of `nl_ring_kernel`), has met one
geometry per level count, all three on the overlapped branch.  `grid_support.eta_family` puts the window [klo, khi] of
levels with 0.1 < eta < 0.4 everywhere else: at the top, at the bottom, nowhere, on both sides of the hand-over
nps == klo, on the chunk tail of the pre-scan, with holes, and with T(0.1) / T(0.4) themselves next to it.

float32 and `edge_values`: the kernels compare eta with T(0.1) and T(0.4), so float32(0.1) is NOT > 0.1.  That is the
reference's float32 meaning - a literal takes the field type (tests/golden/gtscript_exec.py) - and what the oracle does
under NumPy 2's promotion rules, where a Python float beside a float32 value is a float32 (`tropopause_window` spells it
out with T(0.1)); under value-based promotion float32(0.1) > 0.1 would hold in double.

Every kernel family that reads `eta` is held to the NumPy oracle: `assert_close` at its default for NL outputs, 100 x for
TL outputs and adjoints (grid_support.py), and the kernel that ran is asserted per case."""
import numpy as np
import pytest

from grid_support import (CORE_GRIDS, Held, eta_family, grid_case, hold_dense, hold_ensemble, hold_masked, hold_multi, hold_nl,
                          hold_perturbed, tropopause_window)
from helpers import eta_levels

ALL_GRIDS = ("synthetic", "uniform", "no_window_above", "no_window_below", "all_inside", "bottom_up", "nps_eq_klo",
             "nps_eq_klo_plus_1", "edge_values", "chunk_tail", "hole", "hole_overlapped")
#: the whole family at nz = 40, the grids that move the window's ends and the hand-over at the other level counts
CASES = [(40, g) for g in ALL_GRIDS] + [(nz, g) for nz in (137, 12) for g in CORE_GRIDS]
DTYPES = [np.float64, np.float32]


# ----------------------------------------------------------------------------------------------
# CPU: what the family contains
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_synthetic_grid_is_one_overlapped_geometry_per_level_count(dtype):
    for nz, window in ((137, (48, 89, 42)), (40, (14, 25, 12)), (12, (4, 7, 4))):
        eta = eta_levels(nz, dtype=dtype)
        assert tropopause_window(eta, nz) == (*window, True)
        for seed in (1, 2, 3):            # the seed reaches eta through the rounding of ps * sigma / ps only
            other = eta_levels(nz, seed=seed, dtype=dtype)
            assert np.allclose(other, eta, rtol=4 * np.finfo(dtype).eps, atol=0) and tropopause_window(other, nz) == (*window, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [137, 40, 12])
def test_family_reaches_every_window_geometry(nz, dtype):
    fam = eta_family(nz, dtype)
    assert set(fam) == set(ALL_GRIDS) - ({"chunk_tail"} if nz < 20 else set())
    T = np.dtype(dtype).type
    w = {}
    for name, eta in fam.items():
        assert eta.dtype == np.dtype(dtype) and eta.shape == (nz + 1,) and eta[nz] == 0
        w[name] = tropopause_window(eta, nz)
    klo, khi, nps, overlap = (dict(zip(w, v)) for v in zip(*w.values()))
    assert overlap["synthetic"] and not overlap["uniform"]                  # both branches of nl_ring_kernel's pre-scan
    assert nps["uniform"] > klo["uniform"]
    assert nps["nps_eq_klo"] == klo["nps_eq_klo"] and overlap["nps_eq_klo"]            # the hand-over, from both sides
    assert nps["nps_eq_klo_plus_1"] == klo["nps_eq_klo_plus_1"] + 1 and not overlap["nps_eq_klo_plus_1"]
    assert klo["all_inside"] == 0 and khi["all_inside"] == nz - 2
    for name in ("no_window_above", "no_window_below"):                               # the empty window
        assert (klo[name], khi[name], nps[name], overlap[name]) == (nz, -1, 0, False)
    assert (fam["no_window_above"][:nz] <= T(0.1)).all() and fam["no_window_above"][nz - 2] == T(0.1)
    assert (fam["no_window_below"][:nz] >= T(0.4)).all() and fam["no_window_below"][0] == T(0.4)
    assert not overlap["bottom_up"] and nps["bottom_up"] <= klo["bottom_up"]          # eta >= 0.4 above the window
    assert (fam["bottom_up"][:klo["bottom_up"]] >= T(0.4)).all()
    e = fam["edge_values"]
    assert e[klo["edge_values"] - 1] == T(0.1) and e[khi["edge_values"] + 1] == T(0.4) and overlap["edge_values"]
    if nz >= 20:
        assert nps["chunk_tail"] % 16 == 1 and nps["chunk_tail"] % 8 == 1 and not overlap["chunk_tail"]
    for name in ("hole", "hole_overlapped"):
        inside = fam[name][klo[name]:khi[name] + 1]
        assert ((inside <= T(0.1)) | (inside >= T(0.4))).sum() == 1
    assert not overlap["hole"] and overlap["hole_overlapped"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", ALL_GRIDS)
def test_oracle_is_finite_on_every_grid(grid, dtype):
    case = grid_case(grid, 40, dtype)
    for what, res in (("nl", case.nl()), ("tl", case.tl(0)), ("ad", case.ad(0, 1)), ("ad carried", case.ad(0, 0, traj=False))):
        for n, a in res.items():
            assert np.isfinite(a).all(), (grid, what, n)


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz,grid", CASES)
def test_nl_kernels_on_the_grid(gpu, nz, grid, dtype):
    """`cloudsc2_nl` on its LDS ring - whole waves (nx = 64), a ragged last wave (66) and one column - and on its
    register-prefetch path, which rows that are not 16-byte aligned select at any nx (66 and the smallest, 1); the fused
    `cloudsc2_nl_saturation` on both paths"""
    case = grid_case(grid, nz, dtype)
    held = Held(f"nl {grid} nz={nz}", dtype)
    for nx in (64, 66, 1):
        hold_nl(held, gpu, case, nx, "ring")
    for nx in (66, 1):
        hold_nl(held, gpu, case, nx, "prefetch")
    hold_nl(held, gpu, case, 64, "fused")
    hold_nl(held, gpu, case, 66, "fused prefetch")
    held.done()


def _general_increments(case):
    """increments that are not proportional to the state: +-2 % of every field, and +-2.5 K on t so that the perturbed t
    moves the tropopause"""
    rng = np.random.default_rng(17)
    inc = {k + "_i": (v * rng.uniform(-0.02, 0.02, size=v.shape)).astype(v.dtype) for k, v in case.fields.items()}
    inc["in_t_i"] = (rng.normal(0.0, 2.5, size=case.fields["in_t"].shape) * (case.fields["in_t"] != 0)).astype(case.dtype)
    return inc


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz,grid", CASES)
def test_perturbed_kernels_on_the_grid(gpu, nz, grid, dtype):
    """`cloudsc2_nl_perturbed` (`trpaus_prescan` on the perturbed t, chunks of 8) point by point, and the all-step-sizes
    `cloudsc2_nl_taylor_multi` (`trpaus_prescan_multi`) by its sums, bounded as tests/test_hip_fused_oracle.py bounds them"""
    case = grid_case(grid, nz, dtype)
    inc = _general_increments(case)
    if tropopause_window(case.eta, nz)[2] > 0:      # the perturbation must move the tropopause, or the pre-scan's
        moved = {k: (v + inc[k + "_i"]).astype(case.dtype) for k, v in case.fields.items()}      # perturbed reads prove nothing
        assert (case.trpaus(moved) != case.trpaus()).any()
    held = Held(f"perturbed {grid} nz={nz}", dtype)
    hold_perturbed(held, gpu, case, inc, (1.0, 0.5, 1e-2))
    held.done()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz,grid", CASES)
def test_derivative_kernels_on_the_grid(gpu, nz, grid, dtype):
    """`cloudsc2_tl` (ring at nx = 64, register path at 66) and `cloudsc2_ad`; `tl_masked` / `ad_masked`, `tl_step` /
    `ad_step`, `tl_multi` / `ad_multi` at 3 directions and a 2-member ensemble, with AD_TRAJ_FIX = 1 where the adjoint reads
    trajectory fluxes"""
    case = grid_case(grid, nz, dtype)
    held = Held(f"derivatives {grid} nz={nz}", dtype)
    hold_dense(held, gpu, case, 64, fix=0)
    hold_dense(held, gpu, case, 66, fix=1)
    hold_masked(held, gpu, case, 66, step=False)
    hold_masked(held, gpu, case, 1, step=False)
    hold_masked(held, gpu, case, 66, step=True)
    hold_multi(held, gpu, case, 66)
    hold_ensemble(held, gpu, case, 66)
    held.done()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [137, 40])
def test_evaporation_on_the_uniform_grid(gpu, nz, dtype):
    """LEVAPLS2 at dt = 60 s, where the suite compares TL with evaporation: NL on both paths, `cloudsc2_tl` / `cloudsc2_ad`
    and `tl_masked` (the adjoints from a trajectory refuse the evaporation block)"""
    case = grid_case("uniform", nz, dtype, LEVAPLS2=True, dt=60.0)
    assert (case.nl()["covptot"] > 0).any(), "the case must reach the evaporation block"
    held = Held(f"LEVAPLS2 dt=60 uniform nz={nz}", dtype)
    hold_nl(held, gpu, case, 64, "ring")
    hold_nl(held, gpu, case, 66, "ring")
    hold_nl(held, gpu, case, 66, "prefetch")
    hold_dense(held, gpu, case, 64, fix=1)
    hold_dense(held, gpu, case, 66, fix=1)
    hold_masked(held, gpu, case, 66, step=False)
    held.done()
