"""CPU checks that pin the oracle's TL and AD restatements relative to its NL restatement - the
reference's own test strategy: Taylor test (TL vs finite differences of NL,
tangent_linear/validation.py:150-261) and symmetry test (AD vs TL, adjoint/validation.py:132-215)."""
import numpy as np
import pytest

from helpers import (NL_IN, NL_OUT, TOL, assert_close, externals, increments, nl_case, nlev_of, run_oracle_ad, run_oracle_nl,
                     run_oracle_tl, straddle_columns, symmetry_norm3, taylor_norms)
from oracle import cloudsc2_numpy as oracle

F2S = tuple(10.0 ** -i for i in range(1, 11))


def test_tl_trajectory_equals_nl():
    ext = externals(NLEV=137)
    fields, eta, dt = nl_case(128)
    nl = run_oracle_nl(fields, eta, dt, ext)
    tl, _ = run_oracle_tl(fields, increments(fields), eta, dt, ext)
    for n in NL_OUT:
        k = nlev_of(n, 137)
        scale = max(np.abs(nl[n]).max(), 1e-300)
        assert np.abs(tl[n][:k] - nl[n][:k]).max() <= 1e-12 * scale, n


def test_taylor_test_of_the_oracle():
    """LREGCL = False, factor1 = 0.01, factor2 = 1e-1 .. 1e-10 (drivers/run_taylor_test.py:75-90):
    every per-field ratio must converge to 1 and the aggregate norm must show the V shape."""
    ext = externals(LREGCL=False, NLEV=137)
    fields, eta, dt = nl_case(192)
    fi = increments(fields, 0.01)
    nl0 = run_oracle_nl(fields, eta, dt, ext)
    _, tl_i = run_oracle_tl(fields, fi, eta, dt, ext)

    def nlp(f2):
        fp = {k: fields[k] + f2 * fi[k + "_i"] for k in fields}
        return run_oracle_nl(fp, eta, dt, ext)

    norms = taylor_norms(nl0, nlp, tl_i, F2S)
    err = np.abs(1 - norms)
    assert err.min() < 1e-6, norms
    assert err[4:9].max() < 1e-4, norms           # 1e-5 .. 1e-9: linear regime
    # per-field derivative check at the best step size (stricter than the aggregate norm)
    f2 = 1e-6
    p = nlp(f2)
    for n in NL_OUT:
        den = f2 * tl_i[n].sum()
        if abs(den) > 1e-300:
            assert abs((p[n] - nl0[n]).sum() / den - 1) < 1e-4, n


def test_symmetry_test_of_the_oracle():
    """AD vs TL as the reference's SymmetryTest (pass criterion norm3 < 1e4, adjoint/validation.py:160).
    With the reference's literal freezing tests (quirks Q4/Q5) the few columns whose saturation
    adjustment crosses RTT fail; with AD_TRAJ_FIX (the NL/TL tests) EVERY column matches to a few eps,
    i.e. the AD restatement is the exact transpose of the TL restatement."""
    fields, eta, dt = nl_case(256)
    fi = increments(fields, 0.01, ignore_supsat=True)
    ext = externals(NLEV=137)
    tl, tl_i = run_oracle_tl(fields, fi, eta, dt, ext)
    _, ad_i = run_oracle_ad(fields, tl_i, eta, dt, ext)
    _, _, norm3 = symmetry_norm3(tl_i, fi, ad_i)
    assert np.mean(norm3 < 1e4) > 0.95, np.mean(norm3 < 1e4)
    assert np.median(norm3) < 10
    ad_nl, ad_i = run_oracle_ad(fields, tl_i, eta, dt, externals(NLEV=137, AD_TRAJ_FIX=1))
    _, _, norm3 = symmetry_norm3(tl_i, fi, ad_i)
    assert norm3.max() < 100, norm3.max()
    for n in NL_OUT:   # and the NL outputs AD recomputes equal TL's trajectory
        k = nlev_of(n, 137)
        assert np.abs(ad_nl[n][:k] - tl[n][:k]).max() <= 1e-12 * max(np.abs(tl[n]).max(), 1e-300), n


def test_increment_and_perturbation():
    fields, _, _ = nl_case(16)
    st = {k[3:]: v for k, v in fields.items()}
    inc = {k + "_i": np.empty_like(v) for k, v in st.items()}
    oracle.state_increment(st, inc, 0.01, ignore_supsat=True)
    assert np.all(inc["supsat_i"] == 0) and np.array_equal(inc["t_i"], 0.01 * st["t"])
    st.update(inc)
    out = {k: np.empty_like(v) for k, v in fields.items() for k in [k[3:]]}
    oracle.perturbed_state(st, out, 1e-3)
    assert np.array_equal(out["q"], st["q"] + 1e-3 * st["q_i"])


# ---------------------------------------------------------------------------------------------- AD from given fluxes
# The oracle of `cloudsc2_ad_from_trajectory`: cloudsc2_ad whose forward sweep reads the fluxes entering each level
# instead of carrying them.  The fixture case has columns whose saturation adjustment crosses RTT (asserted below).
def _flux_case(dtype, **flags):
    ext = externals(NLEV=137, **flags)
    fields, eta, dt = nl_case(512, dtype=dtype)
    fi = increments(fields, 0.01, ignore_supsat=True)
    tl, tl_i = run_oracle_tl(fields, fi, eta, dt, ext)
    diag = {}
    ad_nl, ad_i = run_oracle_ad(fields, tl_i, eta, dt, ext, diag=diag)
    straddle = np.flatnonzero(diag["straddle"])
    assert straddle.size > 0                        # the case exercises quirk Q4 (or its fix)
    assert np.array_equal(straddle, straddle_columns(fields, tl_i, eta, dt, ext))
    return ext, fields, eta, dt, tl, tl_i, ad_nl, ad_i, straddle


def _flux_diff_columns(a, b, dtype, cols):
    """columns of `cols` where a flux of `a` differs from `b` beyond TOL (scale: the flux field's maximum)"""
    tol = TOL[np.dtype(dtype)]
    bad = np.zeros(len(cols), bool)
    for n in ("fplsl", "fplsn"):
        x, y = a[n][:, cols].astype(np.float64), b[n][:, cols].astype(np.float64)
        bound = tol["rtol"] * np.abs(y) + tol["atol_rel"] * float(np.abs(b[n]).max())
        bad |= (np.abs(x - y) > bound).any(axis=0)
    return np.asarray(cols)[bad]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("regcl", [True, False])
def test_ad_from_its_own_fluxes_is_cloudsc2_ad_bit_for_bit(dtype, fix, regcl):
    """`traj_fluxes` = the fluxes cloudsc2_ad's forward sweep wrote: every adjoint and NL output is the same bits"""
    ext, fields, eta, dt, _, tl_i, ad_nl, ad_i, _ = _flux_case(dtype, AD_TRAJ_FIX=fix, LREGCL=regcl)
    nl2, ad2 = run_oracle_ad(fields, tl_i, eta, dt, ext, traj=ad_nl)
    for n in NL_IN:
        assert ad2[n].dtype == dtype and np.array_equal(ad2[n], ad_i[n]), n
    for n in NL_OUT:
        assert np.array_equal(nl2[n], ad_nl[n]), n


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ad_from_given_fluxes_depends_on_the_snow_flux_of_each_level(dtype):
    """what a test of the trajectory kernel can see: without the evaporation block the adjoints depend on the given snow
    flux (through melting, :293-302) and not on the rain flux.  Per-level factors on the snow flux, the snow flux shifted
    by one level, or the two fluxes swapped each change the adjoints; any rain flux leaves them bit for bit."""
    ext, fields, eta, dt, _, tl_i, ad_nl, ad_i, _ = _flux_case(dtype)
    rng = np.random.default_rng(7)

    def changed(fplsl, fplsn):
        _, a = run_oracle_ad(fields, tl_i, eta, dt, ext, traj={"fplsl": fplsl, "fplsn": fplsn})
        return int(np.logical_or.reduce([(a[n] != ad_i[n]).any(axis=0) for n in NL_IN]).sum())

    factors = rng.uniform(0.5, 1.5, size=ad_nl["fplsn"].shape).astype(dtype)
    shifted = np.zeros_like(ad_nl["fplsn"])
    shifted[:-1] = ad_nl["fplsn"][1:]
    assert changed(ad_nl["fplsl"], ad_nl["fplsn"] * factors) > 0
    assert changed(ad_nl["fplsl"], shifted) > 0
    assert changed(ad_nl["fplsn"], ad_nl["fplsl"]) > 0
    assert changed(ad_nl["fplsl"] * factors, ad_nl["fplsn"]) == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tl_fluxes_equal_ad_fluxes_with_the_fix(dtype):
    """AD_TRAJ_FIX = 1: the fluxes of the TL call are those of AD's forward sweep to TOL in every column, the columns whose
    adjustment crosses RTT included - the contract under which the fused symmetry test may feed AD with TL fluxes"""
    _, _, _, _, tl, _, ad_nl, _, straddle = _flux_case(dtype, AD_TRAJ_FIX=1)
    for n in ("fplsl", "fplsn"):
        assert_close(f"TL vs AD (fix) {n}", tl[n], ad_nl[n], dtype)
        assert_close(f"TL vs AD (fix) {n}, crossing columns", tl[n][:, straddle], ad_nl[n][:, straddle], dtype,
                     scale=float(np.abs(ad_nl[n]).max()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tl_fluxes_differ_from_ad_fluxes_only_where_the_adjustment_crosses_rtt(dtype):
    """AD_TRAJ_FIX = 0 (quirk Q4): outside the oracle's straddle mask TL and AD fluxes agree to TOL; inside it some column
    differs beyond TOL - so feeding the reference AD with TL fluxes is a different operation there"""
    _, _, _, _, tl, _, ad_nl, _, straddle = _flux_case(dtype)
    rest = np.setdiff1d(np.arange(512), straddle)
    assert rest.size > 0
    for n in ("fplsl", "fplsn"):
        assert_close(f"TL vs AD {n}, other columns", tl[n][:, rest], ad_nl[n][:, rest], dtype,
                     scale=float(np.abs(ad_nl[n]).max()))
    assert _flux_diff_columns(tl, ad_nl, dtype, straddle).size > 0
