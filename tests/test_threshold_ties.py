"""NL / TL / AD with inputs that sit exactly ON the scheme's thresholds.

`make_state` draws continuous values plus exact zeros, so no comparison of the scheme ever meets equal operands, and `<`
against `<=` - for TL / AD also which operand of a min / max carries the derivative - is never decided by a test:
tests/test_branch_coverage.py proves that branches are reached, not that their boundaries agree.  `grid_support.tie_case`
plants one tie per column on exact input values (the cumulative tendencies and `supsat` are zero, so the first-guess state
IS the input and neither contraction nor an approximate reciprocal can move a planted comparison); the oracle counts the
ties (`oracle.TIE_COUNTERS`).  Equal operands alone do not make a comparison matter, so a counter also asks for what the
comparison multiplies: `t == RTT` is planted at an overcast level that no snow enters and counted where there is
condensate to split by phase and new precipitation to freeze or not; `q == qsat` for min(q, qsat) is planted at a clear
level below an overcast one and counted where the evaporation block, its only reader, is active (LEVAPLS2 - the tests run
that case at dt = 60 s, where the suite compares TL with evaporation).  One plant cannot decide anything and is kept only
because two overcast levels are the one way to reach it: max(covptot, clc) at 1 == 1 has equal values and zero derivatives
on both sides - and random data reach it too (`REACHED_BY_RANDOM_DATA`).

Every kernel family is held to the NumPy oracle on ALL columns: `assert_close` at its default for NL outputs, 100 x for TL
outputs and adjoints (grid_support.py); the transpose identity per column below 1e4 x eps (tests/test_hip_ad_multi.py) -
at a tie TL and AD must take the same side.  The GPU tests take `in_qsat` from the device's `saturation`, so that the
kernels that form qsat themselves (`cloudsc2_nl_saturation`, the step family) meet the same q == qsat."""
import numpy as np
import pytest

from grid_support import (TIE_NX, Case, Held, device_saturation, hold_dense, hold_ensemble, hold_masked, hold_multi, hold_nl,
                          tie_case, transpose_identity)
from helpers import NL_OUT, externals, increments, nl_case, oracle, run_oracle_ad, run_oracle_nl, run_oracle_tl

DTYPES = [np.float64, np.float32]
#: reached by `nl_case` too: an overcast level gives clc = 1 exactly, so two of them in a column tie max(covptot, clc)
#: without any planting; every other tie needs equal INPUTS, which the generator never draws
REACHED_BY_RANDOM_DATA = ("covptot_equals_clc_nonzero",)


def _counts(fields, eta, dt, **flags):
    F = dict(fields)
    for n in NL_OUT:
        F["out_" + n] = np.zeros_like(fields["in_ap"])
    bc = {}
    oracle.cloudsc2_nl(F, eta, dt, externals(**flags), branch_counts=bc)
    return bc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [40, 137])
def test_every_plant_lands_on_its_comparison(nz, dtype):
    fields, eta, dt, plants = tie_case(nz, dtype)
    for flags, counters in ((dict(), tuple(n for n in oracle.TIE_COUNTERS if n != "q_equals_qsat")),
                            (dict(LEVAPLS2=True), oracle.TIE_COUNTERS)):     # min(q, qsat) is read by the evaporation block only
        bc = _counts(fields, eta, 60.0 if flags else dt, **flags)
        print(flags, {n: bc.get(n, 0) for n in oracle.TIE_COUNTERS})
        missing = [n for n in counters if bc.get(n, 0) == 0]
        assert not missing, f"no grid point of tie_case({nz}, {np.dtype(dtype).name}) {flags} ties {missing}"
    assert len(plants) + 8 <= TIE_NX                      # control columns remain


def test_the_generator_never_draws_a_tie():
    """the gap `tie_case` closes"""
    for flags in (dict(), dict(LEVAPLS2=True)):
        bc = _counts(*nl_case(256), **flags)
        hit = {n: bc[n] for n in oracle.TIE_COUNTERS if bc.get(n, 0) != 0 and n not in REACHED_BY_RANDOM_DATA}
        assert not hit, hit
        assert all(bc[n] > 0 for n in REACHED_BY_RANDOM_DATA)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [40, 137])
def test_oracle_is_finite_on_the_ties(nz, dtype):
    """including the 0 / 0 that qt == qcrit == qsat puts into the unselected partial-cloud lane"""
    fields, eta, dt, _ = tie_case(nz, dtype)
    for flags, step in ((dict(AD_TRAJ_FIX=1), dt), (dict(LEVAPLS2=True), 60.0)):
        ext = externals(NLEV=nz, **flags)
        nl0 = run_oracle_nl(fields, eta, step, ext)
        _, tl_i = run_oracle_tl(fields, increments(fields, 0.01), eta, step, ext)
        _, adj = run_oracle_ad(fields, tl_i, eta, step, ext, traj=None if "LEVAPLS2" in flags else nl0)
        for what, res in (("nl", nl0), ("tl", tl_i), ("ad", adj)):
            for n, a in res.items():
                assert np.isfinite(a).all(), (flags, what, n)


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
_cases, _evap = {}, {}


def _case(gpu, nz, dtype):
    """`tie_case` with the device's qsat and three general directions; one per (nz, dtype), never modified"""
    from derivative_support import host_directions

    key = (nz, np.dtype(dtype))
    if key not in _cases:
        fields, eta, dt, plants = tie_case(nz, dtype, device_saturation(gpu, dtype))
        bc = _counts(fields, eta, 60.0, LEVAPLS2=True)
        assert all(bc[n] > 0 for n in oracle.TIE_COUNTERS), bc           # the device's qsat ties as the oracle's does
        _cases[key] = Case(None, fields, eta, dt, host_directions(TIE_NX, nz, dtype, 3)), plants
    return _cases[key]


def _done(held, plants):
    worst = {name: float(held.by_column[c]) for name, c in plants.items()}
    worst["controls"] = float(held.by_column[len(plants):].max())
    print(f"{held.tag} {held.dtype.name}: worst |error| / bound per plant: " + "; ".join(f"{n}: {v:.3g}" for n, v in worst.items()))
    held.done()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [40, 137])
def test_nl_kernels_on_the_ties(gpu, nz, dtype):
    case, plants = _case(gpu, nz, dtype)
    held = Held(f"ties nl nz={nz}", dtype, TIE_NX)
    hold_nl(held, gpu, case, TIE_NX, "ring")
    hold_nl(held, gpu, case, TIE_NX, "prefetch")
    hold_nl(held, gpu, case, TIE_NX, "fused")
    hold_nl(held, gpu, case, TIE_NX, "fused prefetch")
    _done(held, plants)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("nz", [40, 137])
def test_derivative_kernels_on_the_ties(gpu, nz, fix, dtype):
    """TL with general increments, AD with general forcing (the oracle's TL outputs), AD_TRAJ_FIX 0 and 1: `cloudsc2_tl` /
    `cloudsc2_ad`, masked and step; at AD_TRAJ_FIX = 1 also 3 directions in one launch and a 2-member ensemble"""
    case, plants = _case(gpu, nz, dtype)
    held = Held(f"ties derivatives nz={nz} FIX={fix}", dtype, TIE_NX)
    hold_dense(held, gpu, case, TIE_NX, fix=fix)
    hold_masked(held, gpu, case, TIE_NX, step=False, fix=fix)
    hold_masked(held, gpu, case, TIE_NX, step=True, fix=fix)
    if fix:
        hold_multi(held, gpu, case, TIE_NX)
        hold_ensemble(held, gpu, case, TIE_NX)
    _done(held, plants)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [40, 137])
def test_kernels_on_the_ties_with_evaporation(gpu, nz, dtype):
    """LEVAPLS2 at dt = 60 s: the evaporation block reads min(q, qsat) at q == qsat, and TL / AD carry one operand's
    derivative there.  NL on both paths, `cloudsc2_tl` / `cloudsc2_ad` and `tl_masked` (the adjoints from a trajectory
    refuse the evaporation block)"""
    base, plants = _case(gpu, nz, dtype)
    case = _evap.setdefault((nz, np.dtype(dtype)), Case(None, base.fields, base.eta, 60.0, base.dirs, dict(LEVAPLS2=True)))
    held = Held(f"ties LEVAPLS2 dt=60 nz={nz}", dtype, TIE_NX)
    hold_nl(held, gpu, case, TIE_NX, "ring")
    hold_nl(held, gpu, case, TIE_NX, "prefetch")
    hold_dense(held, gpu, case, TIE_NX, fix=1)
    hold_masked(held, gpu, case, TIE_NX, step=False)
    _done(held, plants)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", [40, 137])
def test_tl_and_ad_take_the_same_side_of_every_tie(gpu, nz, dtype):
    case, plants = _case(gpu, nz, dtype)
    _, _, norm3 = transpose_identity(gpu, case, TIE_NX)
    names = {c: n for n, c in plants.items()}
    print(f"ties transpose identity nz={nz} {np.dtype(dtype).name}: " +
          "; ".join(f"{names.get(c, 'control')}: {v:.3g}" for c, v in enumerate(norm3[:len(plants) + 1])) + f"; max {norm3.max():.3g} x eps")
    assert (norm3 < 1e4).all(), {names.get(c, f"control {c}"): float(v) for c, v in enumerate(norm3) if not v < 1e4}
