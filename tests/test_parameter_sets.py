"""The parameter sets of tests/param_support.py bite: run on the ORACLE alone, each set changes at least one output of every
stencil family that reads the moved parameter by more than 10 x the bound the GPU comparison of that family will use
(tests/test_hip_parameters.py), measured on that comparison's own scale.  This is a condition on the sets, not a
measurement of the kernels: without it a kernel that ignored a parameter would pass.

Which parameters a family reads is the oracle's recorded lookups, asserted against `param_support.READS`.  Every
parameter a family reads is live in it in float64; the joint sets are live in both precisions.  There are no float32
exemptions: the one-at-a-time comparisons are float64, the joint set carries every parameter in float32."""
import numpy as np
import pytest

from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import _REAL_FIELDS, default_externals
from param_support import (EVAP_PARAMS, IDENTITIES, NOLIN_PARAMS, ONE_AT_A_TIME, PLANTED, READS, SATURATION_MODES, SETS, TOL_MUL, joint_set,
                           liveness, param_case, planted_state, recorded_reads)

LIVE = 10.0


@pytest.mark.parametrize("family", sorted(READS))
def test_the_oracle_reads_what_the_table_says(family):
    assert recorded_reads(family) == READS[family], family


def test_table_covers_every_parameter():
    read_somewhere = set().union(*READS.values())
    assert read_somewhere == set(_REAL_FIELDS) and len(_REAL_FIELDS) == 35 and set(ONE_AT_A_TIME) == set(_REAL_FIELDS)
    for n in ("QMAX", "RTICECU", "RTWAT_RTICECU_R"):           # never read by a column stencil
        assert not any(n in READS[f] for f in READS if not f.startswith("saturation")), n
    assert all("RPECONS" in READS[f] for f in ("nl[evap]", "tl[evap]", "ad[evap]")) and "RPECONS" not in READS["nl"]


def test_default_set_satisfies_the_identities_and_the_joint_sets_break_them():
    d = default_externals()
    for name, (left, right) in IDENTITIES.items():
        assert abs(left(d) - right(d)) <= 1e-12 * abs(right(d)), name
    for sign in (1, -1):
        j = dict(d, **joint_set(sign))
        for name, (left, right) in IDENTITIES.items():
            assert abs(left(j) - right(j)) > 1e-2 * max(abs(left(j)), abs(right(j))), (sign, name)
        values = [j[n] for n in _REAL_FIELDS]
        assert len(set(values)) == 35 and all(np.isfinite(values))
        factors = [j[n] / (0.6 if n == "RVTMP2" else d[n]) for n in _REAL_FIELDS]
        assert len({round(f, 9) for f in factors}) == 35 and all(0.97 <= f <= 1.03 and abs(f - 1) >= 0.01 for f in factors)
        assert 0.5 < j["RVTMP2"] < 0.7
    assert joint_set(1) == SETS["joint"] and joint_set(-1) == SETS["joint_opposite"]


def test_planted_columns_hold_partial_cloud_where_zeps1_acts():
    fields, eta, dt = planted_state(np.float64)
    clc = param_case("default", np.float64).nl()["clc"]
    high = (eta[:137] > 0.1) & (eta[:137] < 0.25)
    partial = (clc[:137][high][:, list(PLANTED)] > 0) & (clc[:137][high][:, list(PLANTED)] < 1)
    assert partial.any(axis=0).all()


def _families_of(param):
    fams = [f for f in ("saturation[lphylin]", "saturation[kflag1]", "saturation[kflag0]", "nl", "tl", "ad") if param in READS[f]]
    if param in EVAP_PARAMS:
        fams += ["nl[evap]", "tl[evap]", "ad[evap]"]
    if param in NOLIN_PARAMS:
        fams += ["nl[nolin]"]
    return fams


def _outputs(name, dtype, family, own_qsat=False):
    fam, _, sw = family.partition("[")
    sw = sw.rstrip("]")
    if fam == "saturation":
        return param_case(name, dtype, own_qsat=own_qsat).saturation(sw)
    return param_case(name, dtype, sw or "default", own_qsat=own_qsat).family(fam)


@pytest.mark.parametrize("param", _REAL_FIELDS)
def test_one_at_a_time_set_is_live_in_every_family_that_reads_it(param):
    fams = _families_of(param)
    assert fams, param
    for family in fams:
        got, base = _outputs(param, np.float64, family), _outputs("default", np.float64, family)
        for n, a in got.items():
            assert np.isfinite(a).all(), (param, family, n)
        ratio = liveness(got, base, np.float64, TOL_MUL[family.partition("[")[0]])
        assert ratio > LIVE, f"{param} = {ONE_AT_A_TIME[param]!r} in {family}: {ratio:.3g} x the bound"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["joint", "joint_opposite"])
def test_joint_sets_are_live_and_finite_in_every_family(name, dtype):
    for family in sorted(READS):
        for n, a in _outputs(name, dtype, family, own_qsat=True).items():       # what the GPU tests compare with
            assert np.isfinite(a).all(), (name, family, n)
        # liveness with in_qsat held at the default set's: the difference is the family's own reading of the parameters,
        # not the changed input
        got, base = _outputs(name, dtype, family), _outputs("default", dtype, family)
        for n, a in got.items():
            assert np.isfinite(a).all(), (name, family, n)
        ratio = liveness(got, base, dtype, TOL_MUL[family.partition("[")[0]])
        assert ratio > LIVE, f"{name} in {family}: {ratio:.3g} x the bound"
    nl = _outputs(name, dtype, "nl", own_qsat=True)
    assert ((nl["clc"] > 0) & (nl["clc"] < 1)).any() and (nl["fplsl"] > 0).any() and (nl["fplsn"] > 0).any()


def test_saturation_modes_are_the_three_forms():
    assert set(SATURATION_MODES) == {"lphylin", "kflag1", "kflag0"}
