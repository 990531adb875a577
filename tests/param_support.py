"""Parameter sets other than the provisional defaults, and what tests/test_parameter_sets.py (CPU: the sets bite) and
tests/test_hip_parameters.py (GPU: the kernels follow them) share.

Every kernel takes the 35 reals of `Cloudsc2Params` by value, and `params.default_externals()` satisfies identities that
hide mistakes: RVTMP2 = 0, RTICE == RTICECU, RTWAT == RTT, ZQMAX == QMAX, RLMLT == RLSTT - RLVTT, R5ALVCP ==
R5LES RLVTT / RCPD ...  The sets here break them:

  * `ONE_AT_A_TIME[name]`: that parameter alone moved to a value at which the oracle's outputs change by far more than
    the tolerance of the GPU comparison (+3 % for most; the thresholds and RVTMP2 need the values given below);
  * `joint_set(sign)`: every real times its own factor 1 + sign * s * u, s = +-1 and u in [0.01, 0.03] drawn from a fixed
    seed in `_REAL_FIELDS` order, and RVTMP2 = 0.6.

`param_case` gives a `grid_support.Case` whose externals carry a set, so that the `hold_*` functions of grid_support hold
the kernels to the oracle run with the same set.  The state is the shared synthetic one plus `PLANTED` columns with
partial cloud between eta = 0.1 and 0.25, without which no output depends on ZEPS1 (it only acts where eta - 0.2 < ZEPS1).

`torch` and the package's GPU side are imported by nobody here."""
import numpy as np

from derivative_support import _once, host_case, host_directions
from grid_support import Case
from helpers import NL_IN, TOL, externals, oracle
from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import _REAL_FIELDS, default_externals

NX, NZ = 66, 137
PLANTED = (3, 17, 40, 65)      # columns with hand-placed partial cloud above eta = 0.25
SEED = 20241030      # the first seed from 20241019 on whose two joint sets break every identity by more than 1 %

_D = default_externals()
#: the parameter alone, moved: +3 % unless the oracle needs more to notice (measured on the oracle alone)
ONE_AT_A_TIME = {n: 1.03 * _D[n] for n in _REAL_FIELDS}
ONE_AT_A_TIME.update(
    RVTMP2=0.6,                              # the default is 0: every RCPD * RVTMP2 * q term vanishes
    ZQMAX=0.005, QMAX=0.01,                  # clips that the default 0.5 never reaches
    RLMIN=1.0e-5, ZEPS2=1.0e-5,              # thresholds far below the values they are compared with
    ZEPS1=0.05,                              # acts where eta - 0.2 < ZEPS1 (the planted columns)
    RTWAT=_D["RTT"] - 4.0,                   # the mixed-phase range of foealfa: 3 % of 273 K would leave it
    RTWAT_RTICE_R=1.2 * _D["RTWAT_RTICE_R"], RTWAT_RTICECU_R=1.2 * _D["RTWAT_RTICECU_R"])

#: switch sets: externals, and the timestep (the evaporation block is compared at dt = 60 s throughout the suite)
SWITCHES = {"default": ({}, None), "evap": (dict(LEVAPLS2=True), 60.0), "nolin": (dict(LPHYLIN=False), None)}
SATURATION_MODES = {"lphylin": dict(LPHYLIN=True), "kflag1": dict(LPHYLIN=False, KFLAG=1), "kflag0": dict(LPHYLIN=False, KFLAG=0)}

_SAT = {"QMAX", "R2ES", "R3IES", "R3LES", "R4IES", "R4LES", "RETV", "RTT", "RTWAT"}
_COLUMN = set(_REAL_FIELDS) - {"QMAX", "RTICECU", "RTWAT_RTICECU_R", "RTWAT", "RTWAT_RTICE_R", "RPECONS"}
#: family -> the reals its oracle reads (asserted against the oracle's recorded lookups).  The column stencils never read
#: QMAX, RTICECU or RTWAT_RTICECU_R; RTWAT and RTWAT_RTICE_R only in NL without LPHYLIN (foealfa); RPECONS only in the
#: evaporation block; NL without LPHYLIN does not read RLPTRC (its phase split is foealfa); TL and AD have no such form.
READS = {"saturation[lphylin]": _SAT | {"RTICE", "RTWAT_RTICE_R"}, "saturation[kflag1]": _SAT | {"RTICECU", "RTWAT_RTICECU_R"},
         "saturation[kflag0]": _SAT | {"RTICE", "RTWAT_RTICE_R"},
         "nl": _COLUMN, "tl": _COLUMN, "ad": _COLUMN,
         "nl[evap]": _COLUMN | {"RPECONS"}, "tl[evap]": _COLUMN | {"RPECONS"}, "ad[evap]": _COLUMN | {"RPECONS"},
         "nl[nolin]": (_COLUMN - {"RLPTRC"}) | {"RTWAT", "RTWAT_RTICE_R"}}
#: the parameters whose use inside the evaporation block differs from their use outside it
EVAP_PARAMS = ("RPECONS", "RCLCRIT", "RKCONV", "RG")
#: what NL reads through foealfa once LPHYLIN is off
NOLIN_PARAMS = ("RTWAT", "RTWAT_RTICE_R", "RTICE")
#: family -> multiple of `helpers.TOL` its GPU comparison uses (grid_support: 1 for values, 100 for TL outputs / adjoints)
TOL_MUL = {"saturation": 1.0, "nl": 1.0, "tl": 100.0, "ad": 100.0}

#: the identities of the default set that a joint set must break: name -> (left, right) as functions of the externals
IDENTITIES = {
    "RVTMP2 == 0": (lambda e: e["RVTMP2"], lambda e: 0.0),
    "RTICE == RTICECU": (lambda e: e["RTICE"], lambda e: e["RTICECU"]),
    "RTWAT_RTICE_R == RTWAT_RTICECU_R": (lambda e: e["RTWAT_RTICE_R"], lambda e: e["RTWAT_RTICECU_R"]),
    "ZQMAX == QMAX": (lambda e: e["ZQMAX"], lambda e: e["QMAX"]),
    "RTWAT == RTT": (lambda e: e["RTWAT"], lambda e: e["RTT"]),
    "RLMLT == RLSTT - RLVTT": (lambda e: e["RLMLT"], lambda e: e["RLSTT"] - e["RLVTT"]),
    "R5ALVCP == R5LES RLVTT / RCPD": (lambda e: e["R5ALVCP"], lambda e: e["R5LES"] * e["RLVTT"] / e["RCPD"]),
    "R5ALSCP == R5IES RLSTT / RCPD": (lambda e: e["R5ALSCP"], lambda e: e["R5IES"] * e["RLSTT"] / e["RCPD"]),
    "RALVDCP == RLVTT / RCPD": (lambda e: e["RALVDCP"], lambda e: e["RLVTT"] / e["RCPD"]),
    "RALSDCP == RLSTT / RCPD": (lambda e: e["RALSDCP"], lambda e: e["RLSTT"] / e["RCPD"]),
    "RTWAT_RTICE_R == 1 / (RTWAT - RTICE)": (lambda e: e["RTWAT_RTICE_R"], lambda e: 1.0 / (e["RTWAT"] - e["RTICE"])),
    "RTWAT_RTICECU_R == 1 / (RTWAT - RTICECU)": (lambda e: e["RTWAT_RTICECU_R"], lambda e: 1.0 / (e["RTWAT"] - e["RTICECU"])),
    "R5LES == R3LES (RTT - R4LES)": (lambda e: e["R5LES"], lambda e: e["R3LES"] * (e["RTT"] - e["R4LES"])),
    "R5IES == R3IES (RTT - R4IES)": (lambda e: e["R5IES"], lambda e: e["R3IES"] * (e["RTT"] - e["R4IES"])),
    "RCPD == 3.5 RD": (lambda e: e["RCPD"], lambda e: 3.5 * e["RD"]),
}


def joint_set(sign=1):
    """name -> value for all 35 reals: the default times 1 + sign * s * u with s = +-1 and u in [0.01, 0.03] from the fixed
    seed, drawn in `_REAL_FIELDS` order; RVTMP2 (default 0) is 0.6 times its factor"""
    rng = np.random.default_rng(SEED)
    out = {}
    for n in _REAL_FIELDS:
        s, u = (1.0 if rng.random() < 0.5 else -1.0), rng.uniform(0.01, 0.03)
        out[n] = (0.6 if n == "RVTMP2" else _D[n]) * (1.0 + sign * s * u)
    return out


SETS = dict({n: {n: v} for n, v in ONE_AT_A_TIME.items()}, joint=joint_set(1), joint_opposite=joint_set(-1))


# ----------------------------------------------------------------------------------------------
# the state
# ----------------------------------------------------------------------------------------------
def planted_state(dtype):
    """-> fields, eta, dt: the shared synthetic state (in_qsat: the oracle's saturation at the default parameters) with, in
    the `PLANTED` columns, a temperature that rises monotonically downwards through the tropopause window (so that trpaus
    stays 0.1 and the critical humidity is below 1 right under it) and q = 0.97 of the scheme's saturation value on the
    levels with 0.1 < eta < 0.25: partial cloud where max(eta - 0.2, ZEPS1) can be ZEPS1"""
    def make():
        fields, eta, dt = host_case(NX, NZ, dtype)
        F = {k: v.copy() for k, v in fields.items()}
        T = np.dtype(dtype).type
        win = [k for k in range(NZ - 1) if eta[k] > T(0.1) and eta[k] < T(0.4)]
        high = [k for k in win if eta[k] < T(0.25)]
        cols = list(PLANTED)
        for n in ("tnd_cml_t", "tnd_cml_q", "tnd_cml_ql", "tnd_cml_qi", "supsat", "ql", "qi", "lude"):
            F["in_" + n][np.ix_(high, cols)] = 0
        lo, hi = win[0], win[-1] + 2
        F["in_tnd_cml_t"][lo:hi, cols] = 0
        F["in_t"][lo:hi, cols] = np.sort(F["in_t"][lo:hi, cols], axis=0)
        qsat = np.zeros_like(F["in_t"])
        oracle.saturation(F["in_ap"], F["in_t"], qsat, externals())
        F["in_qsat"] = qsat
        t = F["in_t"][np.ix_(high, cols)]
        scaled = np.where(t < T(_D["RTICE"]), qsat[np.ix_(high, cols)] * (T(1.8) - T(0.003) * t), qsat[np.ix_(high, cols)])
        F["in_q"][np.ix_(high, cols)] = (T(0.97) * scaled).astype(dtype)
        return F, eta, dt
    return _once(("planted", np.dtype(dtype)), make)


class ParamCase(Case):
    """a `Case` whose externals carry a parameter set, plus the oracle's `saturation` under it"""

    def saturation(self, mode):
        def make():
            q = np.zeros_like(self.fields["in_t"])
            oracle.saturation(self.fields["in_ap"], self.fields["in_t"], q, self.ext(**SATURATION_MODES[mode]))
            return {"qsat": q}
        return self._cached(("param saturation", mode), make)

    def family(self, fam):
        """the oracle's outputs of a family: "saturation", "nl", "tl" (direction 0) or "ad" (forced with it, fluxes carried)"""
        return {"nl": self.nl, "tl": self.tl, "ad": lambda: self.ad(0, 1, traj=False)}[fam]()


def param_case(name, dtype, switches="default", own_qsat=False):
    """the planted state under the set `name` of `SETS` ("default": none) and a switch set of `SWITCHES`.  `own_qsat`:
    in_qsat is the oracle's saturation under the set itself (what the fused kernels form), not under the defaults - the
    one-at-a-time cases keep the default one, so that a difference from the default run is the stencil's own reading"""
    fields, eta, dt = planted_state(dtype)
    flags, dt_sw = SWITCHES[switches]
    flags = dict(flags, **({} if name == "default" else SETS[name]))
    if own_qsat:
        def make():
            q = np.zeros_like(fields["in_t"])
            oracle.saturation(fields["in_ap"], fields["in_t"], q, externals(**flags))
            return dict(fields, in_qsat=q)
        fields = _once(("param own qsat", name, switches, np.dtype(dtype)), make)
    key = ("param", name, switches, own_qsat, np.dtype(dtype))
    return ParamCase(key, fields, eta, dt if dt_sw is None else dt_sw, host_directions(NX, NZ, dtype, 3), flags)


# ----------------------------------------------------------------------------------------------
# liveness and the oracle's lookups
# ----------------------------------------------------------------------------------------------
def liveness(got, base, dtype, mul):
    """the largest |got - base| / bound over all fields, bound = mul x the `helpers.TOL` bound of `Held` / `assert_close`
    at `base` - the scale on which the GPU comparisons judge an error"""
    tol, worst = TOL[np.dtype(dtype)], 0.0
    for n in base:
        w = base[n].astype(np.float64)
        bound = mul * (tol["rtol"] * np.abs(w) + tol["atol_rel"] * float(np.max(np.abs(w))))
        err = np.abs(got[n].astype(np.float64) - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))))
    return worst


class Recording(dict):
    """externals that remember which keys were looked up"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.seen = set()

    def __getitem__(self, key):
        self.seen.add(key)
        return super().__getitem__(key)


def recorded_reads(family):
    """the reals the oracle looks up when it runs `family` (a key of `READS`) on the planted state"""
    from helpers import run_oracle_ad, run_oracle_nl, run_oracle_tl

    fields, eta, dt = planted_state(np.float64)
    fam, _, sw = family.partition("[")
    sw = sw.rstrip("]")
    if fam == "saturation":
        ext = Recording(externals(**SATURATION_MODES[sw]))
        oracle.saturation(fields["in_ap"], fields["in_t"], np.zeros_like(fields["in_t"]), ext)
    else:
        flags, dt_sw = SWITCHES[sw or "default"]
        ext = Recording(externals(NLEV=NZ, **flags))
        u = host_directions(NX, NZ, np.float64, 1)[0]
        if fam == "nl":
            run_oracle_nl(fields, eta, dt_sw or dt, ext)
        elif fam == "tl":
            run_oracle_tl(fields, {"in_" + n + "_i": u[n] for n in NL_IN}, eta, dt_sw or dt, ext)
        else:
            from helpers import NL_OUT

            forcing = {n: np.ones_like(fields["in_t"]) for n in NL_OUT}
            run_oracle_ad(fields, forcing, eta, dt_sw or dt, ext)
    return ext.seen & set(_REAL_FIELDS)
