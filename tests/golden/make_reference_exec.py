"""Generate golden vectors by executing the REFERENCE's own stencil source (read from
/root/reference, never copied) through tests/golden/gtscript_exec.py on seeded synthetic columns.

Run in the build container only:  python tests/golden/make_reference_exec.py
Writes tests/golden/reference_exec.npz, reference_exec_evap.npz (fp64), reference_exec_f32.npz (float32 fields:
the drivers' cases + LEVAPLS2; see main() for the fp32 semantics) and reference_exec_params.npz (fp64, the joint
parameter set of tests/param_support.py; see main_params()) - inputs + outputs, data only.  The GPU box has no
/root/reference, so the tests read the .npz.

What the vectors pin: saturation, cloudsc2_nl (driver flags, and LEVAPLS2=True), cloudsc2_tl
(LREGCL True/False), cloudsc2_ad (LREGCL True), state_increment, perturbed_state - i.e. every stencil
the three drivers call - under the executor's reading of gtscript semantics (module docstring there)
and the provisional parameter set (params.default_externals()).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from gtscript_exec import Executor, load_definitions, reference_stencil_files  # noqa: E402

from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import DEFAULT_TIMESTEP_S, default_externals  # noqa: E402
from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state  # noqa: E402

REFERENCE = "/root/reference"
NX, NZ, SEED = 40, 137, 20240807
NL_IN = ("ap", "aph", "lu", "lude", "mfd", "mfu", "q", "qi", "ql", "qsat", "supsat", "t",
         "tnd_cml_q", "tnd_cml_qi", "tnd_cml_ql", "tnd_cml_t")
NL_OUT = ("clc", "covptot", "fhpsl", "fhpsn", "fplsl", "fplsn", "tnd_q", "tnd_qi", "tnd_ql", "tnd_t")


DTYPE = np.float64     # field dtype of the run in progress (main() is executed once per precision)


def zeros(nx=NX):
    return np.zeros((NZ + 1, nx), DTYPE)


class _Exec(Executor):
    """Executor in the precision of the run in progress."""

    def __init__(self, defs, externals):
        super().__init__(defs, externals, dtype=DTYPE)


def main(dtype=np.float64):
    """dtype=float64: the two fp64 files (every case).  dtype=float32: `reference_exec_f32.npz`, the drivers' cases
    plus LEVAPLS2, executed with float32 fields.  fp32 semantics of this executor = GT4Py's numpy backend under
    value-based scalar casting: fields, temporaries and the scalar arguments (`dt`, `f`) are float32; externals and
    literals are Python floats, i.e. *weak* scalars that take the field's precision in every operation with a field
    (scalar-only sub-expressions such as RLVTT / RCPD are evaluated in double and rounded once when they meet a field)."""
    global DTYPE
    DTYPE = np.dtype(dtype).type
    f32 = DTYPE is np.float32
    Executor = _Exec  # noqa: N806 - every stencil run below uses the run's precision
    defs = load_definitions(reference_stencil_files(REFERENCE))
    ext = default_externals()
    ext["NLEV"] = NZ
    dt = DEFAULT_TIMESTEP_S
    s = make_state(NX, NZ, seed=SEED, dtype=DTYPE)
    eta = eta_levels(NZ, seed=SEED, dtype=DTYPE)
    out = {"eta": eta, "dt": np.float64(dt), "nz": np.int64(NZ)}
    ins = {"in_" + k[2:]: v.copy() for k, v in s.items()}

    # saturation (domain nz levels; kflag=1, lphylin=True as the drivers)
    qsat = zeros()
    Executor(defs, {**ext, "KFLAG": 1, "LPHYLIN": True, "QMAX": 0.5}).run(
        "saturation", {"in_ap": ins["in_ap"], "in_t": ins["in_t"], "out_qsat": qsat}, {}, NZ, domain_levels=NZ)
    ins["in_qsat"] = qsat
    for n in NL_IN:
        out["in_" + n] = ins["in_" + n]

    def ij():
        return np.zeros(NX, DTYPE)

    def run_nl(e, inputs):
        f = {k: v.copy() for k, v in inputs.items()}
        f["in_eta"] = eta
        for n in NL_OUT:
            f["out_" + n] = zeros()
        for n in ("tmp_aph_s", "tmp_covptot", "tmp_rfl", "tmp_sfl", "tmp_trpaus"):
            f[n] = ij()
        Executor(defs, e).run("cloudsc2_nl", f, {"dt": dt}, NZ)
        return {n: f["out_" + n] for n in NL_OUT}

    nl_cases = (("nl", ext), ("nl_evap", {**ext, "LEVAPLS2": True}), ("nl_nolin", {**ext, "LPHYLIN": False}))
    for tag, e in nl_cases[:2] if f32 else nl_cases:
        r = run_nl(e, ins)
        for n in NL_OUT:
            out[f"{tag}_out_{n}"] = r[n]

    # state_increment (f = 0.01) and perturbed_state (f = 1e-3)
    INC = ("aph", "ap", "q", "qsat", "t", "ql", "qi", "lude", "lu", "mfu", "mfd",
           "tnd_cml_t", "tnd_cml_q", "tnd_cml_ql", "tnd_cml_qi", "supsat")
    for tag, ign in (("inc", False), ("inc_nosupsat", True)):
        f = {"in_" + n: ins["in_" + n].copy() for n in INC}
        f.update({"out_" + n + "_i": zeros() for n in INC})
        Executor(defs, {"IGNORE_SUPSAT": ign}).run("state_increment", f, {"f": 0.01}, NZ)
        for n in INC:
            out[f"{tag}_{n}_i"] = f["out_" + n + "_i"]
    f = {"in_" + n: ins["in_" + n].copy() for n in INC}
    f.update({"in_" + n + "_i": out[f"inc_{n}_i"].copy() for n in INC})
    f.update({"out_" + n: zeros() for n in INC})
    Executor(defs, {}).run("perturbed_state", f, {"f": 1e-3}, NZ)
    for n in INC:
        out[f"pert_{n}"] = f["out_" + n]

    klevel = np.arange(0, NZ + 1)

    def run_tl(e, inc_tag, dt=dt, src=None):
        src = out if src is None else src
        f = {k: v.copy() for k, v in ins.items()}
        f.update({"in_" + n + "_i": src[f"{inc_tag}_{n}_i"].copy() for n in NL_IN})
        f["in_eta"] = eta
        f["tmp_klevel"] = klevel
        for n in NL_OUT:
            f["out_" + n] = zeros()
            f["out_" + n + "_i"] = zeros()
        for n in ("tmp_aph_s", "tmp_aph_s_i", "tmp_covptot", "tmp_covptot_i", "tmp_rfl", "tmp_rfl_i", "tmp_sfl",
                  "tmp_sfl_i", "tmp_trpaus"):
            f[n] = ij()
        Executor(defs, e).run("cloudsc2_tl", f, {"dt": dt}, NZ)
        return f

    evap = {**ext, "LEVAPLS2": True}
    tl_cases = (("tl", ext, "inc"), ("tl_noreg", {**ext, "LREGCL": False}, "inc"),
                ("tl_sym", ext, "inc_nosupsat"), ("tl_evap", evap, "inc_nosupsat"))
    for tag, e, inc_tag in tl_cases[1:3] if f32 else tl_cases:   # fp32: the Taylor test's and the symmetry test's TL
        f = run_tl(e, inc_tag)
        for n in NL_OUT:
            out[f"{tag}_out_{n}"] = f["out_" + n]
            out[f"{tag}_out_{n}_i"] = f["out_" + n + "_i"]

    # cloudsc2_ad forced with the TL outputs of the symmetry-test setup (adjoint/validation.py:132-153)
    # (no AD vector with LEVAPLS2: on these columns the reference's own TL evaporation block already
    #  produces perturbations of order 1e43 - "the code never enters this branch when input data are
    #  retrieved from input.h5", tangent_linear/_stencils/cloudsc2.py:529-530 - so its adjoint is noise)
    def run_ad(e, forcing, dt=dt):
        f = {k: v.copy() for k, v in ins.items()}
        f["in_eta"] = eta
        f["tmp_klevel"] = klevel
        for n in NL_OUT:
            f["in_" + n + "_i"] = forcing[n].copy()
            f["out_" + n] = zeros()
        for n in NL_IN:
            f["out_" + n + "_i"] = zeros()
        for n in ("tmp_aph_s", "tmp_aph_s_i", "tmp_covptotp", "tmp_rfln", "tmp_rfln_i", "tmp_sfln", "tmp_sfln_i",
                  "tmp_trpaus"):
            f[n] = ij()
        Executor(defs, e).run("cloudsc2_ad", f, {"dt": dt}, NZ)
        return f

    ad_cases = (("ad", ext, "tl_sym"), ("ad_noreg", {**ext, "LREGCL": False}, "tl_sym"))
    for tag, e, tl_tag in ad_cases[:1] if f32 else ad_cases:
        f = run_ad(e, {n: out[f"{tl_tag}_out_{n}_i"] for n in NL_OUT})
        for n in NL_OUT:
            out[f"{tag}_out_{n}"] = f["out_" + n]
        for n in NL_IN:
            out[f"{tag}_out_{n}_i"] = f["out_" + n + "_i"]

    if not f32:
        path = os.path.join(HERE, "reference_exec.npz")
        np.savez_compressed(path, **out)
        print(path, len(out), "arrays", os.path.getsize(path) // 1024, "KiB")

    # ---- evaporation block of TL and AD (LEVAPLS2) at dt = 60 s with increments that are NOT proportional to
    # the state: at the drivers' 3600 s the reference's TL recurrence amplifies rounding noise (its b_i carries
    # dt**2 where the derivative has dt, tangent_linear/_stencils/cloudsc2.py:565-569) and a uniform 1 % scaling
    # is nearly a symmetry of the scheme, so the vectors above cannot pin this block.  Same inputs as above.
    ev = {"dt": np.float64(60.0)}
    rng = np.random.default_rng(SEED)
    for n in NL_IN:
        ev[f"inc_{n}_i"] = (0.01 * ins["in_" + n] * rng.uniform(0.5, 1.5, size=ins["in_" + n].shape)).astype(DTYPE)
    ev["inc_supsat_i"][...] = 0.0
    if f32:
        # fp32 file: + the evaporation block of TL / AD (LEVAPLS2, LREGCL as the drivers) at dt = 60 s, then done
        f = run_tl(evap, "inc", dt=60.0, src=ev)
        for n in NL_IN:
            out[f"evap60_inc_{n}_i"] = ev[f"inc_{n}_i"]
        for n in NL_OUT:
            out[f"evap60_tl_out_{n}"] = f["out_" + n]
            out[f"evap60_tl_out_{n}_i"] = f["out_" + n + "_i"]
        f = run_ad(evap, {n: out[f"evap60_tl_out_{n}_i"] for n in NL_OUT}, dt=60.0)
        for n in NL_OUT:
            out[f"evap60_ad_out_{n}"] = f["out_" + n]
        for n in NL_IN:
            out[f"evap60_ad_out_{n}_i"] = f["out_" + n + "_i"]
        bad = [k for k, v in out.items() if isinstance(v, np.ndarray) and v.ndim == 2 and v.dtype != np.float32]
        assert not bad, bad
        path = os.path.join(HERE, "reference_exec_f32.npz")
        np.savez_compressed(path, **out)
        print(path, len(out), "arrays", os.path.getsize(path) // 1024, "KiB")
        return
    for tag, e in (("tl_evap", evap), ("tl_evap_noreg", {**evap, "LREGCL": False})):
        f = run_tl(e, "inc", dt=60.0, src=ev)
        for n in NL_OUT:
            ev[f"{tag}_out_{n}"] = f["out_" + n]
            ev[f"{tag}_out_{n}_i"] = f["out_" + n + "_i"]
    for tag, e, tl_tag in (("ad_evap", evap, "tl_evap"), ("ad_evap_noreg", {**evap, "LREGCL": False}, "tl_evap_noreg")):
        f = run_ad(e, {n: ev[f"{tl_tag}_out_{n}_i"] for n in NL_OUT}, dt=60.0)
        for n in NL_OUT:
            ev[f"{tag}_out_{n}"] = f["out_" + n]
        for n in NL_IN:
            ev[f"{tag}_out_{n}_i"] = f["out_" + n + "_i"]
    # ---- default switches, driver timestep, but GENERAL data: every input field gets its own random increment
    # (signs included, +-0.3 K on t) and the adjoint is forced with ten independent random fields - the vectors of the
    # first file use `state_increment`'s proportional increments, under which many TL / AD terms cancel or vanish
    rng = np.random.default_rng(SEED + 1)
    for n in NL_IN:
        ev[f"gen_{n}_i"] = ins["in_" + n] * rng.uniform(-0.02, 0.02, size=ins["in_" + n].shape)
    ev["gen_t_i"] = rng.normal(0.0, 0.3, size=ins["in_t"].shape) * (ins["in_t"] != 0)
    for tag, e in (("tl_gen", ext), ("tl_gen_noreg", {**ext, "LREGCL": False})):
        f = run_tl(e, "gen", src=ev)
        for n in NL_OUT:
            ev[f"{tag}_out_{n}"] = f["out_" + n]
            ev[f"{tag}_out_{n}_i"] = f["out_" + n + "_i"]
    for n in NL_OUT:
        scale = max(float(np.abs(out[f"nl_out_{n}"]).max()), 1e-30) if n != "covptot" else 1.0
        ev[f"genf_{n}"] = rng.normal(0.0, 1.0, size=(NZ + 1, NX)) * scale
        ev[f"genf_{n}"][NZ if n in ("clc", "covptot", "tnd_q", "tnd_qi", "tnd_ql", "tnd_t") else NZ + 1:] = 0.0
    for tag, e in (("ad_gen", ext), ("ad_gen_noreg", {**ext, "LREGCL": False})):
        f = run_ad(e, {n: ev[f"genf_{n}"] for n in NL_OUT})
        for n in NL_OUT:
            ev[f"{tag}_out_{n}"] = f["out_" + n]
        for n in NL_IN:
            ev[f"{tag}_out_{n}_i"] = f["out_" + n + "_i"]
    path = os.path.join(HERE, "reference_exec_evap.npz")
    np.savez_compressed(path, **ev)
    print(path, len(ev), "arrays", os.path.getsize(path) // 1024, "KiB")


def main_params(nx=16):
    """`reference_exec_params.npz`: the reference's stencils under the joint parameter set of tests/param_support.py (every
    real of the externals moved by its own factor, RVTMP2 = 0.6 x its factor - no identity of the provisional set holds),
    fp64, 16 columns: saturation in its three forms, cloudsc2_nl, cloudsc2_tl with general increments and cloudsc2_ad with
    general forcing.  Inputs, parameter values and outputs - data only."""
    global DTYPE
    DTYPE = np.float64
    sys.path.insert(0, os.path.dirname(HERE))
    from param_support import SATURATION_MODES, joint_set

    defs = load_definitions(reference_stencil_files(REFERENCE))
    params = joint_set(1)
    ext = {**default_externals(), **params, "NLEV": NZ}
    dt = DEFAULT_TIMESTEP_S
    s = make_state(nx, NZ, seed=SEED + 2, dtype=DTYPE)
    eta = eta_levels(NZ, seed=SEED + 2, dtype=DTYPE)
    out = {"eta": eta, "dt": np.float64(dt), "nz": np.int64(NZ)}
    for n, v in params.items():
        out["param_" + n] = np.float64(v)
    ins = {"in_" + k[2:]: v.copy() for k, v in s.items()}
    for mode, sw in SATURATION_MODES.items():
        qsat = zeros(nx)
        _Exec(defs, {**ext, "KFLAG": 1, **sw}).run(
            "saturation", {"in_ap": ins["in_ap"], "in_t": ins["in_t"], "out_qsat": qsat}, {}, NZ, domain_levels=NZ)
        out["qsat_" + mode] = qsat
    ins["in_qsat"] = out["qsat_lphylin"]
    for n in NL_IN:
        out["in_" + n] = ins["in_" + n]
    klevel = np.arange(0, NZ + 1)
    ij = lambda: np.zeros(nx, DTYPE)  # noqa: E731

    f = {k: v.copy() for k, v in ins.items()}
    f["in_eta"] = eta
    for n in NL_OUT:
        f["out_" + n] = zeros(nx)
    for n in ("tmp_aph_s", "tmp_covptot", "tmp_rfl", "tmp_sfl", "tmp_trpaus"):
        f[n] = ij()
    _Exec(defs, ext).run("cloudsc2_nl", f, {"dt": dt}, NZ)
    for n in NL_OUT:
        out["nl_out_" + n] = f["out_" + n]

    rng = np.random.default_rng(SEED + 3)
    for n in NL_IN:
        out[f"gen_{n}_i"] = ins["in_" + n] * rng.uniform(-0.02, 0.02, size=ins["in_" + n].shape)
    out["gen_t_i"] = rng.normal(0.0, 0.3, size=ins["in_t"].shape) * (ins["in_t"] != 0)
    f = {k: v.copy() for k, v in ins.items()}
    f.update({"in_" + n + "_i": out[f"gen_{n}_i"].copy() for n in NL_IN})
    f["in_eta"] = eta
    f["tmp_klevel"] = klevel
    for n in NL_OUT:
        f["out_" + n] = zeros(nx)
        f["out_" + n + "_i"] = zeros(nx)
    for n in ("tmp_aph_s", "tmp_aph_s_i", "tmp_covptot", "tmp_covptot_i", "tmp_rfl", "tmp_rfl_i", "tmp_sfl", "tmp_sfl_i",
              "tmp_trpaus"):
        f[n] = ij()
    _Exec(defs, ext).run("cloudsc2_tl", f, {"dt": dt}, NZ)
    for n in NL_OUT:
        out[f"tl_out_{n}"] = f["out_" + n]
        out[f"tl_out_{n}_i"] = f["out_" + n + "_i"]

    for n in NL_OUT:
        scale = max(float(np.abs(out[f"nl_out_{n}"]).max()), 1e-30) if n != "covptot" else 1.0
        out[f"genf_{n}"] = rng.normal(0.0, 1.0, size=(NZ + 1, nx)) * scale
        out[f"genf_{n}"][NZ if n in ("clc", "covptot", "tnd_q", "tnd_qi", "tnd_ql", "tnd_t") else NZ + 1:] = 0.0
    f = {k: v.copy() for k, v in ins.items()}
    f["in_eta"] = eta
    f["tmp_klevel"] = klevel
    for n in NL_OUT:
        f["in_" + n + "_i"] = out[f"genf_{n}"].copy()
        f["out_" + n] = zeros(nx)
    for n in NL_IN:
        f["out_" + n + "_i"] = zeros(nx)
    for n in ("tmp_aph_s", "tmp_aph_s_i", "tmp_covptotp", "tmp_rfln", "tmp_rfln_i", "tmp_sfln", "tmp_sfln_i", "tmp_trpaus"):
        f[n] = ij()
    _Exec(defs, ext).run("cloudsc2_ad", f, {"dt": dt}, NZ)
    for n in NL_OUT:
        out[f"ad_out_{n}"] = f["out_" + n]
    for n in NL_IN:
        out[f"ad_out_{n}_i"] = f["out_" + n + "_i"]
    path = os.path.join(HERE, "reference_exec_params.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if sys.argv[1:] != ["params"]:         # `params`: the parameter-set file alone
        main(np.float64)
        main(np.float32)
    main_params()
