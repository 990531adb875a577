"""Parity against the reference's OWN stencil source.

tests/golden/reference_exec.npz holds inputs and outputs obtained by executing the unmodified gtscript
stencils of /root/reference (saturation, cloudsc2_nl, cloudsc2_tl, cloudsc2_ad, state_increment,
perturbed_state) through the build's small gtscript executor (tests/golden/gtscript_exec.py,
generator: tests/golden/make_reference_exec.py) on 40 seeded synthetic columns x 137 levels.

  * CPU: the NumPy oracle reproduces every vector bit for bit (it issues the same NumPy operations
    in the same order), except where noted - so the oracle IS the reference's arithmetic;
  * GPU: the HIP kernels match the same vectors within the fp64 tolerances of tests/helpers.py.
"""
import os

import numpy as np
import pytest

from helpers import (NL_IN, NL_OUT, assert_close, externals, nlev_of, run_oracle_ad, run_oracle_nl,
                     run_oracle_tl)
from oracle import cloudsc2_numpy as oracle

HERE = os.path.dirname(os.path.abspath(__file__))
NZ = 137
INC = ("aph", "ap", "q", "qsat", "t", "ql", "qi", "lude", "lu", "mfu", "mfd",
       "tnd_cml_t", "tnd_cml_q", "tnd_cml_ql", "tnd_cml_qi", "supsat")


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(HERE, "golden", "reference_exec.npz"))
    fields = {"in_" + n: g["in_" + n] for n in NL_IN}
    return g, fields, g["eta"], float(g["dt"])


def test_oracle_saturation_bit_exact(gold):
    g, fields, _, _ = gold
    q = np.zeros_like(fields["in_t"])
    oracle.saturation(fields["in_ap"], fields["in_t"], q, externals())
    assert np.array_equal(q, g["in_qsat"])


@pytest.mark.parametrize("tag,flags", [("nl", {}), ("nl_evap", dict(LEVAPLS2=True)), ("nl_nolin", dict(LPHYLIN=False))])
def test_oracle_nl_bit_exact(gold, tag, flags):
    g, fields, eta, dt = gold
    o = run_oracle_nl(fields, eta, dt, externals(**flags))
    for n in NL_OUT:
        assert np.array_equal(o[n], g[f"{tag}_out_{n}"]), (tag, n)
    if tag == "nl_evap":
        assert (g["nl_evap_out_covptot"] > 0).any()      # the vectors exercise the evaporation block


@pytest.mark.parametrize("tag,flags,inc", [("tl", {}, "inc"), ("tl_noreg", dict(LREGCL=False), "inc"),
                                           ("tl_sym", {}, "inc_nosupsat"),
                                           ("tl_evap", dict(LEVAPLS2=True), "inc_nosupsat")])
def test_oracle_tl_bit_exact(gold, tag, flags, inc):
    g, fields, eta, dt = gold
    fi = {"in_" + n + "_i": g[f"{inc}_{n}_i"] for n in NL_IN}
    o, oi = run_oracle_tl(fields, fi, eta, dt, externals(NLEV=NZ, **flags))
    for n in NL_OUT:
        assert np.array_equal(o[n], g[f"{tag}_out_{n}"]), (tag, n)
        assert np.array_equal(oi[n], g[f"{tag}_out_{n}_i"], equal_nan=True), (tag, n + "_i")


@pytest.mark.parametrize("tag,flags,tl_tag", [("ad", {}, "tl_sym"), ("ad_noreg", dict(LREGCL=False), "tl_sym")])
def test_oracle_ad_matches_reference_source(gold, tag, flags, tl_tag):
    g, fields, eta, dt = gold
    forcing = {n: g[f"{tl_tag}_out_{n}_i"] for n in NL_OUT}
    o, oi = run_oracle_ad(fields, forcing, eta, dt, externals(NLEV=NZ, **flags))
    for n in NL_OUT:
        assert np.array_equal(o[n], g[f"{tag}_out_{n}"]), (tag, n)
    for n in NL_IN:
        want = g[f"{tag}_out_{n}_i"]
        # the oracle factors one common sub-expression of the T-tendency adjoint: out_ap_i can differ
        # from the literal evaluation order in the last bit; everything else is bit-identical
        if n == "ap":
            np.testing.assert_allclose(oi[n], want, rtol=1e-14, atol=0)
        else:
            assert np.array_equal(oi[n], want), (tag, n)


@pytest.fixture(scope="module")
def gold_evap(gold):
    """Evaporation block of TL / AD executed from the reference source at dt = 60 s with non-proportional increments
    (tests/golden/make_reference_exec.py explains why): same inputs as `gold`."""
    ev = np.load(os.path.join(HERE, "golden", "reference_exec_evap.npz"))
    return ev, {"in_" + n + "_i": ev[f"inc_{n}_i"] for n in NL_IN}, float(ev["dt"])


@pytest.mark.parametrize("tag,flags", [("tl_evap", {}), ("tl_evap_noreg", dict(LREGCL=False))])
def test_oracle_tl_evaporation_bit_exact(gold, gold_evap, tag, flags):
    _, fields, eta, _ = gold
    ev, fi, dt = gold_evap
    o, oi = run_oracle_tl(fields, fi, eta, dt, externals(NLEV=NZ, LEVAPLS2=True, **flags))
    assert (ev[f"{tag}_out_covptot"] > 0).any() and (ev[f"{tag}_out_covptot_i"] != 0).any()
    for n in NL_OUT:
        assert np.array_equal(o[n], ev[f"{tag}_out_{n}"]), (tag, n)
        assert np.array_equal(oi[n], ev[f"{tag}_out_{n}_i"]), (tag, n + "_i")


@pytest.mark.parametrize("tag,flags,tl_tag", [("ad_evap", {}, "tl_evap"),
                                              ("ad_evap_noreg", dict(LREGCL=False), "tl_evap_noreg")])
def test_oracle_ad_evaporation_matches_reference_source(gold, gold_evap, tag, flags, tl_tag):
    _, fields, eta, _ = gold
    ev, _, dt = gold_evap
    forcing = {n: ev[f"{tl_tag}_out_{n}_i"] for n in NL_OUT}
    o, oi = run_oracle_ad(fields, forcing, eta, dt, externals(NLEV=NZ, LEVAPLS2=True, **flags))
    for n in NL_OUT:
        assert np.array_equal(o[n], ev[f"{tag}_out_{n}"]), (tag, n)
    for n in NL_IN:
        # not bit-identical (the oracle groups a few sums differently), so judged on each column's own scale;
        # out_lu_i = -(...) * a_clc inherits the cancellation inside a_clc (|terms| ~ 1e8 x |sum|) in 2-3 columns
        want = ev[f"{tag}_out_{n}_i"]
        scale = np.abs(want).max(axis=0, keepdims=True)
        tol = 1e-6 if n == "lu" else 1e-12
        assert (np.abs(oi[n] - want) <= tol * scale).all(), (tag, n, np.abs(oi[n] - want).max())


@pytest.mark.parametrize("tag,flags", [("tl_gen", {}), ("tl_gen_noreg", dict(LREGCL=False))])
def test_oracle_tl_general_increments_bit_exact(gold, gold_evap, tag, flags):
    """Default switches, dt = 3600 s, every input with its own random increment (signs included): the vectors of the
    first file use proportional increments, under which many TL terms cancel."""
    _, fields, eta, dt = gold
    ev, _, _ = gold_evap
    fi = {"in_" + n + "_i": ev[f"gen_{n}_i"] for n in NL_IN}
    o, oi = run_oracle_tl(fields, fi, eta, dt, externals(NLEV=NZ, **flags))
    for n in NL_OUT:
        assert np.array_equal(o[n], ev[f"{tag}_out_{n}"]), (tag, n)
        assert np.array_equal(oi[n], ev[f"{tag}_out_{n}_i"]), (tag, n + "_i")
    assert np.abs(ev[f"{tag}_out_clc_i"]).max() > 1e-3           # a real signal, not rounding noise


@pytest.mark.parametrize("tag,flags", [("ad_gen", {}), ("ad_gen_noreg", dict(LREGCL=False))])
def test_oracle_ad_general_forcing_matches_reference_source(gold, gold_evap, tag, flags):
    _, fields, eta, dt = gold
    ev, _, _ = gold_evap
    forcing = {n: ev[f"genf_{n}"] for n in NL_OUT}
    o, oi = run_oracle_ad(fields, forcing, eta, dt, externals(NLEV=NZ, **flags))
    for n in NL_OUT:
        assert np.array_equal(o[n], ev[f"{tag}_out_{n}"]), (tag, n)
    for n in NL_IN:
        want = ev[f"{tag}_out_{n}_i"]
        scale = np.abs(want).max(axis=0, keepdims=True)
        assert (np.abs(oi[n] - want) <= 1e-12 * scale).all(), (tag, n, np.abs(oi[n] - want).max())


def test_oracle_increment_and_perturbation_bit_exact(gold):
    g, fields, _, _ = gold
    st = {n: g["in_" + n] for n in INC}
    for tag, ign in (("inc", False), ("inc_nosupsat", True)):
        inc = {n + "_i": np.empty_like(st[n]) for n in INC}
        oracle.state_increment(st, inc, 0.01, ign)
        for n in INC:
            assert np.array_equal(inc[n + "_i"], g[f"{tag}_{n}_i"]), (tag, n)
    st.update({n + "_i": g[f"inc_{n}_i"] for n in INC})
    out = {n: np.empty_like(st[n]) for n in INC}
    oracle.perturbed_state(st, out, 1e-3)
    for n in INC:
        assert np.array_equal(out[n], g[f"pert_{n}"]), n


# ------------------------------------------------------------- off the provisional parameter point
@pytest.fixture(scope="module")
def gold_params():
    """The reference's stencils executed under the joint parameter set of tests/param_support.py (RVTMP2 non-zero, no
    identity of the provisional set left; tests/golden/make_reference_exec.py, `main_params`): 16 columns, fp64.
    -> the file, the externals it was made with, the NL inputs"""
    from param_support import joint_set

    g = np.load(os.path.join(HERE, "golden", "reference_exec_params.npz"))
    params = {k[len("param_"):]: float(g[k]) for k in g.files if k.startswith("param_")}
    assert params == joint_set(1)                      # the file was made with the set the other tests use
    return g, externals(NLEV=NZ, **params), {"in_" + n: g["in_" + n] for n in NL_IN}


def test_oracle_under_the_joint_parameter_set_bit_exact(gold_params):
    """saturation in its three forms, cloudsc2_nl, cloudsc2_tl with general increments and cloudsc2_ad with general forcing:
    the oracle's RVTMP2 terms and its reading of the unequal pairs are the reference source's, as the vectors at the
    provisional point are reproduced (the adjoints within 1e-12 of each column's scale: a few sums are grouped differently)"""
    from param_support import SATURATION_MODES

    g, ext, fields = gold_params
    eta, dt = g["eta"], float(g["dt"])
    for mode, sw in SATURATION_MODES.items():
        q = np.zeros_like(fields["in_t"])
        oracle.saturation(fields["in_ap"], fields["in_t"], q, {**ext, "KFLAG": 1, **sw})
        assert np.array_equal(q, g["qsat_" + mode]), mode
    assert not np.array_equal(g["qsat_kflag1"], g["qsat_kflag0"])          # RTICECU != RTICE is seen
    o = run_oracle_nl(fields, eta, dt, ext)
    for n in NL_OUT:
        assert np.array_equal(o[n], g[f"nl_out_{n}"]), n
    o, oi = run_oracle_tl(fields, {"in_" + n + "_i": g[f"gen_{n}_i"] for n in NL_IN}, eta, dt, ext)
    for n in NL_OUT:
        assert np.array_equal(o[n], g[f"tl_out_{n}"]), n
        assert np.array_equal(oi[n], g[f"tl_out_{n}_i"]), n + "_i"
    assert np.abs(g["tl_out_clc_i"]).max() > 1e-3
    o, oi = run_oracle_ad(fields, {n: g[f"genf_{n}"] for n in NL_OUT}, eta, dt, ext)
    for n in NL_OUT:
        assert np.array_equal(o[n], g[f"ad_out_{n}"]), n
    for n in NL_IN:
        want = g[f"ad_out_{n}_i"]
        scale = np.abs(want).max(axis=0, keepdims=True)
        assert (np.abs(oi[n] - want) <= 1e-12 * scale).all(), (n, np.abs(oi[n] - want).max())


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags", [("nl", {}), ("nl_evap", dict(LEVAPLS2=True)), ("nl_nolin", dict(LPHYLIN=False))])
def test_hip_nl_matches_reference_source(gpu, gold, tag, flags):
    from test_hip_nl import run_hip_nl

    g, fields, eta, dt = gold
    got = run_hip_nl(fields, eta, dt, externals(**flags), gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        assert_close(f"{tag} out_{n}", got[n][:k], g[f"{tag}_out_{n}"][:k])


@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags,inc", [("tl", {}, "inc"), ("tl_noreg", dict(LREGCL=False), "inc")])
def test_hip_tl_matches_reference_source(gpu, gold, tag, flags, inc):
    from test_hip_tl_ad import run_hip_tl

    g, fields, eta, dt = gold
    fi = {"in_" + n + "_i": g[f"{inc}_{n}_i"] for n in NL_IN}
    got, got_i = run_hip_tl(fields, fi, eta, dt, externals(NLEV=NZ, **flags), gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        assert_close(f"{tag} out_{n}", got[n][:k], g[f"{tag}_out_{n}"][:k])
        assert_close(f"{tag} out_{n}_i", got_i[n][:k], g[f"{tag}_out_{n}_i"][:k], rtol_mul=100.0)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags", [("ad", {}), ("ad_noreg", dict(LREGCL=False))])
def test_hip_ad_matches_reference_source(gpu, gold, tag, flags):
    from test_hip_tl_ad import run_hip_ad

    g, fields, eta, dt = gold
    forcing = {n: g[f"tl_sym_out_{n}_i"] for n in NL_OUT}
    got, got_i = run_hip_ad(fields, forcing, eta, dt, externals(NLEV=NZ, **flags), gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        assert_close(f"{tag} out_{n}", got[n][:k], g[f"{tag}_out_{n}"][:k])
    for n in NL_IN:
        k = 138 if n in ("aph", "lu") else 137
        assert_close(f"{tag} out_{n}_i", got_i[n][:k], g[f"{tag}_out_{n}_i"][:k], rtol_mul=1000.0)


def _close_by_column(name, got, want, tol):
    assert not np.isnan(got).any(), name
    scale = np.abs(want).max(axis=0, keepdims=True)
    err = np.abs(got - want)
    assert (err <= tol * scale + np.finfo(np.float64).tiny).all(), \
        f"{name}: worst {np.max(err / (scale + 1e-300)):.2e} of the column scale (tol {tol:.0e})"


@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags", [("tl_evap", {}), ("tl_evap_noreg", dict(LREGCL=False))])
def test_hip_tl_evaporation_matches_reference_source(gpu, gold, gold_evap, tag, flags):
    from test_hip_tl_ad import run_hip_tl

    _, fields, eta, _ = gold
    ev, fi, dt = gold_evap
    ext = externals(NLEV=NZ, LEVAPLS2=True, **flags)
    got, got_i = run_hip_tl(fields, fi, eta, dt, ext, gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"{tag} out_{n}", got[n][:k], ev[f"{tag}_out_{n}"][:k], 1e-9)
        _close_by_column(f"{tag} out_{n}_i", got_i[n][:k], ev[f"{tag}_out_{n}_i"][:k], 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags,tl_tag", [("ad_evap", {}, "tl_evap"),
                                              ("ad_evap_noreg", dict(LREGCL=False), "tl_evap_noreg")])
def test_hip_ad_evaporation_matches_reference_source(gpu, gold, gold_evap, tag, flags, tl_tag):
    from test_hip_tl_ad import run_hip_ad

    _, fields, eta, _ = gold
    ev, _, dt = gold_evap
    forcing = {n: ev[f"{tl_tag}_out_{n}_i"] for n in NL_OUT}
    ext = externals(NLEV=NZ, LEVAPLS2=True, **flags)
    got, got_i = run_hip_ad(fields, forcing, eta, dt, ext, gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"{tag} out_{n}", got[n][:k], ev[f"{tag}_out_{n}"][:k], 1e-9)
    for n in NL_IN:
        k = 138 if n in ("aph", "lu") else 137
        # out_lu_i: see test_oracle_ad_evaporation_matches_reference_source (cancellation inside a_clc)
        _close_by_column(f"{tag} out_{n}_i", got_i[n][:k], ev[f"{tag}_out_{n}_i"][:k], 1e-4 if n == "lu" else 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags", [("tl_gen", {}), ("tl_gen_noreg", dict(LREGCL=False))])
def test_hip_tl_general_increments_match_reference_source(gpu, gold, gold_evap, tag, flags):
    from test_hip_tl_ad import run_hip_tl

    _, fields, eta, dt = gold
    ev, _, _ = gold_evap
    fi = {"in_" + n + "_i": ev[f"gen_{n}_i"] for n in NL_IN}
    got, got_i = run_hip_tl(fields, fi, eta, dt, externals(NLEV=NZ, **flags), gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"{tag} out_{n}", got[n][:k], ev[f"{tag}_out_{n}"][:k], 1e-9)
        _close_by_column(f"{tag} out_{n}_i", got_i[n][:k], ev[f"{tag}_out_{n}_i"][:k], 1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,flags", [("ad_gen", {}), ("ad_gen_noreg", dict(LREGCL=False))])
def test_hip_ad_general_forcing_matches_reference_source(gpu, gold, gold_evap, tag, flags):
    from test_hip_tl_ad import run_hip_ad

    _, fields, eta, dt = gold
    ev, _, _ = gold_evap
    forcing = {n: ev[f"genf_{n}"] for n in NL_OUT}
    got, got_i = run_hip_ad(fields, forcing, eta, dt, externals(NLEV=NZ, **flags), gpu, fields["in_ap"].shape[1], NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"{tag} out_{n}", got[n][:k], ev[f"{tag}_out_{n}"][:k], 1e-9)
    for n in NL_IN:
        k = 138 if n in ("aph", "lu") else 137
        _close_by_column(f"{tag} out_{n}_i", got_i[n][:k], ev[f"{tag}_out_{n}_i"][:k], 1e-7)


@pytest.mark.gpu
def test_hip_saturation_matches_reference_source(gpu, gold):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil
    from helpers import from_device, to_device

    g, fields, _, _ = gold
    nx = fields["in_ap"].shape[1]
    dev = to_device({k: fields[k] for k in ("in_ap", "in_t")}, gpu)
    out = storage.zeros(nx, NZ, np.float64, gpu)
    compile_stencil("saturation", externals())(**dev, out_qsat=out, origin=(0, 0, 0), domain=(nx, 1, NZ),
                                                validate_args=True, exec_info=None)
    torch.cuda.synchronize()
    assert_close("qsat", from_device(out)[:NZ], g["in_qsat"][:NZ])


@pytest.mark.gpu
def test_hip_under_the_joint_parameter_set_matches_reference_source(gpu, gold_params):
    """the kernels against the executed reference source off the provisional parameter point, at the tolerances of the
    general-increment vectors above: 1e-9 of a column's scale for values, 1e-8 for TL outputs, 1e-7 for adjoints"""
    from derivative_support import Box
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil
    from helpers import from_device
    from param_support import SATURATION_MODES
    from test_hip_tl_ad import run_hip_ad, run_hip_tl

    g, ext, fields = gold_params
    eta, dt, nx = g["eta"], float(g["dt"]), fields["in_ap"].shape[1]
    box = Box(nx, NZ, np.float64, gpu, False)
    for mode, sw in SATURATION_MODES.items():
        out = box.nan()
        compile_stencil("saturation", {**ext, "KFLAG": 1, **sw})(
            in_ap=box.put(fields["in_ap"]), in_t=box.put(fields["in_t"]), out_qsat=out, origin=(0, 0, 0), domain=(nx, 1, NZ),
            validate_args=True, exec_info=None)
        assert_close("qsat " + mode, from_device(out)[:NZ], g["qsat_" + mode][:NZ])
    got, got_i = run_hip_tl(fields, {"in_" + n + "_i": g[f"gen_{n}_i"] for n in NL_IN}, eta, dt, ext, gpu, nx, NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"params nl out_{n}", got[n][:k], g[f"nl_out_{n}"][:k], 1e-9)
        _close_by_column(f"params tl out_{n}", got[n][:k], g[f"tl_out_{n}"][:k], 1e-9)
        _close_by_column(f"params tl out_{n}_i", got_i[n][:k], g[f"tl_out_{n}_i"][:k], 1e-8)
    outs = {n: box.nan() for n in NL_OUT}
    box.stencil("cloudsc2_nl", ext, box.torch.as_tensor(eta, device=gpu), dt, **{k: box.put(v) for k, v in fields.items()},
                **{"out_" + n: f for n, f in outs.items()})
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"params cloudsc2_nl out_{n}", from_device(outs[n])[:k], g[f"nl_out_{n}"][:k], 1e-9)
    got, got_i = run_hip_ad(fields, {n: g[f"genf_{n}"] for n in NL_OUT}, eta, dt, ext, gpu, nx, NZ)
    for n in NL_OUT:
        k = nlev_of(n, NZ)
        _close_by_column(f"params ad out_{n}", got[n][:k], g[f"ad_out_{n}"][:k], 1e-9)
    for n in NL_IN:
        k = 138 if n in ("aph", "lu") else 137
        _close_by_column(f"params ad out_{n}_i", got_i[n][:k], g[f"ad_out_{n}_i"][:k], 1e-7)
