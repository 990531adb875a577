#!/usr/bin/env python3
"""Times the step's tangent-linear and adjoint on an ENSEMBLE of `nmem` states of `nx` columns with HIP events, on the 4D-Var
mask (perturbations / adjoints of t, q, ql, qi; perturbed outputs / forcing on the four tendencies), three ways, in ONE
process with the cases interleaved round by round:

  ens      ONE ensemble launch (cloudsc2_tl_step_ens / cloudsc2_ad_step_ens) on the member-major fields
  looped   `nmem` single launches (cloudsc2_tl_step / cloudsc2_ad_step), one per member: the only way before the ensemble
           entries existed
  wide     ONE single launch on the same columns laid side by side as [level][member * nx + column], with the copies of
           every input into that layout and of every result back INSIDE the timed region

  python profiles/bench_ensemble.py [--rounds=R] [--shapes=8x8192:double,32x2048:double,64x1024:double,8x65536:single,...]

Prints one JSON line per shape: median / min microseconds and the min-max spread of every case, and the ens / looped and
ens / wide ratios of the medians (docs/TUNING_LOG.md 3.20)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
SHAPES = "8x8192:double,32x2048:double,64x1024:double,8x65536:single,32x16384:single,64x8192:single"


def measure(nmem, nx, prec, rounds):
    import ctypes

    import numpy as np
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN, NL_OUT
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    nz = 137
    np_dtype = np.float64 if prec == "double" else np.float32
    sfx = "f64" if prec == "double" else "f32"
    dev = torch.device("cuda:0")
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1)
    lib = _lib.load()
    names = tuple(n for n in NL_IN if n != "qsat")
    kc = lambda f: f.permute(0, 3, 2, 1).squeeze(2)  # noqa: E731   (nmem, nx, 1, nz+1) -> (nmem, nz+1, nx)
    new = lambda: storage.zeros_batched(nmem, nx, nz, np_dtype, dev)  # noqa: E731
    # the members: the columns of one synthetic state of nmem * nx columns, member m = columns m * nx ...
    s = make_state(nmem * nx, nz, dtype=np_dtype, device=dev)
    state = {n: new() for n in names}
    for n in names:
        kc(state[n]).copy_(torch.as_tensor(s["f_" + n], device=dev).view(nz + 1, nmem, nx).permute(1, 0, 2))
    del s
    eta = torch.as_tensor(eta_levels(nz, dtype=np_dtype), device=dev)
    dt = 3600.0
    pert = {n: new() for n in STATE4}
    for n in STATE4:
        pert[n].copy_(0.01 * state[n])
    nl, w = autodiff.tl_step_ens(state, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    traj = {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}
    forc = {n: w[n] for n in TND4}
    res = {k: {n: new() for n in (TND4 if k[0] == "tl" else STATE4)} for k in (("tl", "ens"), ("tl", "looped"), ("ad", "ens"),
                                                                             ("ad", "looped"))}
    # the wide layout: fields of nmem * nx columns
    wnx = nmem * nx
    wide = lambda: storage.zeros(wnx, nz, np_dtype, dev)  # noqa: E731
    wstate, wpert, wforc = {n: wide() for n in names}, {n: wide() for n in STATE4}, {n: wide() for n in TND4}
    wtraj = {n: wide() for n in traj}
    wres = {"tl": {n: wide() for n in TND4}, "ad": {n: wide() for n in STATE4}}
    back = {"tl": {n: new() for n in TND4}, "ad": {n: new() for n in STATE4}}
    wkc = lambda f: storage.klayout(f).view(nz + 1, nmem, nx).permute(1, 0, 2)  # noqa: E731   as (nmem, nz+1, nx)
    _, nlev, ls = storage.field_geometry(state["t"][0])
    ms = storage.direction_stride(state["t"])
    _, _, wls = storage.field_geometry(wstate["t"])
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, state["t"].dtype)
    stream = int(torch.cuda.current_stream().cuda_stream)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    m_of = lambda fields, m: {n: f[m] for n, f in fields.items()}  # noqa: E731

    def tl_args(geo, st, pe, out_i, tail=()):
        return autodiff._tl_args(p, geo, st, pe, zero, eta, None, out_i, dt, stream, tail)

    def ad_args(geo, st, fo, tr, out_adj, tail=()):
        return autodiff._ad_args(p, geo, st, fo, zero, eta, tr, out_adj, dt, stream, tail)

    geo, wgeo = (nx, nlev, ls), (wnx, nlev, wls)
    calls = {}
    a_ens = tl_args(geo, m_of(state, 0), m_of(pert, 0), m_of(res["tl", "ens"], 0), (nmem, ms))
    calls["tl ens"] = lambda: fn("tl_step_ens")(*a_ens)
    a_loop = [tl_args(geo, m_of(state, m), m_of(pert, m), m_of(res["tl", "looped"], m)) for m in range(nmem)]
    b_ens = ad_args(geo, m_of(state, 0), m_of(forc, 0), m_of(traj, 0), m_of(res["ad", "ens"], 0), (nmem, ms))
    calls["ad ens"] = lambda: fn("ad_step_ens")(*b_ens)
    b_loop = [ad_args(geo, m_of(state, m), m_of(forc, m), m_of(traj, m), m_of(res["ad", "looped"], m)) for m in range(nmem)]

    def looped(single, args):
        def call():
            rc = 0
            for a in args:
                rc = rc or fn(single)(*a)
            return rc
        return call
    calls["tl looped"], calls["ad looped"] = looped("tl_step", a_loop), looped("ad_step", b_loop)
    a_wide, b_wide = tl_args(wgeo, wstate, wpert, wres["tl"]), ad_args(wgeo, wstate, wforc, wtraj, wres["ad"])

    def wide_call(single, args, pairs, kind):
        def call():
            for src, dst in pairs:
                for n in src:
                    wkc(dst[n]).copy_(kc(src[n]))
            rc = fn(single)(*args)
            for n, f in wres[kind].items():
                kc(back[kind][n]).copy_(wkc(f))
            return rc
        return call
    calls["tl wide"] = wide_call("tl_step", a_wide, ((state, wstate), (pert, wpert)), "tl")
    calls["ad wide"] = wide_call("ad_step", b_wide, ((state, wstate), (forc, wforc), (traj, wtraj)), "ad")

    times = {k: [] for k in calls}
    for r in range(rounds + 2):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(call(), name)
            b.record()
            b.synchronize()
            if r >= 2:                      # two warm-up rounds
                times[name].append(a.elapsed_time(b) * 1e3)
    rec = {"nmem": nmem, "columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    for kind in ("tl", "ad"):
        rec[f"{kind} ens == looped (bits)"] = all(torch.equal(res[kind, "ens"][n], res[kind, "looped"][n]) for n in res[kind, "ens"])
        rec[f"{kind} ens == wide (bits)"] = all(torch.equal(res[kind, "ens"][n], back[kind][n]) for n in back[kind])
        for case in ("ens", "looped", "wide"):
            v = times[f"{kind} {case}"]
            rec[f"{kind} {case}"] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1),
                                     "max_us": round(float(np.max(v)), 1)}
        for other in ("looped", "wide"):
            rec[f"{kind} ens_over_{other}"] = round(rec[f"{kind} ens"]["median_us"] / rec[f"{kind} {other}"]["median_us"], 3)
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 15))
    import __graft_entry__ as ge

    ge.build()
    for shape in opts.get("shapes", SHAPES).split(","):
        dims, prec = shape.split(":")
        nmem, nx = (int(x) for x in dims.split("x"))
        print(json.dumps(measure(nmem, nx, prec, rounds)), flush=True)
        import torch

        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
