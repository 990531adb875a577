#!/usr/bin/env python3
"""Times the step's adjoint WITH the evaporation block (LEVAPLS2, dt = 60 s) on an ENSEMBLE of `nmem` states of `nx` columns
with HIP events, on the 4D-Var mask (forcing on the four tendencies, adjoints of t, q, ql, qi), in ONE process with the
cases interleaved round by round after two warm-up rounds:

  ens            ONE cloudsc2_ad_evap_step_ens launch on the member-major fields (cs2::ad_cover_ens_step_kernel)
  looped         `nmem` cloudsc2_ad_evap_step launches, one per member (cs2::ad_cover_step_kernel): what the derivative rules
                 do by default (`autodiff.EVAP_ENSEMBLE = False`)
  ens ready      the same two with cover_ready = 1 on the cover field the first of each pair has filled: sweep 1 is skipped
  looped ready

  masked ...     all four again for the masked (non-step) family, `qsat` a field of the state: cloudsc2_ad_evap_ens against
                 `nmem` cloudsc2_ad_evap launches (cs2::ad_cover_ens_kernel / cs2::ad_cover_kernel)

  timeout -k 10 900 python profiles/bench_ad_evap_ens.py [--rounds=R] [--shapes=8x8192:double,...,64x8192:single]

The events stand around the launches alone; every field is allocated before the first round.  The library must have been
built (`__graft_entry__.build()`): this script does not build it.  A call that fails ends the run.  Prints one JSON line per
shape: median / min / max microseconds of every case and the ens / looped ratios of the medians (docs/TUNING_LOG.md 3.25)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
SHAPES = "8x8192:double,32x2048:double,64x1024:double,8x65536:single,32x16384:single,64x8192:single"


def measure(nmem, nx, prec, rounds):
    import numpy as np
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN, NL_OUT
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    nz, dt = 137, 60.0
    np_dtype = np.float64 if prec == "double" else np.float32
    sfx = "f64" if prec == "double" else "f32"
    dev = torch.device("cuda:0")
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1, LEVAPLS2=True)
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
    # trajectory fluxes and a forcing: the NL outputs and the perturbed tendencies of a 1 % perturbation of t, q, ql, qi
    pert = {n: new() for n in STATE4}
    for n in STATE4:
        pert[n].copy_(0.01 * state[n])
    nl, w = autodiff.tl_step_ens(state, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    traj = {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}
    forc = {n: w[n] for n in TND4}
    with torch.no_grad():       # the masked family reads qsat as a field: the one the step forms
        masked_state = dict(state, qsat=autodiff.cloudsc2_step_ensemble(state, eta, dt, ext)["qsat"])
    states = {"": state, "masked ": masked_state}
    entries = {"": "ad_evap_step", "masked ": "ad_evap"}
    cases = tuple(f + c for f in states for c in ("ens", "looped", "ens ready", "looped ready"))
    res = {k: {n: new() for n in STATE4} for k in cases}
    cover = {f + c: new() for f in states for c in ("ens", "looped")}
    _, nlev, ls = storage.field_geometry(state["t"][0])
    ms = storage.direction_stride(state["t"])
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, state["t"].dtype)
    stream = int(torch.cuda.current_stream().cuda_stream)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    m_of = lambda fields, m: {n: f[m] for n, f in fields.items()}  # noqa: E731

    def args(fam, m, out, cov, ready, members=()):
        return autodiff._ad_args(p, (nx, nlev, ls), m_of(states[fam], m), m_of(forc, m), zero, eta, m_of(traj, m), m_of(out, m),
                                 dt, stream, cover=(cov[m].data_ptr(), ready), members=members)

    def ens(fam, key, ready):
        a = args(fam, 0, res[fam + key], cover[fam + "ens"], ready, (nmem, ms))
        return lambda: fn(entries[fam] + "_ens")(*a)

    def looped(fam, key, ready):
        per_member = [args(fam, m, res[fam + key], cover[fam + "looped"], ready) for m in range(nmem)]

        def call():
            rc = 0
            for a in per_member:
                rc = rc or fn(entries[fam])(*a)
            return rc
        return call
    calls = {}
    for fam in states:
        calls.update({fam + "ens": ens(fam, "ens", 0), fam + "looped": looped(fam, "looped", 0),
                      fam + "ens ready": ens(fam, "ens ready", 1), fam + "looped ready": looped(fam, "looped ready", 1)})
    times = {k: [] for k in calls}
    kernels = {}
    for r in range(rounds + 2):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(call(), name)
            b.record()
            b.synchronize()
            kernels[name] = _lib.last_kernel()
            if r >= 2:                      # two warm-up rounds
                times[name].append(a.elapsed_time(b) * 1e3)
    same = lambda x, y: all(torch.equal(res[x][n], res[y][n]) for n in STATE4)  # noqa: E731
    rec = {"nmem": nmem, "columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "kernels": kernels}
    for f in states:
        rec.update({f + "ens == looped (bits)": same(f + "ens", f + "looped"),
                    f + "ens ready == ens (bits)": same(f + "ens ready", f + "ens"),
                    f + "cover ens == looped (bits)": bool(torch.equal(cover[f + "ens"], cover[f + "looped"])),
                    f + "max |ens - looped| / max |looped|": max(
                        float((res[f + "ens"][n] - res[f + "looped"][n]).abs().max() / res[f + "looped"][n].abs().max())
                        for n in STATE4)})
    for case in cases:
        v = times[case]
        rec[case] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1),
                     "max_us": round(float(np.max(v)), 1)}
    for f in states:
        rec[f + "ens_over_looped"] = round(rec[f + "ens"]["median_us"] / rec[f + "looped"]["median_us"], 3)
        rec[f + "ens_over_looped ready"] = round(rec[f + "ens ready"]["median_us"] / rec[f + "looped ready"]["median_us"], 3)
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 11))
    for shape in opts.get("shapes", SHAPES).split(","):
        dims, prec = shape.split(":")
        nmem, nx = (int(x) for x in dims.split("x"))
        print(json.dumps(measure(nmem, nx, prec, rounds)), flush=True)
        import torch

        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
