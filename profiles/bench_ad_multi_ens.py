#!/usr/bin/env python3
"""Times an ENSEMBLE of Jacobian row blocks with HIP events: ONE members-times-directions launch
(cloudsc2_ad_multi_step_ens) against the loop over the members of cloudsc2_ad_multi_step - the path there was before the
entry existed, and the baseline - in one process per configuration, the two cases interleaved round by round.  The 4D-Var
mask of the step family: forcing on the four tendencies, adjoints of t, q, ql, qi; 17 + 8 D words per member, level and
column either way.

  python profiles/bench_ad_multi_ens.py [--rounds=R] [--members=4,16,64] [--columns=1024,16384] [--dirs=2,4,8]
                                        [--precisions=double,single] [--max-gib=48] [--timeout=240]

Every configuration (members, columns per member, precision) runs in a child process of its own under `--timeout` seconds,
with at most 16 CPU threads; the first child that fails or runs out of time ends the run.  A direction count whose fields
would not fit `--max-gib` is left out and reported.  Prints one JSON line per configuration: median, min and max
microseconds of both cases per D, the ratio of the medians, and `pays`: whether the one launch beats the loop by more than
the loop's own min-max spread in the same run (the rule of docs/TUNING_LOG.md 3.19).  docs/TUNING_LOG.md 3.26 holds the
table."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
NZ = 137


def footprint_gib(nmem, nx, item, ndir):
    """15 state fields, 2 trajectory fluxes, 4 forcings and 4 results of ndir directions each, per member"""
    return nmem * nx * (NZ + 1) * item * (17 + 8 * ndir) / 2 ** 30


def measure(nmem, nx, prec, rounds, dirs):
    import ctypes

    import numpy as np
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN, NL_OUT
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    torch.set_num_threads(min(16, torch.get_num_threads()))
    np_dtype = np.float64 if prec == "double" else np.float32
    sfx = "f64" if prec == "double" else "f32"
    dev = torch.device("cuda:0")
    ext = dict(default_externals(), NLEV=NZ, AD_TRAJ_FIX=1)      # what the derivative rules of autodiff.py launch
    lib = _lib.load()
    # every member: the synthetic state of nmem * nx columns, cut into members
    s = make_state(nmem * nx, NZ, dtype=np_dtype, device=dev)
    names = tuple(n for n in NL_IN if n != "qsat")
    state = {}
    for n in names:
        f = storage.zeros_batched(nmem, nx, NZ, np_dtype, dev)
        whole = torch.as_tensor(s["f_" + n], device=dev)           # [level][column]
        for m in range(nmem):
            storage.klayout(f[m]).copy_(whole[:, m * nx:(m + 1) * nx])
        state[n] = f
    del s
    eta = torch.as_tensor(eta_levels(NZ, dtype=np_dtype), device=dev)
    dt = 3600.0
    pert = {n: 0.01 * state[n] for n in STATE4}
    nl, w = autodiff.tl_step_ens(state, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    del pert
    traj = {n: nl[n] for n in ("fplsl", "fplsn")}
    dmax = max(dirs)
    _, _, ls = storage.field_geometry(state["t"][0])
    field = (NZ + 1) * ls
    new = lambda: storage.zeros_batched(nmem * dmax, nx, NZ, np_dtype, dev).unflatten(0, (nmem, dmax))  # noqa: E731
    forc = {n: new() for n in TND4}
    for n in TND4:
        for d in range(dmax):       # direction d: (d + 1) times the forcing, sign alternating
            forc[n][:, d].copy_((-1.0) ** d * (d + 1) * w[n])
    del w, nl
    out = {n: new() for n in STATE4}    # both cases write the same fields: the results are compared in the GPU tests
    ms = storage.direction_stride(state["t"])
    p = autodiff._params(ext, NZ)
    zero = autodiff._zero_line(dev, state["t"].dtype).data_ptr()
    stream = int(torch.cuda.current_stream().cuda_stream)
    P, head = autodiff._ptrs, (ctypes.byref(p), nx, NZ, ls)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    member = [(P({n: f[m] for n, f in state.items()}, NL_IN), P({n: f[m, 0] for n, f in forc.items()}, NL_OUT),
               traj["fplsl"][m].data_ptr(), traj["fplsn"][m].data_ptr(), P({n: f[m, 0] for n, f in out.items()}, NL_IN))
              for m in range(nmem)]

    def looped(ndir):
        def call():
            rc = 0
            for ins, adj, tl, tn, res in member:
                rc = rc or fn("ad_multi_step")(*head, ins, adj, zero, eta.data_ptr(), tl, tn, res, dt, stream, ndir, field, field)
            return rc
        return call

    def one(ndir):
        ins, adj, tl, tn, res = member[0]
        return lambda: fn("ad_multi_step_ens")(*head, ins, adj, zero, eta.data_ptr(), tl, tn, res, dt, stream, ndir, field,
                                               field, nmem, ms, dmax * field, dmax * field)

    calls = {}
    for d in dirs:
        calls[f"loop D={d}"] = looped(d)
        calls[f"one D={d}"] = one(d)
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
    rec = {"members": nmem, "columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    for d in dirs:
        for key in (f"loop D={d}", f"one D={d}"):
            v = times[key]
            rec[key] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1),
                        "max_us": round(float(np.max(v)), 1)}
        lo, on = rec[f"loop D={d}"], rec[f"one D={d}"]
        rec[f"one_over_loop D={d}"] = round(on["median_us"] / lo["median_us"], 3)
        rec[f"pays D={d}"] = bool(lo["median_us"] - on["median_us"] > lo["max_us"] - lo["min_us"])
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 15))
    dirs = [int(d) for d in opts.get("dirs", "2,4,8").split(",")]
    if "child" in opts:
        nmem, nx, prec = opts["child"].split(":")
        print(json.dumps(measure(int(nmem), int(nx), prec, rounds, dirs)), flush=True)
        return
    import __graft_entry__ as ge

    ge.build()
    max_gib = float(opts.get("max-gib", 48))
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(min(16, int(env.get(var, 16))))
    for prec in opts.get("precisions", "double,single").split(","):
        for nx in (int(v) for v in opts.get("columns", "1024,16384").split(",")):
            for nmem in (int(v) for v in opts.get("members", "4,16,64").split(",")):
                item = 8 if prec == "double" else 4
                fit = [d for d in dirs if footprint_gib(nmem, nx, item, max(x for x in dirs if x <= d)) <= max_gib]
                fit = [d for d in fit if footprint_gib(nmem, nx, item, max(fit)) <= max_gib]
                if len(fit) < len(dirs):
                    print(json.dumps({"members": nmem, "columns": nx, "precision": prec,
                                      "left_out_dirs": [d for d in dirs if d not in fit], "max_gib": max_gib}), flush=True)
                if not fit:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), f"--child={nmem}:{nx}:{prec}", f"--rounds={rounds}",
                       "--dirs=" + ",".join(map(str, fit))]
                done = subprocess.run(cmd, env=env, timeout=float(opts.get("timeout", 240)))   # raises when it runs out
                if done.returncode != 0:
                    sys.exit(f"{cmd[2]} ended with {done.returncode}: nothing further is started")


if __name__ == "__main__":
    main()
