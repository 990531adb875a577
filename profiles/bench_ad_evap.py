#!/usr/bin/env python3
"""Times the backward of the 4D-Var mask (forcing on the four tendencies, adjoints of t, q, ql, qi) under LEVAPLS2 at
dt = 60 s with HIP events, in ONE process with the cases interleaved round by round:

  (a) the dense path        cloudsc2_ad with ten forcing fields (six of them zero) and 26 scratch results: 70 words per
                            level and column; for the step, cloudsc2_saturation_ad (accumulating) behind it
  (b) one trajectory launch cloudsc2_ad_evap / cloudsc2_ad_evap_step: 19 + 19 + 8 = 46 words (step: 18 + 18 + 8);
                            with cover_ready 19 + 8 = 27
  (c) 8 cotangents          8 x (a) against ONE cloudsc2_ad_evap_multi launch (38 + 64 words) and the same with cover_ready

  python profiles/bench_ad_evap.py [--rounds=R] [--sizes=65536:double,524288:single]

Prints one JSON line per size: median / min microseconds and the min-max spread of every case.  docs/TUNING_LOG.md 3.22
records the lines and says when to set `autodiff.EVAP_ADJOINT = "trajectory"`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
NDIR = 8


def measure(nx, prec, rounds):
    import ctypes

    import numpy as np
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN, NL_OUT
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    nz, dt = 137, 60.0
    np_dtype = np.float64 if prec == "double" else np.float32
    sfx = "f64" if prec == "double" else "f32"
    dev = torch.device("cuda:0")
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1, LEVAPLS2=True)
    lib = _lib.load()
    s = make_state(nx, nz, dtype=np_dtype, device=dev)
    state = {k[2:]: storage.from_klayout(v, np_dtype, dev) for k, v in s.items()}
    del s
    new = lambda: storage.zeros(nx, nz, np_dtype, dev)  # noqa: E731
    eta = torch.as_tensor(eta_levels(nz, dtype=np_dtype), device=dev)
    state["qsat"] = new()
    geo = dict(origin=(0, 0, 0), validate_args=False, exec_info=None)
    compile_stencil("saturation", ext)(in_ap=state["ap"], in_t=state["t"], out_qsat=state["qsat"], domain=(nx, 1, nz), **geo)
    nl = {n: new() for n in NL_OUT}
    compile_stencil("cloudsc2_nl", ext)(**{"in_" + n: state[n] for n in NL_IN}, **{"out_" + n: f for n, f in nl.items()},
                                         in_eta=eta, dt=dt, domain=(nx, 1, nz + 1), **geo)
    step_in = {n: state[n] for n in NL_IN if n != "qsat"}
    forc = {n: storage.zeros_batched(NDIR, nx, nz, np_dtype, dev) for n in TND4}
    for n in TND4:
        for d in range(NDIR):
            forc[n][d].copy_((-1.0) ** d * (d + 1) * nl[n])
    # (a): what autodiff._dense_ad allocates per backward is allocated once here - the launches alone are timed
    dense_args = {"in_" + n: state[n] for n in NL_IN}
    dense_args.update({"in_" + n + "_i": new() for n in NL_OUT if n not in TND4})
    dense_args.update({"out_" + n: new() for n in NL_OUT})
    dense_adj = {n: new() for n in NL_IN}
    dense_args.update({"out_" + n + "_i": f for n, f in dense_adj.items()})
    dense_st = compile_stencil("cloudsc2_ad", ext)

    def dense(d, step):
        dense_st(**dense_args, **{"in_" + n + "_i": forc[n][d] for n in TND4}, in_eta=eta, dt=dt, domain=(nx, 1, nz + 1), **geo)
        if step:
            autodiff.saturation_ad(state["ap"], state["t"], dense_adj["qsat"], ext, want=("ap", "t"),
                                   into={"ap": dense_adj["ap"], "t": dense_adj["t"]})
        return 0

    out = {n: storage.zeros_batched(NDIR, nx, nz, np_dtype, dev) for n in STATE4}
    cover = new()
    dstride = storage.direction_stride(forc["tnd_t"])
    _, _, ls = storage.field_geometry(state["t"])
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, state["t"].dtype).data_ptr()
    stream = int(torch.cuda.current_stream().cuda_stream)
    P, head = autodiff._ptrs, (ctypes.byref(p), nx, nz, ls)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    mid = (zero, eta.data_ptr(), nl["fplsl"].data_ptr(), nl["fplsn"].data_ptr())
    in0, out0 = P({n: forc[n][0] for n in TND4}, NL_OUT), P({n: out[n][0] for n in STATE4}, NL_IN)

    def single(entry, st, ready):
        return lambda: fn(entry)(*head, P(st, NL_IN), in0, *mid, out0, dt, cover.data_ptr(), ready, stream)

    def multi(ready):
        return lambda: fn("ad_evap_multi")(*head, P(state, NL_IN), in0, *mid, out0, dt, stream, NDIR, dstride, dstride,
                                           cover.data_ptr(), ready)

    calls = {"a dense cloudsc2_ad": lambda: dense(0, False),
             "a dense cloudsc2_ad + saturation_ad (step)": lambda: dense(0, True),
             "b ad_evap": single("ad_evap", state, 0), "b ad_evap cover_ready": single("ad_evap", state, 1),
             "b ad_evap_step": single("ad_evap_step", step_in, 0), "b ad_evap_step cover_ready": single("ad_evap_step", step_in, 1),
             f"c {NDIR} x dense cloudsc2_ad": lambda: [dense(d, False) for d in range(NDIR)] and 0,
             f"c ad_evap_multi D={NDIR}": multi(0), f"c ad_evap_multi D={NDIR} cover_ready": multi(1)}
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
    rec = {"columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    for key, v in times.items():
        rec[key] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1),
                    "spread_us": round(float(np.max(v) - np.min(v)), 1)}
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 15))
    sizes = [s.split(":") for s in opts.get("sizes", "65536:double,524288:single").split(",")]
    import __graft_entry__ as ge

    ge.build()
    for nx, prec in sizes:
        print(json.dumps(measure(int(nx), prec, rounds)), flush=True)
        import torch

        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
