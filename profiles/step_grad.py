#!/usr/bin/env python3
"""Times the derivative of the whole step (saturation + cloudsc2_nl) with HIP events, fused against composed, in ONE process
with interleaved rounds, for the header's example mask (forcing on the four tendencies; adjoints of t, q, ql, qi;
perturbations of the same four inputs, perturbed tendencies wanted):

  AD  fused      cloudsc2_ad_step                                              25 words per level and column
      composed   cloudsc2_ad_masked (wanting qsat too) + cloudsc2_saturation_ad    27 + 3 + 2 x 1 (t read-modify-write)
  TL  fused      cloudsc2_tl_step                                              15 + 4 + 4 = 23 words
      composed   cloudsc2_saturation_tl + cloudsc2_tl_masked                   (2 + 1 + 1) + (16 + 5 + 4)

  python profiles/step_grad.py [--rounds=R] [--sizes=65536:double,524288:single]

Prints one JSON line per size: median / min microseconds of each of the four, the fused / composed ratios and the fraction
of 8 TB/s that the fused kernels' algorithmic bytes give."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
PEAK = 8.0e12


def measure(nx, prec, rounds):
    import ctypes

    import numpy as np
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import NL_IN, NL_OUT
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    nz = 137
    np_dtype = np.float64 if prec == "double" else np.float32
    sfx = "f64" if prec == "double" else "f32"
    dev = torch.device("cuda:0")
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1)
    lib = _lib.load()
    s = make_state(nx, nz, dtype=np_dtype, device=dev)
    state = {k[2:]: storage.from_klayout(v, np_dtype, dev) for k, v in s.items()}
    del s
    eta = torch.as_tensor(eta_levels(nz, dtype=np_dtype), device=dev)
    dt = 3600.0
    new = lambda: storage.zeros(nx, nz, np_dtype, dev)  # noqa: E731
    # the step itself: qsat and the trajectory fluxes
    nl = {n: new() for n in NL_OUT}
    qsat = new()
    compile_stencil("cloudsc2_nl_saturation", ext)(**{"in_" + n: f for n, f in state.items() if n != "qsat"}, out_qsat=qsat,
                                                   **{"out_" + n: f for n, f in nl.items()}, in_eta=eta, dt=dt,
                                                   origin=(0, 0, 0), domain=(nx, 1, nz + 1), validate_args=False, exec_info=None)
    full = dict(state, qsat=qsat)
    step = {n: f for n, f in full.items() if n != "qsat"}
    pert = {n: new().copy_(0.01 * state[n]) for n in STATE4}
    _, forcing = autodiff.tl_step(step, pert, eta, dt, ext, want=TND4)
    adj = {n: new() for n in STATE4 + ("qsat",)}
    out_i = {n: new() for n in TND4}
    qsat_i = new()
    _, _, ls = storage.field_geometry(qsat)
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, qsat.dtype).data_ptr()
    stream = int(torch.cuda.current_stream().cuda_stream)
    P, head = autodiff._ptrs, (ctypes.byref(p), nx, nz, ls)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    in_step, in_full, frc = P(step, NL_IN), P(full, NL_IN), P(forcing, NL_OUT)
    adj4, adj5 = P({n: adj[n] for n in STATE4}, NL_IN), P(adj, NL_IN)
    pert4, pert5, outs = P(pert, NL_IN), P(dict(pert, qsat=qsat_i), NL_IN), P(out_i, NL_OUT)
    tl_, tn_ = nl["fplsl"].data_ptr(), nl["fplsn"].data_ptr()

    def ad_fused():
        return fn("ad_step")(*head, in_step, frc, zero, eta.data_ptr(), tl_, tn_, adj4, dt, stream)

    def ad_composed():
        rc = fn("ad_masked")(*head, in_full, frc, zero, eta.data_ptr(), tl_, tn_, adj5, dt, stream)
        return rc or fn("saturation_ad")(*head, state["ap"].data_ptr(), state["t"].data_ptr(), adj["qsat"].data_ptr(), None,
                                         adj["t"].data_ptr(), 1, stream)

    def tl_fused():
        return fn("tl_step")(*head, in_step, pert4, zero, eta.data_ptr(), None, outs, dt, stream)

    def tl_composed():
        rc = fn("saturation_tl")(*head, state["ap"].data_ptr(), state["t"].data_ptr(), None, pert["t"].data_ptr(), None,
                                 qsat_i.data_ptr(), stream)
        return rc or fn("tl_masked")(*head, in_full, pert5, zero, eta.data_ptr(), None, outs, dt, stream)

    calls = {"ad_step": ad_fused, "ad_masked+saturation_ad": ad_composed, "tl_step": tl_fused,
             "saturation_tl+tl_masked": tl_composed}
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
    item = np.dtype(np_dtype).itemsize
    words = {"ad_step": 25, "tl_step": 23}
    rec = {"columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        rec[k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1)}
    for k, w in words.items():
        bytes_ = w * nz * nx * item
        rec[k]["algorithmic_bytes"] = bytes_
        rec[k]["fraction_of_8TBs"] = round(bytes_ / (rec[k]["median_us"] * 1e-6) / PEAK, 3)
    rec["ad_fused_over_composed"] = round(rec["ad_step"]["median_us"] / rec["ad_masked+saturation_ad"]["median_us"], 3)
    rec["tl_fused_over_composed"] = round(rec["tl_step"]["median_us"] / rec["saturation_tl+tl_masked"]["median_us"], 3)
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 15))
    sizes = [s.split(":") for s in opts.get("sizes", "65536:double,524288:single").split(",")]
    import __graft_entry__ as ge

    ge.build()
    for nx, prec in sizes:
        print(json.dumps(measure(int(nx), prec, rounds)), flush=True)


if __name__ == "__main__":
    main()
