#!/usr/bin/env python3
"""Times D tangent-linear directions on one trajectory with HIP events: ONE multi-direction launch (cloudsc2_tl_multi_step /
cloudsc2_tl_multi) against D single launches (cloudsc2_tl_step / cloudsc2_tl_masked), in ONE process with the cases
interleaved round by round, for the 4D-Var mask (perturbations of t, q, ql, qi; the four perturbed tendencies wanted):

  step    D x cloudsc2_tl_step      D x (15 + 4 + 4) words per level and column     cloudsc2_tl_multi_step   15 + 8 D
  masked  D x cloudsc2_tl_masked    D x (16 + 4 + 4)                                cloudsc2_tl_multi        16 + 8 D

  python profiles/bench_tl_multi.py [--rounds=R] [--sizes=65536:double,524288:single] [--dirs=2,4,8]

Prints one JSON line per size: median / min microseconds of every case, microseconds per direction, the multi / looped
ratio per family and D, and whether the two wrote the same bits at the timed size.  `autodiff.MULTI_WIDTH` is chosen from
these lines (docs/TUNING_LOG.md 3.18)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
PEAK = 8.0e12


def measure(nx, prec, rounds, dirs):
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
    ext = dict(default_externals(), NLEV=nz)
    lib = _lib.load()
    s = make_state(nx, nz, dtype=np_dtype, device=dev)
    state = {k[2:]: storage.from_klayout(v, np_dtype, dev) for k, v in s.items()}
    del s
    eta = torch.as_tensor(eta_levels(nz, dtype=np_dtype), device=dev)
    dt = 3600.0
    qsat = storage.zeros(nx, nz, np_dtype, dev)
    compile_stencil("saturation", ext)(in_ap=state["ap"], in_t=state["t"], out_qsat=qsat, origin=(0, 0, 0), domain=(nx, 1, nz),
                                        validate_args=False, exec_info=None)
    full = dict(state, qsat=qsat)
    dmax = max(dirs)
    # direction d: (d + 1) % of the state, sign alternating - independent enough for a timing, reproducible
    pert = {n: storage.zeros_batched(dmax, nx, nz, np_dtype, dev) for n in STATE4}
    for n in STATE4:
        for d in range(dmax):
            pert[n][d].copy_((-1.0) ** d * 0.01 * (d + 1) * state[n])
    out_multi = {n: storage.zeros_batched(dmax, nx, nz, np_dtype, dev) for n in TND4}
    out_loop = {n: storage.zeros_batched(dmax, nx, nz, np_dtype, dev) for n in TND4}
    dstride = storage.direction_stride(pert["t"])
    _, _, ls = storage.field_geometry(qsat)
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, qsat.dtype).data_ptr()
    stream = int(torch.cuda.current_stream().cuda_stream)
    P, head = autodiff._ptrs, (ctypes.byref(p), nx, nz, ls)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    ins = P(full, NL_IN)
    in_d = [P({n: f[d] for n, f in pert.items()}, NL_IN) for d in range(dmax)]
    loop_d = [P({n: f[d] for n, f in out_loop.items()}, NL_OUT) for d in range(dmax)]
    multi0 = P({n: f[0] for n, f in out_multi.items()}, NL_OUT)

    def looped(single, ndir):
        def call():
            rc = 0
            for d in range(ndir):
                rc = rc or fn(single)(*head, ins, in_d[d], zero, eta.data_ptr(), None, loop_d[d], dt, stream)
            return rc
        return call

    def multi(entry, ndir):
        return lambda: fn(entry)(*head, ins, in_d[0], zero, eta.data_ptr(), None, multi0, dt, stream, ndir, dstride, dstride)

    families = {"step": ("tl_step", "tl_multi_step", 15), "masked": ("tl_masked", "tl_multi", 16)}
    calls = {}
    for fam, (single, entry, _) in families.items():
        for d in dirs:
            calls[f"{fam} {d} x {single}"] = looped(single, d)
            calls[f"{fam} {entry} D={d}"] = multi(entry, d)
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
    rec = {"columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    for fam, (single, entry, nstate) in families.items():
        # same bits?  (the last multi launch of the rounds was D = max(dirs), as was the last loop)
        _lib.check(looped(single, dmax)(), single)
        _lib.check(multi(entry, dmax)(), entry)
        torch.cuda.synchronize()
        rec[f"{fam} bit_equal"] = all(torch.equal(out_multi[n], out_loop[n]) for n in TND4)
        rec[f"{fam} max_abs_diff"] = max(float((out_multi[n] - out_loop[n]).abs().max()) for n in TND4)
        for d in dirs:
            for key, words in ((f"{fam} {d} x {single}", d * (nstate + 8)), (f"{fam} {entry} D={d}", nstate + 8 * d)):
                v = times[key]
                med = float(np.median(v))
                bytes_ = words * nz * nx * item
                rec[key] = {"median_us": round(med, 1), "min_us": round(float(np.min(v)), 1), "us_per_direction": round(med / d, 1),
                            "words": words, "fraction_of_8TBs": round(bytes_ / (med * 1e-6) / PEAK, 3)}
            rec[f"{fam} multi_over_looped D={d}"] = round(rec[f"{fam} {entry} D={d}"]["median_us"]
                                                          / rec[f"{fam} {d} x {single}"]["median_us"], 3)
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 15))
    sizes = [s.split(":") for s in opts.get("sizes", "65536:double,524288:single").split(",")]
    dirs = [int(d) for d in opts.get("dirs", "2,4,8").split(",")]
    import __graft_entry__ as ge

    ge.build()
    for nx, prec in sizes:
        print(json.dumps(measure(int(nx), prec, rounds, dirs)), flush=True)


if __name__ == "__main__":
    main()
