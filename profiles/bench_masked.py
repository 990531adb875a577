#!/usr/bin/env python3
"""Masked TL / AD kernels against the dense ones, one process (dev tool; record in docs/TUNING_LOG.md 3.16).
  python profiles/bench_masked.py [--cols=65536] [--precision=double] [--rounds=9] [--reps=10]
Per case: the median over `rounds` of the mean of `reps` back-to-back launches (HIP events), the min-max spread of the
rounds, the words moved per level and column, and the TB/s those words amount to.  The cases are interleaved round by
round, so drift hits all of them alike.  Run each precision as its own process under its own `timeout`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATE4 = ("t", "q", "ql", "qi")
TND4 = ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")


def main():
    import ctypes

    import numpy as np
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import NL_IN, NL_OUT, compile_stencil
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    nx = int(opts.get("cols", 65536))
    rounds, reps = int(opts.get("rounds", 9)), int(opts.get("reps", 10))
    dt_np = np.float64 if opts.get("precision", "double") == "double" else np.float32
    sfx = "f64" if dt_np is np.float64 else "f32"
    nz, dev = 137, torch.device("cuda:0")
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1)
    s = make_state(nx, nz, dtype=dt_np, device=dev)
    eta = torch.as_tensor(eta_levels(nz, dtype=dt_np), device=dev)
    Z = lambda: storage.zeros(nx, nz, dt_np, dev)  # noqa: E731
    state = {k[2:]: storage.logical_view(v) for k, v in s.items()}
    state["qsat"] = Z()
    com = dict(origin=(0, 0, 0), validate_args=False, exec_info=None)
    compile_stencil("saturation", ext)(in_ap=state["ap"], in_t=state["t"], out_qsat=state["qsat"], domain=(nx, 1, nz), **com)
    f = {"in_" + n: state[n] for n in NL_IN}
    pert = {n: Z() for n in NL_IN}
    for n in NL_IN:
        pert[n].copy_(state[n] * 0.01)
    out, out_i = {n: Z() for n in NL_OUT}, {n: Z() for n in NL_OUT}
    adj, nl2 = {n: Z() for n in NL_IN}, {n: Z() for n in NL_OUT}
    dom = dict(domain=(nx, 1, nz + 1), in_eta=eta, dt=3600.0, **com)
    tl = compile_stencil("cloudsc2_tl", ext)
    ad = compile_stencil("cloudsc2_ad", ext)
    adt = compile_stencil("cloudsc2_ad_from_trajectory", ext)
    o_ = lambda d, suffix="": {"out_" + n + suffix: v for n, v in d.items()}  # noqa: E731
    i_ = lambda d: {"in_" + n + "_i": v for n, v in d.items()}  # noqa: E731
    calls, words = {}, {}
    calls["cloudsc2_tl"] = lambda: tl(**f, **i_(pert), **o_(out), **o_(out_i, "_i"), **dom)
    calls["cloudsc2_tl"]()                                  # out_i = the forcing, out = the trajectory fluxes
    words["cloudsc2_tl"] = 52
    # the masked entries, called as autodiff does but on preallocated results (no allocation inside the timed region)
    lib, p = _lib.load(), autodiff._params(ext, nz)
    _, _, ls = storage.field_geometry(state["t"])
    zl, stream = autodiff._zero_line(dev, storage.torch_dtype(dt_np)), int(torch.cuda.current_stream(dev).cuda_stream)

    def tl_masked(have, want, nl):
        a = (ctypes.byref(p), nx, nz, ls, autodiff._ptrs(state, NL_IN), autodiff._ptrs({n: pert[n] for n in have}, NL_IN),
             zl.data_ptr(), eta.data_ptr(), autodiff._ptrs(nl2, NL_OUT) if nl else None,
             autodiff._ptrs({n: out_i[n] for n in want}, NL_OUT), 3600.0, stream)
        fn = getattr(lib, "cloudsc2_tl_masked_" + sfx)
        return lambda: _lib.check(fn(*a), "tl_masked")

    def ad_masked(have, want):
        a = (ctypes.byref(p), nx, nz, ls, autodiff._ptrs(state, NL_IN), autodiff._ptrs({n: out_i[n] for n in have}, NL_OUT),
             zl.data_ptr(), eta.data_ptr(), out["fplsl"].data_ptr(), out["fplsn"].data_ptr(),
             autodiff._ptrs({n: adj[n] for n in want}, NL_IN), 3600.0, stream)
        fn = getattr(lib, "cloudsc2_ad_masked_" + sfx)
        return lambda: _lib.check(fn(*a), "ad_masked")

    # out_i is read by the AD cases and written by the TL cases: the TL cases write the same values again
    calls["tl_masked full"], words["tl_masked full"] = tl_masked(NL_IN, NL_OUT, True), 52
    calls["tl_masked 4dvar"], words["tl_masked 4dvar"] = tl_masked(STATE4, TND4, False), 16 + 4 + 4
    calls["cloudsc2_ad"] = lambda: ad(**f, **i_(out_i), **o_(nl2), **o_(adj, "_i"), **dom)
    words["cloudsc2_ad"] = 70
    calls["ad_from_trajectory"] = lambda: adt(**f, **i_(out_i), traj_fplsl=out["fplsl"], traj_fplsn=out["fplsn"],
                                              **o_(adj, "_i"), **dom)
    words["ad_from_trajectory"] = 44
    calls["ad_masked full"], words["ad_masked full"] = ad_masked(NL_OUT, NL_IN), 44
    calls["ad_masked 4dvar"], words["ad_masked 4dvar"] = ad_masked(TND4, STATE4), 16 + 2 + 4 + 4

    print(f"{nx} columns x {nz} levels, {np.dtype(dt_np).name}, {torch.cuda.get_device_name(0)}", flush=True)
    for _ in range(3):                    # prewarm: clocks and the memory side (measuring-on-mi355x)
        for fn in calls.values():
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / reps * 1e3)
    wsize = np.dtype(dt_np).itemsize
    med_of, spread_of = {}, {}
    for name, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        med_of[name], spread_of[name] = med, ts[-1] - ts[0]
        tbs = words[name] * (nz + 1) * nx * wsize / (med * 1e-6) / 1e12
        print(f"  {name:20s} median {med:9.1f} us   min {ts[0]:9.1f}   max {ts[-1]:9.1f}   spread {100 * (ts[-1] - ts[0]) / med:4.1f} %"
              f"   {words[name]:3d} words/level   {tbs:5.2f} TB/s", flush=True)
    # the two conditions the masked kernels are held to, against the dense kernels timed above
    def verdict(what, ok, detail):
        print(f"  {'PASS' if ok else 'FAIL'}  {what}: {detail}", flush=True)

    for masked, dense in (("tl_masked full", "cloudsc2_tl"), ("ad_masked full", "ad_from_trajectory")):
        over = med_of[masked] - med_of[dense]
        verdict(f"{masked} no slower than {dense} by more than that kernel's spread", over <= spread_of[dense],
                f"{over:+.1f} us against a spread of {spread_of[dense]:.1f} us")
    for masked, denses in (("tl_masked 4dvar", ("cloudsc2_tl",)), ("ad_masked 4dvar", ("cloudsc2_ad", "ad_from_trajectory"))):
        for dense in denses:
            verdict(f"{masked} faster than {dense}", med_of[masked] < med_of[dense],
                    f"{med_of[masked]:.1f} us against {med_of[dense]:.1f} us ({med_of[dense] / med_of[masked]:.2f} x)")


if __name__ == "__main__":
    main()
