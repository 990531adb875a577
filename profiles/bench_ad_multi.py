#!/usr/bin/env python3
"""Times D adjoint directions (cotangents) on one trajectory with HIP events: ONE multi-direction launch
(cloudsc2_ad_multi_step / cloudsc2_ad_multi) against D single launches (cloudsc2_ad_step / cloudsc2_ad_masked), in ONE
process with the cases interleaved round by round, on two masks:

  4dvar   forcing on the four tendencies, adjoints of t, q, ql, qi
          step    D x cloudsc2_ad_step      D x (15 + 2 + 4 + 4) words per level and column   cloudsc2_ad_multi_step   17 + 8 D
          masked  D x cloudsc2_ad_masked    D x (16 + 2 + 4 + 4)                              cloudsc2_ad_multi        18 + 8 D
  full    forcing on the nine outputs the adjoint reads (all but covptot), every adjoint wanted
          step    D x (15 + 2 + 9 + 15)     cloudsc2_ad_multi_step   17 + 24 D
          masked  D x (16 + 2 + 9 + 16)     cloudsc2_ad_multi        18 + 25 D

  python profiles/bench_ad_multi.py [--rounds=R] [--sizes=65536:double,524288:single] [--dirs=2,4,8]

Prints one JSON line per size: median / min microseconds and the min-max spread of every case, microseconds per direction,
the multi / looped ratio per family, mask and D, and whether the two wrote the same bits at the timed size (if not: the
largest difference relative to a field's largest magnitude, and whether non-finite values sit in the same places).
`autodiff.AD_MULTI_WIDTH` is chosen from these lines (docs/TUNING_LOG.md 3.19)."""
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
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1)      # what the derivative rules of autodiff.py launch
    lib = _lib.load()
    s = make_state(nx, nz, dtype=np_dtype, device=dev)
    state = {k[2:]: storage.from_klayout(v, np_dtype, dev) for k, v in s.items()}
    del s
    eta = torch.as_tensor(eta_levels(nz, dtype=np_dtype), device=dev)
    dt = 3600.0
    # forcing and trajectory: the perturbed outputs of the step's tangent-linear for a 1 % perturbation of t, q, ql, qi, and
    # its NL outputs (qsat included: the masked family runs on the step's own qsat)
    step_in = {n: state[n] for n in NL_IN if n != "qsat"}
    pert = {n: storage.zeros(nx, nz, np_dtype, dev) for n in STATE4}
    for n in STATE4:
        pert[n].copy_(0.01 * state[n])
    nl, w = autodiff.tl_step(step_in, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    del pert
    qsat = storage.zeros(nx, nz, np_dtype, dev)
    compile_stencil("saturation", ext)(in_ap=state["ap"], in_t=state["t"], out_qsat=qsat, origin=(0, 0, 0), domain=(nx, 1, nz),
                                        validate_args=False, exec_info=None)
    full = dict(step_in, qsat=qsat)
    dmax = max(dirs)
    full_have = tuple(n for n in NL_OUT if n != "covptot")
    # direction d: (d + 1) times the forcing, sign alternating - independent enough for a timing, reproducible
    forc = {n: storage.zeros_batched(dmax, nx, nz, np_dtype, dev) for n in full_have}
    for n in full_have:
        for d in range(dmax):
            forc[n][d].copy_((-1.0) ** d * (d + 1) * w[n])
    del w
    out_multi = {n: storage.zeros_batched(dmax, nx, nz, np_dtype, dev) for n in NL_IN}
    out_loop = {n: storage.zeros_batched(dmax, nx, nz, np_dtype, dev) for n in NL_IN}
    dstride = storage.direction_stride(forc["tnd_t"])
    _, _, ls = storage.field_geometry(state["t"])
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, state["t"].dtype).data_ptr()
    stream = int(torch.cuda.current_stream().cuda_stream)
    P, head = autodiff._ptrs, (ctypes.byref(p), nx, nz, ls)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    tail = (eta.data_ptr(), nl["fplsl"].data_ptr(), nl["fplsn"].data_ptr())
    families = {"step": ("ad_step", "ad_multi_step", step_in, 15), "masked": ("ad_masked", "ad_multi", full, 16)}
    masks = {"4dvar": (TND4, lambda names: STATE4), "full": (full_have, lambda names: names)}

    calls, words, wanted = {}, {}, {}
    for fam, (single, entry, st, nstate) in families.items():
        ins = P(st, NL_IN)
        for mask, (have, want_of) in masks.items():
            want = tuple(want_of(tuple(st)))
            wanted[fam, mask] = want
            in_d = [P({n: forc[n][d] for n in have}, NL_OUT) for d in range(dmax)]
            loop_d = [P({n: out_loop[n][d] for n in want}, NL_IN) for d in range(dmax)]
            multi0 = P({n: out_multi[n][0] for n in want}, NL_IN)
            per_dir = len(have) + len(want)

            def looped(ndir, single=single, ins=ins, in_d=in_d, loop_d=loop_d):
                def call():
                    rc = 0
                    for d in range(ndir):
                        rc = rc or fn(single)(*head, ins, in_d[d], zero, *tail, loop_d[d], dt, stream)
                    return rc
                return call

            def multi(ndir, entry=entry, ins=ins, in_d=in_d, multi0=multi0):
                return lambda: fn(entry)(*head, ins, in_d[0], zero, *tail, multi0, dt, stream, ndir, dstride, dstride)

            for d in dirs:
                calls[f"{fam} {mask} {d} x {single}"] = looped(d)
                words[f"{fam} {mask} {d} x {single}"] = d * (nstate + 2 + per_dir)
                calls[f"{fam} {mask} {entry} D={d}"] = multi(d)
                words[f"{fam} {mask} {entry} D={d}"] = nstate + 2 + d * per_dir
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
    for fam, (single, entry, _, _) in families.items():
        for mask in masks:
            # same bits?  D = max(dirs), both ways, at the timed size
            want = wanted[fam, mask]
            _lib.check(calls[f"{fam} {mask} {dmax} x {single}"](), single)
            _lib.check(calls[f"{fam} {mask} {entry} D={dmax}"](), entry)
            torch.cuda.synchronize()
            rec[f"{fam} {mask} bit_equal"] = all(torch.equal(out_multi[n], out_loop[n]) for n in want)
            # not bit-equal (hipcc contracts the shared level functions per kernel): the largest difference relative to the
            # field's largest finite magnitude, and whether the two have their non-finite values in the same places
            rel, same, bad = 0.0, True, 0
            for n in want:
                a, b = out_multi[n], out_loop[n]
                fa, fb = torch.isfinite(a), torch.isfinite(b)
                same = same and bool(torch.equal(fa, fb))
                bad += int((~fb).sum())
                both = fa & fb
                scale = float(b[both].abs().max()) if bool(both.any()) else 0.0
                if scale > 0.0:
                    rel = max(rel, float((a[both] - b[both]).abs().max()) / scale)
                del a, b, fa, fb, both
            rec[f"{fam} {mask} max_rel_diff"] = rel
            rec[f"{fam} {mask} non_finite_in_looped"] = bad
            rec[f"{fam} {mask} non_finite_in_same_places"] = same
            for d in dirs:
                for key in (f"{fam} {mask} {d} x {single}", f"{fam} {mask} {entry} D={d}"):
                    v = times[key]
                    med = float(np.median(v))
                    bytes_ = words[key] * nz * nx * item
                    rec[key] = {"median_us": round(med, 1), "min_us": round(float(np.min(v)), 1),
                                "spread_us": round(float(np.max(v) - np.min(v)), 1), "us_per_direction": round(med / d, 1),
                                "words": words[key], "fraction_of_8TBs": round(bytes_ / (med * 1e-6) / PEAK, 3)}
                rec[f"{fam} {mask} multi_over_looped D={d}"] = round(rec[f"{fam} {mask} {entry} D={d}"]["median_us"]
                                                                     / rec[f"{fam} {mask} {d} x {single}"]["median_us"], 3)
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
        import torch

        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
