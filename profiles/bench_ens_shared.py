#!/usr/bin/env python3
"""Times the NL step, the step's tangent-linear and its adjoint (4D-Var mask: perturbations / adjoints of t, q, ql, qi; perturbed
outputs / forcing on the four tendencies) on an ensemble whose members SHARE every state field but t, q, ql, qi - four ways,
in ONE process with HIP events, the cases interleaved round by round, two warm-up rounds, default placement:

  copy+ens   what the package did for this input before the shared-state entries: the 11 shared fields copied into member-major
             batches (the `expand` materialised), then the `cloudsc2_*_ens_*` launch
  ens        the `cloudsc2_*_ens_*` launch alone, on members that are already materialised
  enss mm    the `cloudsc2_*_enss_*` launch on the shared fields themselves, member-major block order
  enss cm    the same, column-block-major block order (column block * nmem + member)

  python profiles/bench_ens_shared.py [--rounds=R] [--shapes=4x65536:double,8x65536:double,...]

Prints one JSON line per shape: median / min / max microseconds of every case, the words moved per column and level by each
case (counted from the call, see `words`), whether the four give the same sums (of the finite values, with equal counts of the others), and which order the rule of
docs/TUNING_LOG.md 3.27 would pick for this shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE4, TND4 = ("t", "q", "ql", "qi"), ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
SHAPES = ("4x65536:double,8x65536:double,16x65536:double,4x524288:single,8x524288:single,16x524288:single")


def words(nmem, nshared):
    """words per column and level, summed over the members: (read per member, written per member) of each family, and from
    them the four cases.  `enss` is given as a range: every shared line fetched once for all members .. once per member."""
    nown = 15 - nshared
    per = {"nl": (15, 11), "tl": (15 + 4, 4), "ad": (15 + 2 + 4, 4)}    # nl: + qsat_out; tl / ad: the present fields only
    out = {}
    for fam, (rd, wr) in per.items():
        ens = nmem * (rd + wr)
        out[fam] = {"copy+ens": ens + nshared * nmem + nshared, "ens": ens,
                    "enss": [nmem * (rd - nshared + wr) + nshared, ens], "own_fields": nown}
    return out


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
    shared_names = tuple(n for n in names if n not in STATE4)
    new = lambda: storage.zeros_batched(nmem, nx, nz, np_dtype, dev)  # noqa: E731
    s = make_state(nx, nz, dtype=np_dtype, device=dev)
    one = {n: storage.zeros(nx, nz, np_dtype, dev) for n in names}
    for n in names:
        storage.klayout(one[n]).copy_(torch.as_tensor(s["f_" + n], device=dev))
    del s
    # materialised members: member m's own fields are the state's scaled by (1 + m / 1000); the shared ones repeated
    full = {n: new() for n in names}
    for n in names:
        for m in range(nmem):
            full[n][m].copy_(one[n] * (1.0 + 1e-3 * m) if n in STATE4 else one[n])
    part = {n: (one[n].unsqueeze(0) if n in shared_names else full[n]) for n in names}      # [0]: the pointer the call gets
    mask = sum(1 << NL_IN.index(n) for n in shared_names)
    eta = torch.as_tensor(eta_levels(nz, dtype=np_dtype), device=dev)
    dt = 3600.0
    pert = {n: new() for n in STATE4}
    for n in STATE4:
        pert[n].copy_(0.01 * full[n])
    nl, w = autodiff.tl_step_ens(full, pert, eta, dt, ext, want=NL_OUT, write_nl=True)
    traj = {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}
    forc = {n: w[n] for n in TND4}
    del nl, w
    cases = ("copy+ens", "ens", "enss mm", "enss cm")
    # ONE set of result buffers for the four cases (at 16 x 524 288 fp32 columns a batch is 4.6 GB): what a case wrote is
    # compared through float64 sums taken after the timing, one more call each
    res = {"nl": dict({n: new() for n in NL_OUT}, qsat=new()), "tl": {n: new() for n in TND4}, "ad": {n: new() for n in STATE4}}
    _, nlev, ls = storage.field_geometry(full["t"][0])
    ms = storage.direction_stride(full["t"])
    p = autodiff._params(ext, nz)
    zero = autodiff._zero_line(dev, full["t"].dtype)
    stream = int(torch.cuda.current_stream().cuda_stream)
    fn = lambda name: getattr(lib, f"cloudsc2_{name}_{sfx}")  # noqa: E731
    m0 = lambda fields: {n: f[0] for n, f in fields.items()}  # noqa: E731
    geo = (nx, nlev, ls)

    def args(fam, state, r, tail):
        if fam == "nl":
            return (ctypes.byref(p), nx, nz, ls, autodiff._ptrs(m0(state), NL_IN), None, 0.0, r["qsat"][0].data_ptr(),
                    eta.data_ptr(), autodiff._ptrs(m0({n: f for n, f in r.items() if n != "qsat"}), NL_OUT), dt, stream) + tail
        if fam == "tl":
            return autodiff._tl_args(p, geo, m0(state), m0(pert), zero, eta, None, m0(r), dt, stream, tail)
        return autodiff._ad_args(p, geo, m0(state), m0(forc), zero, eta, m0(traj), m0(r), dt, stream, members=tail)

    entry = {"nl": "nl_fused", "tl": "tl_step", "ad": "ad_step"}
    calls = {}
    for fam in ("nl", "tl", "ad"):
        a_ens = a_copy = args(fam, full, res[fam], (nmem, ms))
        a_mm = args(fam, part, res[fam], (nmem, ms, mask | _lib.ENSS_MEMBER_MAJOR, 0))
        a_cm = args(fam, part, res[fam], (nmem, ms, mask | _lib.ENSS_COLUMN_MAJOR, 0))

        def copy_then(fam=fam, a=a_copy):
            for n in shared_names:      # the `expand` of the shared field, materialised per call
                full[n].copy_(one[n].unsqueeze(0).expand(nmem, *one[n].shape))
            return fn(entry[fam] + "_ens")(*a)
        calls[fam, "copy+ens"] = copy_then
        calls[fam, "ens"] = lambda fam=fam, a=a_ens: fn(entry[fam] + "_ens")(*a)
        calls[fam, "enss mm"] = lambda fam=fam, a=a_mm: fn(entry[fam] + "_enss")(*a)
        calls[fam, "enss cm"] = lambda fam=fam, a=a_cm: fn(entry[fam] + "_enss")(*a)

    times = {k: [] for k in calls}
    for r in range(rounds + 2):
        for key, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(call(), " ".join(key))
            b.record()
            b.synchronize()
            if r >= 2:                      # two warm-up rounds
                times[key].append(a.elapsed_time(b) * 1e3)
    rec = {"nmem": nmem, "columns": nx, "precision": prec, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "shared_fields": len(shared_names), "words_per_column_level": words(nmem, len(shared_names))}
    for fam in ("nl", "tl", "ad"):
        sums = {}
        for c in cases:
            for f in res[fam].values():
                f.fill_(float("nan"))
            _lib.check(calls[fam, c](), c)
            # per result: (float64 sum of the finite values, how many are not finite).  The synthetic adjoint overflows fp32
            # in a few columns with any library (docs/TUNING_LOG.md 3.11): those count, they do not poison the sum
            sums[c] = [(float(torch.nan_to_num(f[:, :, :, :nz].double(), nan=0.0, posinf=0.0, neginf=0.0).sum()),
                        int((~torch.isfinite(f[:, :, :, :nz])).sum())) for f in res[fam].values()]
        rec[f"{fam} same sums"] = all(sums[c] == sums["ens"] for c in cases)
        rec[f"{fam} not finite"] = sum(k for _, k in sums["ens"])
        for c in cases:
            v = times[fam, c]
            rec[f"{fam} {c}"] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1),
                                 "max_us": round(float(np.max(v)), 1)}
        mm, cm, ens = rec[f"{fam} enss mm"], rec[f"{fam} enss cm"], rec[f"{fam} ens"]
        rec[f"{fam} enss_mm_over_ens"] = round(mm["median_us"] / ens["median_us"], 3)
        rec[f"{fam} enss_cm_over_ens"] = round(cm["median_us"] / ens["median_us"], 3)
        rec[f"{fam} enss_mm_over_copy"] = round(mm["median_us"] / rec[f"{fam} copy+ens"]["median_us"], 3)
        # the rule: column-major only if its median beats member-major's by more than member-major's min-max spread
        rec[f"{fam} cm_wins"] = bool(mm["median_us"] - cm["median_us"] > mm["max_us"] - mm["min_us"])
    return rec


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    rounds = int(opts.get("rounds", 9))
    import __graft_entry__ as ge

    ge.build()
    for shape in opts.get("shapes", SHAPES).split(","):
        dims, prec = shape.split(":")
        nmem, nx = (int(x) for x in dims.split("x"))
        print(json.dumps(measure(nmem, nx, prec, rounds)), flush=True)
        import gc

        import torch

        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
