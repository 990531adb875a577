"""What tests/test_vertical_grids.py and tests/test_threshold_ties.py share: vertical grids other than the synthetic one
(`eta_family`), the tropopause window a grid gives (`tropopause_window`, the kernels' `build_level_table` in Python), a
state with inputs planted exactly on the scheme's thresholds (`tie_case`), and one way to hold every kernel family that
reads `eta` to the NumPy oracle (`Held`).

Bounds are the suite's own: `assert_close` at its default for NL outputs, 100 x for TL outputs and adjoints against the
oracle (tests/test_hip_masked.py, test_hip_ad_multi.py, test_hip_ensemble.py), 1e4 x eps for the transpose identity.

`torch` and the package are imported inside functions, so that collecting a test module needs neither."""
import numpy as np

from derivative_support import STEP_IN, Box, Ens, _once, ens_ad, ens_nl, ens_tl, host_case, host_directions
from helpers import (NL_IN, NL_OUT, TOL, adjoint_nlev_of, assert_close, eta_levels, externals, from_device, nl_case, nlev_of,
                     oracle, run_oracle_ad, run_oracle_nl, run_oracle_tl, symmetry_norm3, to_device)
from saturation_oracle import saturation_derivative


# ----------------------------------------------------------------------------------------------
# vertical grids
# ----------------------------------------------------------------------------------------------
def tropopause_window(eta, nz):
    """-> (klo, khi, nps, overlap): the levels k in [0, nz-2] with 0.1 < eta[k] < 0.4 as `build_level_table`
    (csrc/cloudsc2_common.hpp) finds them - klo = nz, khi = -1 when there is none - their number as `nl_ring_kernel` counts
    it, and whether that kernel overlaps the tropopause pre-scan with its sweep (csrc/cloudsc2_nl.hip, "Tropopause
    pre-scan": nps <= klo and eta <= 0.1 on every level above the window) or runs `trpaus_prescan` before it.
    The comparisons are made in the grid's own precision, as the kernels make them with T(0.1) and T(0.4)."""
    T = eta.dtype.type
    inside = [k for k in range(nz - 1) if eta[k] > T(0.1) and eta[k] < T(0.4)]
    klo, khi = (inside[0], inside[-1]) if inside else (nz, -1)
    nps = khi - klo + 1 if khi >= klo else 0
    overlap = 0 < nps <= klo and all(eta[k] <= T(0.1) for k in range(klo))
    return klo, khi, nps, overlap


def eta_family(nz, dtype):
    """name -> eta (nz + 1 entries in `dtype`, the padding slot 0).  `synthetic` is the one grid every other test runs on;
    the others put the tropopause window where that grid never has it.  A grid that needs more levels than `nz` is left
    out (`chunk_tail`: 20 levels)."""
    T = np.dtype(dtype).type
    k = np.arange(nz)

    def grid(levels):
        eta = np.zeros(nz + 1, dtype)
        eta[:nz] = np.asarray(levels, np.float64).astype(dtype)
        return eta

    def banded(klo, nwin, above=0.05):
        """`klo` levels of `above`, a window of `nwin` levels rising from 0.15 to 0.35, the rest from 0.5 to 0.99"""
        assert klo + nwin <= nz - 1
        return grid(np.concatenate([np.full(klo, above), np.linspace(0.15, 0.35, nwin), np.linspace(0.5, 0.99, nz - klo - nwin)]))

    fam = {"synthetic": eta_levels(nz, dtype=dtype),
           "uniform": grid((k + 0.5) / nz),
           "no_window_above": grid(np.minimum(np.linspace(0.002, 0.11, nz), 0.1)),     # ends on T(0.1) itself
           "no_window_below": grid(np.maximum(np.linspace(0.39, 1.0, nz), 0.4)),       # starts on T(0.4) itself
           "all_inside": grid(np.linspace(0.11, 0.39, nz)),
           "bottom_up": grid((nz - k - 0.5) / nz),
           "nps_eq_klo": banded(nz // 3, nz // 3),
           "nps_eq_klo_plus_1": banded(nz // 3, nz // 3 + 1)}
    # the levels next to the window are T(0.1) and T(0.4) themselves: the strict inequalities exclude them
    a, b = nz // 4, nz // 2
    edge = grid(np.concatenate([np.linspace(0.01, 0.09, a), np.linspace(0.15, 0.35, b - a), np.linspace(0.45, 0.99, nz - b)]))
    edge[a - 1], edge[b] = T(0.1), T(0.4)
    fam["edge_values"] = edge
    # a window of 17 levels = one beyond a multiple of both chunk lengths of `trpaus_prescan` (16, and 8 when perturbed);
    # two levels above it, so the pre-scan runs before the sweep
    if nz >= 20:
        fam["chunk_tail"] = banded(2, 17)
    # a value outside (0.1, 0.4) inside [klo, khi]: once on the path that scans before the sweep, once on the overlapped one
    nwin = min(10, nz - 3)
    hole = banded(1, nwin)
    hole[1 + nwin // 2] = T(0.45)
    fam["hole"] = hole
    hole = banded(nz // 2, nz // 4)
    hole[nz // 2 + nz // 8] = T(0.05)
    fam["hole_overlapped"] = hole
    return fam


#: the grids held at every level count; the whole family is held at nz = 40
CORE_GRIDS = ("uniform", "all_inside", "nps_eq_klo", "nps_eq_klo_plus_1")


# ----------------------------------------------------------------------------------------------
# inputs planted on the thresholds
# ----------------------------------------------------------------------------------------------
TIE_NX = 64


def tie_case(nz, dtype, saturation=None):
    """-> fields, eta, dt, {plant: column}.  `nl_case` with `tnd_cml_*` and `supsat` zeroed, so that the scheme's first-guess
    t, q, ql, qi ARE the inputs, bit for bit; one plant per column, the other columns are controls.  Every planted value is
    cast to the field type first.  `saturation(ap, t) -> qsat` replaces the oracle's `saturation` for `in_qsat` (the GPU
    tests pass the device's, so that the kernels that form qsat themselves meet the same q == qsat)."""
    ext = externals()
    T = np.dtype(dtype).type
    fields, eta, dt = nl_case(TIE_NX, nz, dtype=dtype)
    F = {k[3:]: v.copy() for k, v in fields.items()}
    for n in ("tnd_cml_t", "tnd_cml_q", "tnd_cml_ql", "tnd_cml_qi", "supsat"):
        F[n][:] = 0
    t, q = F["t"], F["q"]
    klo, khi, nps, _ = tropopause_window(eta, nz)
    assert nps > 1 and klo > 0
    RTT, RTICE = T(ext["RTT"]), T(ext["RTICE"])
    cols = {}

    def col(name):
        cols[name] = len(cols)
        return cols[name]

    def nearest(c, value, first=0):
        return first + int(np.argmin(np.abs(t[first:nz, c].astype(np.float64) - float(value))))

    # --- temperatures (before qsat is formed from them)
    c_rtt = col("t == RTT at an overcast level, no snow from above")
    k_rtt = nearest(c_rtt, RTT)
    t[k_rtt, c_rtt] = RTT
    c = col("t == RTICE")
    t[nearest(c, RTICE), c] = RTICE
    c_melt = col("t == RTT + 2, snow from above")
    k_melt = nearest(c_melt, ext["RTT"] + 2.0, first=1)
    t[k_melt, c_melt] = T(ext["RTT"] + 2.0)
    t[k_melt - 1, c_melt] = T(ext["RTT"] - 5.0)            # an overcast mixed-phase level: its precipitation freezes
    c_iso = col("isothermal tropopause window")
    t[klo:khi + 2, c_iso] = t[klo, c_iso]
    c = col("t[k] == t[k+1] at the level that decides trpaus")
    deciding = [k for k in range(klo, khi + 1) if t[k, c] > t[k + 1, c]]
    assert deciding, "the base column has no tropopause in the window"
    t[deciding[-1], c] = t[deciding[-1] + 1, c]             # `>` now finds an earlier level or none, `>=` would find this one
    c_above = col("q == qsat above the tropopause (crh2 == 1: qt == qcrit == qsat)")
    t[klo - 1, c_above] = T(255.0)                         # t >= RTICE: qsat is not scaled there
    c_below = col("q == qsat below the tropopause (qt == qsat > qcrit)")
    k_below = nz - 3
    c_twice = col("overcast on two consecutive levels")
    assert t[k_below, c_below] >= RTICE and (t[nz - 6:nz - 4, c_twice] >= RTICE).all()
    c_min = col("q == qsat below saturation, under an overcast level (min(q, qsat) in the evaporation block)")
    k_min = nearest(c_min, 248.0, first=1)
    assert t[k_min, c_min] < RTICE                          # qsat is scaled up there: qt == in_qsat is not overcast

    # --- qsat of the planted temperatures, then the moisture
    qsat = np.zeros_like(t)
    if saturation is None:
        oracle.saturation(F["ap"], t, qsat, ext)
    else:
        qsat[:nz] = saturation(F["ap"], t)[:nz]
    F["qsat"] = qsat
    for n in ("ql", "qi", "lude"):
        F[n][:k_rtt, c_rtt] = 0                            # nothing condenses or precipitates above the t == RTT level
    q[:k_rtt, c_rtt] = (T(0.1) * qsat[:k_rtt, c_rtt]).astype(dtype)
    # the window is as cold as its top now: keep the humidity it had below saturation, or its lower levels hold several
    # times qsat and the adjoints there are differences of huge terms that float32 cannot resolve
    q[klo:khi + 2, c_iso] = np.minimum(q[klo:khi + 2, c_iso], T(0.8) * qsat[klo:khi + 2, c_iso])
    q[k_rtt, c_rtt] = T(1.2) * qsat[k_rtt, c_rtt]          # condensate to split by phase, precipitation to freeze or not
    F["mfu"][k_rtt, c_rtt] = F["mfd"][k_rtt, c_rtt] = 0    # ... and no subsidence that evaporates it first
    q[k_melt - 1, c_melt] = T(1.2) * qsat[k_melt - 1, c_melt]
    for c, k in ((c_above, klo - 1), (c_below, k_below)):
        q[k, c] = qsat[k, c]
        F["ql"][k, c] = F["qi"][k, c] = 0
    q[nz - 6:nz - 4, c_twice] = T(1.2) * qsat[nz - 6:nz - 4, c_twice]
    q[k_min - 1, c_min] = T(2.0) * qsat[k_min - 1, c_min]  # overcast whatever the scaling: precipitation and covptot = 1 below
    q[k_min, c_min] = qsat[k_min, c_min]
    for n in ("ql", "qi", "lude"):
        F[n][k_min, c_min] = 0
    k = nz // 2
    for name, value in (("lu[k+1] == ZEPS2", T(ext["ZEPS2"])), ("lu[k+1] just below ZEPS2", np.nextafter(T(ext["ZEPS2"]), T(0)))):
        c = col(name)
        F["lude"][k, c] = T(2.0e-6)                        # dt * lude * g / dp is about 1e-5 there: well above RLMIN
        F["lu"][k + 1, c] = value
    c = col("no moisture, no convection")
    for n in ("q", "ql", "qi", "lu", "lude", "mfu", "mfd"):
        F[n][:, c] = 0
    c = col("mfu == -mfd")
    F["mfd"][:, c] = -F["mfu"][:, c]
    assert (F["mfu"][:nz, c] != 0).any() and len(cols) < TIE_NX - 8
    return {"in_" + n: v for n, v in F.items()}, eta, dt, cols


def device_saturation(gpu, dtype):
    """`saturation(ap, t) -> qsat` by the HIP kernel, for `tie_case`"""
    def saturation(ap, t):
        nz, nx = ap.shape[0] - 1, ap.shape[1]
        box = Box(nx, nz, dtype, gpu, False)
        out = box.nan()
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

        compile_stencil("saturation", externals())(in_ap=box.put(ap), in_t=box.put(t), out_qsat=out, origin=(0, 0, 0),
                                                   domain=(nx, 1, nz), validate_args=True, exec_info=None)
        return from_device(out)
    return saturation


# ----------------------------------------------------------------------------------------------
# cases: a state, a grid, directions - and what the oracle gives for them, computed once
# ----------------------------------------------------------------------------------------------
class Case:
    """one host state on one grid with `ndir` general directions.  `cut(nx)` is its first nx columns (columns are
    independent, so the oracle's results are cut the same way)."""

    def __init__(self, key, fields, eta, dt, dirs, flags=None):
        self.key, self.fields, self.eta, self.dt, self.dirs, self.flags = key, fields, eta, dt, dirs, dict(flags or {})
        self.nz, self.nx = fields["in_ap"].shape[0] - 1, fields["in_ap"].shape[1]
        self.dtype, self._own = fields["in_ap"].dtype, {}

    def ext(self, **flags):
        return externals(NLEV=self.nz, **dict(self.flags, **flags))

    def _cached(self, what, make):
        """once per (what, key) for the whole session; a case without a key keeps its results itself"""
        if self.key is not None:
            return _once((what, self.key), make)
        if what not in self._own:
            self._own[what] = make()
        return self._own[what]

    def nl(self):
        return self._cached("grid nl", lambda: run_oracle_nl(self.fields, self.eta, self.dt, self.ext()))

    def tl(self, d=0, qsat_from_saturation=False):
        """the oracle's perturbed outputs for direction d; `qsat_from_saturation`: the perturbation of qsat is saturation's
        derivative applied to those of t and ap (what the step kernels form)"""
        def make():
            u = dict(self.dirs[d])
            if qsat_from_saturation:
                _, g_t, g_ap, _ = self.saturation_derivative()
                u["qsat"] = (g_t * u["t"].astype(np.float64) + g_ap * u["ap"].astype(np.float64)).astype(self.dtype)
            return run_oracle_tl(self.fields, {"in_" + n + "_i": u[n] for n in NL_IN}, self.eta, self.dt, self.ext())[1]
        return self._cached(("grid tl", d, qsat_from_saturation), make)

    def saturation_derivative(self):
        return self._cached("grid dsat", lambda: saturation_derivative(self.fields["in_ap"], self.fields["in_t"], self.ext()))

    def ad(self, d=0, fix=1, traj=True, step=False, outputs=False):
        """the oracle's adjoints forced with `tl(d)`: on its own NL fluxes as trajectory, or carrying them (`traj` False);
        `step`: chained through saturation (the adjoint of qsat arrives in those of t and ap).  `outputs`: the NL outputs
        of the adjoint stencil's own forward sweep instead"""
        def make():
            ext = self.ext(AD_TRAJ_FIX=fix)
            out, adj = run_oracle_ad(self.fields, self.tl(d), self.eta, self.dt, ext, traj=self.nl() if traj else None)
            adj = dict(adj)
            if step:
                _, g_t, g_ap, _ = self.saturation_derivative()
                for n, g in (("t", g_t), ("ap", g_ap)):
                    adj[n] = (adj[n].astype(np.float64) + g * adj["qsat"].astype(np.float64)).astype(self.dtype)
            return out, adj
        return self._cached(("grid ad", d, fix, traj, step), make)[0 if outputs else 1]

    def trpaus(self, fields=None):
        """the oracle's tropopause eta per column (of `fields`, by default the state's own)"""
        f = self.fields if fields is None else fields
        t3d = f["in_t"][:self.nz] + self.dtype.type(self.dt) * f["in_tnd_cml_t"][:self.nz]
        return oracle._trpaus(self.eta, t3d, self.nz, self.dtype)


def grid_case(grid, nz, dtype, nx=66, ndir=3, **flags):
    """the shared host state of (nx, nz) on the grid `grid` of `eta_family`"""
    fields, _, dt = host_case(nx, nz, dtype)
    dt = flags.pop("dt", dt)
    key = ("grid", grid, nx, nz, np.dtype(dtype), dt, tuple(sorted(flags.items())))
    return Case(key, fields, eta_family(nz, dtype)[grid], dt, host_directions(nx, nz, dtype, ndir), flags)


def cut(arr, nx):
    return np.ascontiguousarray(arr[:, :nx])


# ----------------------------------------------------------------------------------------------
# holding a kernel's result to the oracle's
# ----------------------------------------------------------------------------------------------
class Held:
    """compares fields with the oracle's, remembers the worst |error| / bound, and fails at the end with every miss"""

    def __init__(self, tag, dtype, columns=None):
        self.tag, self.dtype, self.worst, self.where, self.failures = tag, np.dtype(dtype), 0.0, None, []
        self.by_column = None if columns is None else np.zeros(columns)       # worst |error| / bound per column

    def field(self, name, got, want, mul=1.0):
        tol = TOL[self.dtype]
        w = want.astype(np.float64)
        bound = mul * (tol["rtol"] * np.abs(w) + tol["atol_rel"] * float(np.max(np.abs(w))))
        err = np.abs(got.astype(np.float64) - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
        if ratio > self.worst:
            self.worst, self.where = ratio, name
        if self.by_column is not None and err.ndim == 2 and err.shape[1] == self.by_column.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                self.by_column = np.fmax(self.by_column, np.max(np.where(bound > 0, err / bound, 0.0), axis=0))
        try:
            assert_close(f"{self.tag} {name}", got, want, self.dtype, rtol_mul=mul)
        except AssertionError as exc:
            self.failures.append(str(exc))

    def fields(self, what, got, want, names, levels, nz, nx, mul=1.0, padding_nan=True, reversed_columns=False):
        """`got`: name -> device field (`reversed_columns`: its columns in reverse order); `want`: name -> host array of at
        least nx columns"""
        for n in names:
            k = levels(n, nz)
            a = from_device(got[n])[:, ::-1] if reversed_columns else from_device(got[n])
            self.field(f"{what} {n}", a[:k], cut(want[n], nx)[:k], mul)
            if padding_nan and not np.isnan(a[k:]).all():
                self.failures.append(f"{self.tag} {what} {n}: padding level written")

    def done(self):
        print(f"{self.tag} {self.dtype.name}: worst |error| / bound {self.worst:.3g} ({self.where})")
        assert not self.failures, "\n".join(self.failures)


class Shifted(Box):
    """a column window that starts at column 1 of wider allocations: no row is 16-byte aligned, so `cloudsc2_nl` takes its
    register-prefetch path at any nx (the launcher's conditions for the LDS ring: csrc/cloudsc2_nl.hip, `launch_nl`)"""

    def __init__(self, nx, nz, dtype, device):
        super().__init__(nx, nz, dtype, device, False)
        self.pitch, self.col0 = nx + 3, 1


def device_eta(gpu, eta):
    import torch

    return torch.as_tensor(eta, device=gpu)


def hold_nl(held, gpu, case, nx, path):
    """`cloudsc2_nl` (path "ring": aligned storages, "prefetch": a misaligned window) or `cloudsc2_nl_saturation` ("fused",
    "fused prefetch") on the first nx columns; the kernel that ran is asserted"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nz, dtype = case.nz, case.dtype
    fused, prefetch = path.startswith("fused"), path.endswith("prefetch")
    box = Shifted(nx, nz, dtype, gpu) if prefetch else Box(nx, nz, dtype, gpu, False)
    st = box.state({k: cut(v, nx) for k, v in case.fields.items()}, tuple(n for n in NL_IN if not (fused and n == "qsat")))
    outs = {n: box.nan() for n in NL_OUT}
    extra = {"out_qsat": box.nan()} if fused else {}
    box.stencil("cloudsc2_nl_saturation" if fused else "cloudsc2_nl", case.ext(), device_eta(gpu, case.eta), case.dt,
                **{"in_" + n: f for n, f in st.items()}, **{"out_" + n: f for n, f in outs.items()}, **extra)
    want = "cs2::nl_kernel" if prefetch else "cs2::nl_ring_kernel<ragged>" if nx % 64 else "cs2::nl_ring_kernel"
    assert _lib.last_kernel() == want, (path, nx, _lib.last_kernel())
    held.fields(f"nl[{path}, nx={nx}]", outs, case.nl(), NL_OUT, nlev_of, nz, nx)
    if fused:
        held.field(f"nl[{path}, nx={nx}] qsat", from_device(extra["out_qsat"])[:nz], cut(case.fields["in_qsat"], nx)[:nz])
    return outs


def hold_perturbed(held, gpu, case, inc, f2s):
    """`cloudsc2_nl_perturbed` at f2s[0] point by point; the all-step-sizes `cloudsc2_nl_taylor_multi` and, one launch per
    step size, `cloudsc2_nl_taylor` by their sums against the oracle's separate perturbed_state + cloudsc2_nl calls,
    bounded as tests/test_hip_fused_oracle.py bounds them.  `inc`: in_*_i increments of the case's fields"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil, taylor_blocks
    from test_hip_fused_oracle import _oracle_perturbed, _oracle_taylor_sums

    nx, nz, dtype, ext = case.nx, case.nz, case.dtype, case.ext()
    want = _oracle_perturbed(case.fields, inc, f2s[0], case.eta, case.dt, ext)
    box = Box(nx, nz, dtype, gpu, False)
    dev, dev_i = to_device(case.fields, gpu), to_device(inc, gpu)
    com = dict(in_eta=device_eta(gpu, case.eta), dt=case.dt, origin=(0, 0, 0), domain=(nx, 1, nz + 1), validate_args=True,
               exec_info=None)
    outs = {n: box.nan() for n in NL_OUT}
    compile_stencil("cloudsc2_nl_perturbed", ext)(**dev, **dev_i, **{"out_" + n: f for n, f in outs.items()}, f=f2s[0], **com)
    assert _lib.last_kernel() == "cs2::nl_kernel"
    held.fields("nl_perturbed", outs, want, NL_OUT, nlev_of, nz, nx)
    ref = {n: box.nan() for n in NL_OUT}
    compile_stencil("cloudsc2_nl", ext)(**dev, **{"out_" + n: f for n, f in ref.items()}, **com)
    for f in ref.values():
        f.nan_to_num_(nan=0.0)                     # the padding level of the reference outputs is read, and is zero
    refs = {"ref_" + n: f for n, f in ref.items()}
    part = torch.full((taylor_blocks(nx), len(f2s), len(NL_OUT)), float("nan"), dtype=torch.float64, device=gpu)
    compile_stencil("cloudsc2_nl_taylor_multi", ext)(**dev, **dev_i, **refs, out_partials=part, fs=f2s, **com)
    assert _lib.last_kernel() == "cs2::nl_taylor_multi_kernel"
    single = torch.full((len(f2s), taylor_blocks(nx), len(NL_OUT)), float("nan"), dtype=torch.float64, device=gpu)
    one = compile_stencil("cloudsc2_nl_taylor", ext)
    for j, f2 in enumerate(f2s):
        one(**dev, **dev_i, **refs, out_partials=single[j], f=f2, **com)
    torch.cuda.synchronize()
    got, got1 = part.sum(dim=0).cpu().numpy(), single.sum(dim=1).cpu().numpy()
    base, sums, _ = _oracle_taylor_sums(case.fields, inc, f2s, case.eta, case.dt, ext)
    tol = TOL[np.dtype(dtype)]
    for fi, n in enumerate(NL_OUT):
        bound = 2.0 * (tol["rtol"] + tol["atol_rel"]) * float(np.abs(base[n]).sum(dtype=np.float64)) + 1e-300
        assert np.all(np.abs(got[:, fi] - sums[:, fi]) <= bound), (n, got[:, fi], sums[:, fi], bound)
        assert np.all(np.abs(got1[:, fi] - sums[:, fi]) <= bound), (n, got1[:, fi], sums[:, fi], bound)


def _put_dir(box, u, names, nx):
    return {n: box.put(cut(u[n], nx)) for n in names}


def hold_dense(held, gpu, case, nx, fix=1):
    """the stencils `cloudsc2_tl` (its LDS ring at nx % 64 == 0, else its register path) and `cloudsc2_ad` (fluxes carried)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nz, dtype = case.nz, case.dtype
    box = Box(nx, nz, dtype, gpu, False)
    ext, eta = case.ext(AD_TRAJ_FIX=fix), device_eta(gpu, case.eta)
    st = box.state({k: cut(v, nx) for k, v in case.fields.items()})
    out, out_i = box.dense_tl(st, _put_dir(box, case.dirs[0], NL_IN, nx), ext, eta, case.dt)
    assert _lib.last_kernel() == ("cs2::tl_kernel" if nx % 64 else "cs2::tl_ring_kernel"), _lib.last_kernel()
    held.fields(f"tl[nx={nx}] out", out, case.nl(), NL_OUT, nlev_of, nz, nx)
    held.fields(f"tl[nx={nx}] out_i", out_i, case.tl(0), NL_OUT, nlev_of, nz, nx, 100.0)
    forcing = {n: box.put(cut(case.tl(0)[n], nx)) for n in NL_OUT}
    nl, adj = {n: box.nan() for n in NL_OUT}, {n: box.nan() for n in NL_IN}
    box.stencil("cloudsc2_ad", ext, eta, case.dt, **{"in_" + n: f for n, f in st.items()},
                **{"in_" + n + "_i": f for n, f in forcing.items()}, **{"out_" + n: f for n, f in nl.items()},
                **{"out_" + n + "_i": f for n, f in adj.items()})
    assert _lib.last_kernel() == "cs2::ad_kernel", _lib.last_kernel()
    # the adjoint stencil's forward sweep is not NL's: it takes qt <= qcrit for clear (adjoint/_stencils/cloudsc2.py:235)
    held.fields(f"ad[nx={nx}, FIX={fix}] out", nl, case.ad(0, fix, traj=False, outputs=True), NL_OUT, nlev_of, nz, nx)
    held.fields(f"ad[nx={nx}, FIX={fix}]", adj, case.ad(0, fix, traj=False), NL_IN, adjoint_nlev_of, nz, nx, 100.0)


def hold_masked(held, gpu, case, nx, step, fix=1):
    """`tl_masked` / `ad_masked` or, `step`, `tl_step` / `ad_step`, every field present and wanted"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    nz, dtype = case.nz, case.dtype
    names = STEP_IN if step else NL_IN
    box = Box(nx, nz, dtype, gpu, False)
    ext, eta = case.ext(AD_TRAJ_FIX=fix), device_eta(gpu, case.eta)
    st = box.state({k: cut(v, nx) for k, v in case.fields.items()}, names)
    tl, ad = (autodiff.tl_step, autodiff.ad_step) if step else (autodiff.tl_masked, autodiff.ad_masked)
    what = "step" if step else "masked"
    nl, out_i = tl(st, _put_dir(box, case.dirs[0], names, nx), eta, case.dt, ext, want=NL_OUT, write_nl=True)
    assert _lib.last_kernel() == f"cs2::tl_{what}_kernel", _lib.last_kernel()
    held.fields(f"tl_{what} out", nl, case.nl(), NL_OUT, nlev_of, nz, nx, padding_nan=False)
    held.fields(f"tl_{what} out_i", out_i, case.tl(0, step), NL_OUT, nlev_of, nz, nx, 100.0, padding_nan=False)
    if ext["LEVAPLS2"] or ext["LDRAIN1D"]:
        return nl, out_i, None                                  # the trajectory adjoints refuse the evaporation block
    forcing = {n: box.put(cut(case.tl(0)[n], nx)) for n in NL_OUT}
    adj = ad(st, forcing, eta, case.dt, ext, traj={"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}, want=names)
    assert _lib.last_kernel() == f"cs2::ad_{what}_kernel", _lib.last_kernel()
    held.fields(f"ad_{what}[FIX={fix}]", adj, case.ad(0, fix, step=step), names, adjoint_nlev_of, nz, nx, 100.0, padding_nan=False)
    return nl, out_i, adj


def hold_multi(held, gpu, case, nx, ndir=3):
    """`tl_multi` / `ad_multi` at `ndir` directions in one launch each (AD_TRAJ_FIX = 1)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    nz, dtype = case.nz, case.dtype
    box = Box(nx, nz, dtype, gpu, False)
    ext, eta = case.ext(AD_TRAJ_FIX=1), device_eta(gpu, case.eta)
    st = box.state({k: cut(v, nx) for k, v in case.fields.items()})
    pert = {n: box.batch([cut(u[n], nx) for u in case.dirs[:ndir]]) for n in NL_IN}
    nl, out_i = autodiff.tl_multi(st, pert, eta, case.dt, ext, want=NL_OUT, write_nl=True, width=_lib.TL_MAX_DIRS)
    assert _lib.last_kernel() == "cs2::tl_dirs_kernel", _lib.last_kernel()
    forcing = {n: box.batch([cut(case.tl(d)[n], nx) for d in range(ndir)]) for n in NL_OUT}
    adj = autodiff.ad_multi(st, forcing, eta, case.dt, ext, traj={"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}, want=NL_IN,
                            width=_lib.AD_MAX_DIRS)
    assert _lib.last_kernel() == "cs2::ad_dirs_kernel", _lib.last_kernel()
    held.fields("tl_multi out", nl, case.nl(), NL_OUT, nlev_of, nz, nx, padding_nan=False)
    for d in range(ndir):
        held.fields(f"tl_multi out_i[{d}]", {n: f[d] for n, f in out_i.items()}, case.tl(d), NL_OUT, nlev_of, nz, nx, 100.0,
                    padding_nan=False)
        held.fields(f"ad_multi[{d}]", {n: f[d] for n, f in adj.items()}, case.ad(d, 1), NL_IN, adjoint_nlev_of, nz, nx, 100.0,
                    padding_nan=False)


def hold_ensemble(held, gpu, case, nx):
    """`cloudsc2_{nl,tl,ad}_ens` on two members: the first nx columns, and the same columns in reverse order (another
    state per member at the cost of one oracle run); AD_TRAJ_FIX = 1, the trajectory fluxes are the TL launch's own"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nz, dtype = case.nz, case.dtype
    box = Box(nx, nz, dtype, gpu, False)
    ens = Ens(box, 2, 0)
    ext, eta = case.ext(AD_TRAJ_FIX=1), device_eta(gpu, case.eta)
    both = lambda a: [cut(a, nx), np.ascontiguousarray(cut(a, nx)[:, ::-1])]  # noqa: E731
    state = {n: ens.put(both(case.fields["in_" + n])) for n in NL_IN}
    out = {n: ens.nan() for n in NL_OUT}
    ens_nl(ens, ext, state, eta, case.dt, out)
    assert _lib.last_kernel() == "cs2::nl_ens_kernel", _lib.last_kernel()
    pert = {n: ens.put(both(case.dirs[0][n])) for n in NL_IN}
    tl_out, out_i = {n: ens.nan() for n in NL_OUT}, {n: ens.nan() for n in NL_OUT}
    ens_tl("tl_ens", ens, ext, state, pert, eta, case.dt, tl_out, out_i)
    assert _lib.last_kernel() == "cs2::tl_ens_kernel", _lib.last_kernel()
    forcing = {n: ens.put(both(case.tl(0)[n])) for n in NL_OUT}
    adj = {n: ens.nan() for n in NL_IN}
    ens_ad("ad_ens", ens, ext, state, forcing, eta, case.dt, {n: tl_out[n] for n in ("fplsl", "fplsn")}, adj)
    assert _lib.last_kernel() == "cs2::ad_ens_kernel", _lib.last_kernel()
    for m in range(2):                                         # the second member's columns are in reverse order
        held.fields(f"nl_ens[{m}]", {n: f[m] for n, f in out.items()}, case.nl(), NL_OUT, nlev_of, nz, nx, reversed_columns=m == 1)
        held.fields(f"tl_ens[{m}] out_i", {n: f[m] for n, f in out_i.items()}, case.tl(0), NL_OUT, nlev_of, nz, nx, 100.0,
                    reversed_columns=m == 1)
        held.fields(f"ad_ens[{m}]", {n: f[m] for n, f in adj.items()}, case.ad(0, 1), NL_IN, adjoint_nlev_of, nz, nx, 100.0,
                    reversed_columns=m == 1)


def transpose_identity(gpu, case, nx):
    """per column |<J u, J u> - <u, J^T J u>| / (eps <u, J^T J u>) by `tl_masked` / `ad_masked` with AD_TRAJ_FIX = 1 and
    `supsat` unperturbed (its adjoint is the reference's literal dt x the q adjoint, not the transpose)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    nz, dtype = case.nz, case.dtype
    names = tuple(n for n in NL_IN if n != "supsat")
    box = Box(nx, nz, dtype, gpu, False)
    ext, eta = case.ext(AD_TRAJ_FIX=1), device_eta(gpu, case.eta)
    st = box.state({k: cut(v, nx) for k, v in case.fields.items()})
    nl, w = autodiff.tl_masked(st, _put_dir(box, case.dirs[0], names, nx), eta, case.dt, ext, want=NL_OUT, write_nl=True)
    adj = autodiff.ad_masked(st, w, eta, case.dt, ext, traj={"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}, want=names)
    tl_i = {n: from_device(w[n])[:nlev_of(n, nz)] for n in NL_OUT}
    zero = np.zeros((nz + 1, nx), dtype)
    u = {"in_" + n + "_i": (cut(case.dirs[0][n], nx) if n in names else zero)[:adjoint_nlev_of(n, nz)] for n in NL_IN}
    a = {n: (from_device(adj[n]) if n in names else zero)[:adjoint_nlev_of(n, nz)] for n in NL_IN}
    return symmetry_norm3(tl_i, u, a, dtype)
