"""What the bitwise metamorphic tests share (tests/test_metamorphic_linearity.py, tests/test_metamorphic_locality.py): host
cases, the transformations of a case, one runner per C entry on NaN-prefilled buffers, and the bitwise comparison.

A `Case` is host data only: per member a state, trajectory fluxes (the oracle's NL outputs), `NDIR` perturbations (1 %, 2 %,
... increments of other seeded states) and `NDIR` forcings (the oracle's TL outputs for those perturbations).  Every
per-column input of every entry is taken from it, so a transformation of the case (scaling, replacing columns, members or
directions, permuting columns or members) is a transformation of plain arrays, and nothing is recomputed from transformed data.
Single entries run member 0, direction 0; ensembles every member on its direction 0; multi-direction entries every direction of
member 0; members times directions everything.

A runner returns `{(group, member, direction, name): (host array [level][column], number of written levels)}` with the groups
`nl` (what does not depend on perturbations or forcings: NL outputs, `cover`, `qsat`) and `out` (perturbed outputs, adjoints).

`torch` and the package are imported inside functions, so that collecting a test module needs neither."""
import ctypes
from typing import Callable, NamedTuple

import numpy as np

import test_evap_adjoint as evap_single
import test_hip_ad_multi_ens as mdirs
import test_hip_ens_shared as shared_state
import test_hip_evap_ensemble as evap_ens
from derivative_support import SEED, STEP_IN, Box, Ens, ens_ad, ens_nl, ens_tl, raw_ad, raw_tl
from grid_support import eta_family, tropopause_window
from helpers import (NL_IN, NL_OUT, adjoint_nlev_of, externals, from_device, increments, nl_case, nlev_of, run_oracle_nl,
                     run_oracle_tl)

NZ, NMEM, NDIR = 12, 3, 5
#: two full waves plus two lanes of a third; a second workgroup with a ragged end
NXS = (130, 321)
SCALES = (8.0, 0.125, -1.0, -1024.0)
FLUXES = ("fplsl", "fplsn")
INC = ("aph", "ap", "q", "qsat", "t", "ql", "qi", "lude", "lu", "mfu", "mfd", "tnd_cml_t", "tnd_cml_q", "tnd_cml_ql",
       "tnd_cml_qi", "supsat")
#: the state fields the members of a shared-state call read from ONE field (the `da` mask of tests/test_hip_ens_shared.py)
SHARED = shared_state.MASKS["da"]
BASE, NOREG, FIX, L2, D1 = {}, dict(LREGCL=False), dict(AD_TRAJ_FIX=1), dict(LEVAPLS2=True), dict(LDRAIN1D=True)


# ----------------------------------------------------------------------------------------------
# host cases and their transformations
# ----------------------------------------------------------------------------------------------
class Case:
    """`data[(kind, member, direction, name)]` -> [level][column]; kinds `state`, `traj` (direction 0), `tl` (perturbations,
    `NL_IN` names), `ad` (forcings, `NL_OUT` names).  `f`: the factor of `cloudsc2_tl_incremented`.  `shared_member`: the
    member whose fields the shared-state entries read as the shared ones."""

    def __init__(self, nx, dtype, ext, eta, dt, data, f=0.01, shared_member=0):
        self.nx, self.dtype, self.ext, self.eta, self.dt, self.data = nx, np.dtype(dtype), ext, eta, dt, data
        self.f, self.shared_member = f, shared_member

    def get(self, kind, m, d, names):
        return {n: self.data[(kind, m, d, n)] for n in names}

    def mapped(self, fn, **over):
        """a case with `fn(key, array)` in place of every array"""
        new = Case(self.nx, self.dtype, self.ext, self.eta, self.dt, {k: fn(k, a) for k, a in self.data.items()}, self.f,
                   self.shared_member)
        new.__dict__.update(over)
        return new


_cases = {}


def host_case(nx, dtype, flags=BASE, seed=0):
    """the case of `nx` columns under the externals `flags`, built once and never modified.  Grid: `uniform` of
    tests/grid_support.py (a non-empty tropopause window at nz = 12); dt: that of `nl_case`, and with an evaporation switch the
    60 s at which tests/test_evap_adjoint.py finds the evaporation block running."""
    key = (nx, np.dtype(dtype), tuple(sorted(flags.items())), seed)
    if key in _cases:
        return _cases[key]
    ext = externals(NLEV=NZ, **flags)
    eta = eta_family(NZ, dtype)["uniform"]
    assert tropopause_window(eta, NZ)[2] > 0
    data, dt = {}, None
    for m in range(NMEM):
        fields, _, dt = nl_case(nx, NZ, dtype=dtype, seed=SEED + 300 + seed + m)
        if is_evap(flags):
            dt = evap_single.DT
        for n in NL_IN:
            data[("state", m, 0, n)] = fields["in_" + n]
        nl = run_oracle_nl(fields, eta, dt, ext)
        for n in FLUXES:
            data[("traj", m, 0, n)] = nl[n]
        for d in range(NDIR):
            other = nl_case(nx, NZ, dtype=dtype, seed=SEED + 400 + seed + 10 * m + d)[0]
            inc = increments(other, 0.01 * (d + 1))
            for n in NL_IN:
                data[("tl", m, d, n)] = inc["in_" + n + "_i"]
            out_i = run_oracle_tl(fields, inc, eta, dt, ext)[1]
            for n in NL_OUT:
                data[("ad", m, d, n)] = out_i[n]
    for a in data.values():
        assert a.dtype == np.dtype(dtype) and a.shape == (NZ + 1, nx) and np.isfinite(a).all()
        a.setflags(write=False)
    _cases[key] = Case(nx, dtype, ext, eta, dt, data)
    return _cases[key]


def is_evap(flags):
    return bool(flags.get("LEVAPLS2") or flags.get("LDRAIN1D"))


def scaled(case, s, where=lambda m, d: True):
    """perturbations and forcings of the members / directions `where(m, d)` keeps, times `s` (a power of two: exact)"""
    T = case.dtype.type
    assert np.log2(abs(s)) % 1 == 0
    return case.mapped(lambda k, a: a * T(s) if k[0] in ("tl", "ad") and where(k[1], k[2]) else a,
                       f=case.f * s if where(0, 0) else case.f)


def zeroed(case, keep=()):
    """all-zero perturbations and forcings, except the names of `keep`"""
    return case.mapped(lambda k, a: np.zeros_like(a) if k[0] in ("tl", "ad") and k[3] not in keep else a, f=0.0)


def copies_of(case, factors, members=False):
    """directions (or with `members`: members, state included) i = `factors[i]` times direction (member) 0"""
    T = case.dtype.type

    def fn(k, a):
        kind, m, d, n = k
        i = m if members else d
        if i >= len(factors):
            return a
        src = case.data[(kind, 0, d, n) if members else (kind, m, 0, n)]
        return src * T(factors[i]) if kind in ("tl", "ad") else (src if members else a)
    return case.mapped(fn)


def replaced(case, other=None, cols=None, member=None, direction=None):
    """the columns `cols`, all of member `member` or direction `direction` of all perturbations and forcings replaced by
    those of `other`, or by NaN"""
    def fn(k, a):
        kind, m, d, n = k
        if member is not None and m != member:
            return a
        if direction is not None and (d != direction or kind not in ("tl", "ad")):
            return a
        new = a.copy()
        sel = slice(None) if cols is None else cols
        new[:, sel] = np.nan if other is None else other.data[k][:, sel]
        return new
    return case.mapped(fn)


def permuted(case, perm=None, members=None):
    """column c of the new case is column `perm[c]`, member m is member `members[m]` of the old"""
    def fn(k, a):
        kind, m, d, n = k
        src = case.data[(kind, m if members is None else members[m], d, n)]
        return src if perm is None else src[:, perm]
    over = {} if members is None else dict(shared_member=list(members).index(case.shared_member))
    return case.mapped(fn, **over)


def third_of_columns(nx):
    """a fixed third of the columns: every wave and every workgroup keeps lanes and loses lanes"""
    return np.flatnonzero(np.arange(nx) % 3 == 1)


def column_permutation(nx):
    """a fixed permutation that moves every column of `nx` to another lane, and most to another wave and workgroup"""
    rng = np.random.default_rng(nx)
    perm = rng.permutation(nx)
    while (perm == np.arange(nx)).any():
        perm = rng.permutation(nx)
    return perm


# ----------------------------------------------------------------------------------------------
# the bitwise comparison
# ----------------------------------------------------------------------------------------------
def assert_bitwise(what, got, want, cols=None, rescaled=None):
    """Every key of `want` in `got`, on the written levels (and the columns `cols`): `np.array_equal` (so +0 equals -0), no
    NaN in a written level, the padding level still NaN.  Results are `{key: (array, written levels)}`.
    `rescaled = (base, s)`: `want` is `s` times the results `base` of the unscaled run; a differing point is left out where
    one of the two results is subnormal or zero while the other, rescaled, is subnormal - at most 0.1 % of a field's points,
    and the number is printed."""
    failures, left_out = [], 0
    for key, (b_all, k) in want.items():
        a_all, ka = got[key]
        tag = f"{what} {key[0]} {key[3]}[member {key[1]}, direction {key[2]}]"
        if ka != k or a_all.shape != b_all.shape:
            failures.append(f"{tag}: {ka} levels of shape {a_all.shape}, expected {k} of {b_all.shape}")
            continue
        sel = slice(None) if cols is None else cols
        a, b = a_all[:k, sel], b_all[:k, sel]
        if np.isnan(a).any():
            failures.append(f"{tag}: {int(np.isnan(a).sum())} NaN in the written levels")
            continue
        if not np.isnan(a_all[k:]).all():
            failures.append(f"{tag}: the padding level was written")
            continue
        bad = a != b
        if bad.any() and rescaled is not None:
            base, s = rescaled
            s = s(key) if callable(s) else s
            tiny = np.finfo(a.dtype).tiny
            o = np.abs(base[key][0][:k, sel].astype(np.float64))
            a64, b64 = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
            excused = bad & (((a64 < tiny) & (b64 < tiny) & (b64 > 0)) | ((o < tiny) & (a64 / abs(s) < tiny) & (a64 > 0)))
            if excused.sum() <= 1e-3 * a.size:
                left_out += int(excused.sum())
                bad &= ~excused
        if bad.any():
            err = np.where(bad, np.abs(a.astype(np.float64) - b.astype(np.float64)), -1.0)
            i = np.unravel_index(np.argmax(err), err.shape)
            failures.append(f"{tag}: {int(bad.sum())}/{bad.size} points differ; worst at level {i[0]}, column "
                            f"{i[1] if cols is None else np.arange(a_all.shape[1])[sel][i[1]]}: got {float(a[i]).hex()}, "
                            f"want {float(b[i]).hex()}")
    if left_out:
        print(f"{what}: {left_out} subnormal points left out")
    assert not failures, f"{len(failures)} fields differ:\n" + "\n".join(failures[:12])


def times(res, s, groups=("out",)):
    """runner results with the arrays of `groups` times `s`"""
    return {k: ((a * a.dtype.type(s), n) if k[0] in groups else (a, n)) for k, (a, n) in res.items()}


def only(res, keep):
    """the entries of a runner's results whose key `keep(group, m, d, name)` keeps"""
    return {k: v for k, v in res.items() if keep(*k)}


# ----------------------------------------------------------------------------------------------
# the device side of one case
# ----------------------------------------------------------------------------------------------
class Dev:
    """one case on the device: fields of one geometry (`Box`; `window`: column windows of wider allocations; `misaligned`:
    windows that start at column 1, whose rows are not 16-byte aligned), member-major batches with a gap between members"""

    def __init__(self, gpu, case, window=False, misaligned=False):
        import torch

        self.c, self.gpu, self.torch = case, gpu, torch
        self.box = Box(case.nx, NZ, case.dtype, gpu, window or misaligned)
        if misaligned:
            self.box.col0 = 1
        self.ens = Ens(self.box, NMEM, 64)
        self.eta = torch.as_tensor(case.eta, device=gpu)

    def nans(self, names, slots=None):
        return {n: self.box.nan(slots) for n in names}

    def ens_nans(self, names):
        return {n: self.ens.nan() for n in names}

    def _present(self, kind, names, absent):
        """with `absent`: the names of which some member / direction is not all zero"""
        if not absent:
            return names
        return tuple(n for n in names if any(a.any() for k, a in self.c.data.items() if k[0] == kind and k[3] == n))

    def put(self, kind, names, m=0, d=0, absent=False):
        return {n: self.box.put(self.c.data[(kind, m, d, n)]) for n in self._present(kind, names, absent)}

    def dirs(self, kind, names, m=0, absent=False):
        return {n: self.box.batch([self.c.data[(kind, m, d, n)] for d in range(NDIR)]) for n in self._present(kind, names, absent)}

    def members(self, kind, names, d=0, absent=False):
        return {n: self.ens.put([self.c.data[(kind, m, d, n)] for m in range(NMEM)]) for n in self._present(kind, names, absent)}

    def shared_members(self, names):
        """the state of a shared-state call: member-major batches, and for the shared fields member 0 of a NaN-filled batch"""
        state = self.members("state", [n for n in names if n not in SHARED])
        for n in names:
            if n in SHARED:
                state[n] = self.ens.nan()
                self.box.storage.klayout(state[n][0]).copy_(self.torch.as_tensor(self.c.data[("state", self.c.shared_member, 0, n)]))
        return state

    def stencil(self, name, nlev, **kw):
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

        compile_stencil(name, self.c.ext)(**kw, origin=(0, 0, 0), domain=(self.c.nx, 1, nlev), validate_args=True, exec_info=None)


def _res(group, fields, levels, m=0, d=0):
    return {(group, m, d, n): (from_device(f), levels(n, NZ)) for n, f in fields.items()}


def _res_members(group, fields, levels, d=0):
    return {(group, m, d, n): (from_device(f[m]), levels(n, NZ)) for n, f in fields.items() for m in range(NMEM)}


def _res_dirs(group, fields, levels, m=0):
    return {(group, m, d, n): (from_device(f[d]), levels(n, NZ)) for n, f in fields.items() for d in range(NDIR)}


def _nz(name, nz):
    return nz


def _all(name, nz):
    return nz + 1


def _pre(prefix, fields, suffix=""):
    return {prefix + n + suffix: f for n, f in fields.items()}


class _SharedCall:
    """what `enss_nl` / `enss_tl` / `enss_ad` of tests/test_hip_ens_shared.py read off their case"""
    mask_bits = shared_state.Shared.mask_bits

    def __init__(self, dev):
        self.box, self.ens, self.nmem, self.ext, self.dt, self.eta, self.shared = (dev.box, dev.ens, NMEM, dev.c.ext, dev.c.dt,
                                                                                  dev.eta, SHARED)


# ----------------------------------------------------------------------------------------------
# one runner per C entry
# ----------------------------------------------------------------------------------------------
def _dense_tl(inc):
    def run(dev, absent=False):
        c, out, out_i = dev.c, dev.nans(NL_OUT), dev.nans(NL_OUT)
        pert = dict(f=c.f) if inc else _pre("in_", dev.put("tl", NL_IN), "_i")
        dev.box.stencil("cloudsc2_tl_incremented" if inc else "cloudsc2_tl", c.ext, dev.eta, c.dt, **pert,
                        **_pre("in_", dev.put("state", NL_IN)), **_pre("out_", out), **_pre("out_", out_i, "_i"))
        return {**_res("nl", out, nlev_of), **_res("out", out_i, nlev_of)}
    return run


def _dense_ad(traj):
    def run(dev, absent=False):
        c, state, forcing = dev.c, dev.put("state", NL_IN), dev.put("ad", NL_OUT)
        if traj:
            return _res("out", dev.box.dense_ad_traj(state, forcing, dev.put("traj", FLUXES), c.ext, dev.eta, c.dt), adjoint_nlev_of)
        out, adj = dev.nans(NL_OUT), dev.nans(NL_IN)
        dev.box.stencil("cloudsc2_ad", c.ext, dev.eta, c.dt, **_pre("in_", state), **_pre("in_", forcing, "_i"),
                        **_pre("out_", out), **_pre("out_", adj, "_i"))
        return {**_res("nl", out, nlev_of), **_res("out", adj, adjoint_nlev_of)}
    return run


def _tl(entry, names, multi=False):
    def run(dev, absent=False):
        c, out = dev.c, dev.nans(NL_OUT)
        pert = (dev.dirs if multi else dev.put)("tl", names, absent=absent)
        out_i = dev.nans(NL_OUT, NDIR if multi else None)
        raw_tl(entry, dev.box, c.ext, dev.put("state", names), pert, dev.eta, c.dt, out, out_i, NDIR if multi else None)
        return {**_res("nl", out, nlev_of), **(_res_dirs if multi else _res)("out", out_i, nlev_of)}
    return run


def _ad(entry, names, multi=False, evap=False):
    def run(dev, absent=False):
        c, box = dev.c, dev.box
        state, traj = dev.put("state", names), dev.put("traj", FLUXES)
        forcing = (dev.dirs if multi else dev.put)("ad", NL_OUT, absent=absent)
        adj = dev.nans(names, NDIR if multi else None)
        res = {}
        if evap:
            assert c.dt == evap_single.DT
            cover = box.nan()
            evap_single.raw_evap(entry, box, c.ext, state, forcing, dev.eta, traj, adj, cover, 0, NDIR if multi else None)
            res = _res("nl", {"cover": cover}, _nz)
        else:
            raw_ad(entry, box, c.ext, state, forcing, dev.eta, c.dt, traj, adj, NDIR if multi else None)
        return {**res, **(_res_dirs if multi else _res)("out", adj, adjoint_nlev_of)}
    return run


def _tl_ens(entry, names, shared=False):
    def run(dev, absent=False):
        c, out, out_i = dev.c, dev.ens_nans(NL_OUT), dev.ens_nans(NL_OUT)
        pert = dev.members("tl", names, absent=absent)
        if shared:
            shared_state.enss_tl(entry, _SharedCall(dev), dev.shared_members(names), pert, out, out_i)
        else:
            ens_tl(entry, dev.ens, c.ext, dev.members("state", names), pert, dev.eta, c.dt, out, out_i)
        return {**_res_members("nl", out, nlev_of), **_res_members("out", out_i, nlev_of)}
    return run


def _ad_ens(entry, names, shared=False, evap=False):
    def run(dev, absent=False):
        c, adj, traj = dev.c, dev.ens_nans(names), dev.members("traj", FLUXES)
        forcing = dev.members("ad", NL_OUT, absent=absent)
        res = {}
        if shared:
            shared_state.enss_ad(entry, _SharedCall(dev), dev.shared_members(names), forcing, traj, adj)
        elif evap:
            assert c.dt == evap_ens.DT
            cover = dev.ens.nan()
            evap_ens.raw_evap_ens(entry, dev.ens, c.ext, dev.members("state", names), forcing, dev.eta, traj, adj, cover, 0)
            res = _res_members("nl", {"cover": cover}, _nz)
        else:
            ens_ad(entry, dev.ens, c.ext, dev.members("state", names), forcing, dev.eta, c.dt, traj, adj)
        assert dev.ens.gaps_untouched(), f"{entry}: the gap between members was written"
        return {**res, **_res_members("out", adj, adjoint_nlev_of)}
    return run


def _ad_mdirs(family, names):
    def run(dev, absent=False):
        c, box = dev.c, dev.box
        md = mdirs.MD(box, NMEM, NDIR, 64, 32)
        forcing = {n: md.put([[c.data[("ad", m, d, n)] for d in range(NDIR)] for m in range(NMEM)])
                   for n in dev._present("ad", NL_OUT, absent)}
        adj = {n: md.nan() for n in names}
        mdirs._raw(family, box, dev.ens, md, c.ext, dev.members("state", names), forcing, dev.eta, c.dt,
                   dev.members("traj", FLUXES), adj)
        assert md.outside_untouched(), f"{family}: something outside the fields was written"
        return {("out", m, d, n): (from_device(f[m, d]), adjoint_nlev_of(n, NZ)) for n, f in adj.items()
                for m in range(NMEM) for d in range(NDIR)}
    return run


def _saturation_call(dev, which, *args):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    box = dev.box
    p = autodiff._params(dev.c.ext, NZ)
    ptr = lambda f: None if f is None else f.data_ptr()  # noqa: E731
    rc = getattr(_lib.load(), f"cloudsc2_saturation_{which}_{box.sfx}")(
        ctypes.byref(p), box.nx, NZ, box.pitch, *[ptr(a) if hasattr(a, "data_ptr") or a is None else a for a in args],
        int(dev.torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "saturation_" + which)


def _saturation_tl(dev, absent=False):
    st, pert = dev.put("state", ("ap", "t")), dev.put("tl", ("ap", "t"), absent=absent)
    qsat, qsat_i = dev.box.nan(), dev.box.nan()
    _saturation_call(dev, "tl", st["ap"], st["t"], pert.get("ap"), pert.get("t"), qsat, qsat_i)
    return {**_res("nl", {"qsat": qsat}, _nz), **_res("out", {"qsat": qsat_i}, _nz)}


def _saturation_ad(accumulate):
    def run(dev, absent=False):
        st, adj = dev.put("state", ("ap", "t")), dev.put("ad", ("tnd_t",))["tnd_t"]
        if accumulate:      # what the products are added to: two more forcing fields, which scale with the forcing
            into = {"ap": dev.put("ad", ("tnd_q",))["tnd_q"], "t": dev.put("ad", ("clc",))["clc"]}
            for f in into.values():
                dev.box.storage.klayout(f)[NZ:] = float("nan")
        else:
            into = dev.nans(("ap", "t"))
        _saturation_call(dev, "ad", st["ap"], st["t"], adj, into["ap"], into["t"], int(accumulate))
        return _res("out", into, _nz)
    return run


def _nl(fused=False, perturbed=False, misaligned=False):
    def run(dev, absent=False):
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

        c, out = dev.c, dev.nans(NL_OUT)
        kw = _pre("in_", dev.put("state", STEP_IN if fused else NL_IN))
        if fused:
            kw["out_qsat"] = dev.box.nan()
        if perturbed:
            kw.update(_pre("in_", dev.put("tl", NL_IN), "_i"), f=0.5)
        name = "cloudsc2_nl_saturation" if fused else "cloudsc2_nl_perturbed" if perturbed else "cloudsc2_nl"
        dev.box.stencil(name, c.ext, dev.eta, c.dt, **kw, **_pre("out_", out))
        if not fused and not perturbed:      # the register path takes the misaligned rows, the LDS ring everything else
            assert _lib.last_kernel().startswith("cs2::nl_kernel" if misaligned else "cs2::nl_ring_kernel"), _lib.last_kernel()
        return {**(_res("nl", {"qsat": kw["out_qsat"]}, _nz) if fused else {}), **_res("nl", out, nlev_of)}
    return run


def _nl_ens(fused, shared=False):
    def run(dev, absent=False):
        c, names, out = dev.c, STEP_IN if fused else NL_IN, dev.ens_nans(NL_OUT)
        qsat = dev.ens.nan() if fused else None
        if shared:
            shared_state.enss_nl(_SharedCall(dev), dev.shared_members(names), out, qsat)
        else:
            ens_nl(dev.ens, c.ext, dev.members("state", names), dev.eta, c.dt, out, qsat)
        assert dev.ens.gaps_untouched(), "nl ensemble: the gap between members was written"
        return {**_res_members("nl", out, nlev_of), **(_res_members("nl", {"qsat": qsat}, _nz) if fused else {})}
    return run


def _saturation(dev, absent=False):
    st, qsat = dev.put("state", ("ap", "t")), dev.box.nan()
    dev.stencil("saturation", NZ, in_ap=st["ap"], in_t=st["t"], out_qsat=qsat)
    return _res("nl", {"qsat": qsat}, _nz)


def _state_increment(dev, absent=False):
    out = dev.nans(INC)
    dev.stencil("state_increment", NZ + 1, f=0.01, **_pre("in_", dev.put("state", INC)), **_pre("out_", out, "_i"))
    return _res("nl", out, _all)


def _perturbed_state(dev, absent=False):
    out = dev.nans(INC)
    dev.stencil("perturbed_state", NZ + 1, f=0.5, **_pre("in_", dev.put("state", INC)), **_pre("in_", dev.put("tl", INC), "_i"),
                **_pre("out_", out))
    return _res("nl", out, _all)


def _column_dots(dev, absent=False):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.reductions import column_dots

    a, b = dev.put("state", NL_IN), dev.put("tl", NL_IN)
    dots = column_dots([a[n] for n in NL_IN], [b[n] for n in NL_IN])
    return {("nl", 0, 0, "dots"): (dots.cpu().numpy()[None, :], 1)}


class Entry(NamedTuple):
    name: str                   # the C entry `cloudsc2_<name>_*`, or the stencil
    kind: str                   # "nl", "tl" (perturbations in) or "ad" (forcings in)
    run: Callable               # (Dev, absent=False) -> results
    evap: str = "any"           # LEVAPLS2 / LDRAIN1D: "any" = taken, "never" = refused, "only" = required
    members: bool = False       # every member is run
    dirs: bool = False          # every direction is run
    masked: bool = False        # an absent perturbation / forcing is a NULL entry
    misaligned: bool = False    # wants rows that are not 16-byte aligned
    flags: bool = True          # False: no switch of `flag_sets` reaches the entry (pointwise helpers): default externals only


ENTRIES = [
    # NL kernels and the pointwise helpers: locality and permutation only
    Entry("cloudsc2_nl", "nl", _nl()),
    Entry("cloudsc2_nl[register path]", "nl", _nl(misaligned=True), misaligned=True),
    Entry("cloudsc2_nl_saturation", "nl", _nl(fused=True)),
    Entry("cloudsc2_nl_saturation[register path]", "nl", _nl(fused=True), misaligned=True),
    Entry("cloudsc2_nl_perturbed", "nl", _nl(perturbed=True)),
    Entry("nl_ens", "nl", _nl_ens(False), members=True),
    Entry("nl_fused_ens", "nl", _nl_ens(True), members=True),
    Entry("nl_enss", "nl", _nl_ens(False, shared=True), members=True),
    Entry("nl_fused_enss", "nl", _nl_ens(True, shared=True), members=True),
    Entry("saturation", "nl", _saturation, flags=False),
    Entry("state_increment", "nl", _state_increment, flags=False),
    Entry("perturbed_state", "nl", _perturbed_state, flags=False),
    Entry("column_dots", "nl", _column_dots, flags=False),
    # tangent-linear
    Entry("cloudsc2_tl", "tl", _dense_tl(False)),
    Entry("cloudsc2_tl_incremented", "tl", _dense_tl(True)),
    Entry("tl_masked", "tl", _tl("cloudsc2_tl_masked", NL_IN), masked=True),
    Entry("tl_step", "tl", _tl("cloudsc2_tl_step", STEP_IN), masked=True),
    Entry("tl_multi", "tl", _tl("cloudsc2_tl_multi", NL_IN, multi=True), dirs=True, masked=True),
    Entry("tl_multi_step", "tl", _tl("cloudsc2_tl_multi_step", STEP_IN, multi=True), dirs=True, masked=True),
    Entry("tl_ens", "tl", _tl_ens("tl_ens", NL_IN), members=True, masked=True),
    Entry("tl_step_ens", "tl", _tl_ens("tl_step_ens", STEP_IN), members=True, masked=True),
    Entry("tl_enss", "tl", _tl_ens("tl_enss", NL_IN, shared=True), members=True, masked=True),
    Entry("tl_step_enss", "tl", _tl_ens("tl_step_enss", STEP_IN, shared=True), members=True, masked=True),
    Entry("saturation_tl", "tl", _saturation_tl, masked=True, flags=False),
    # adjoint
    Entry("cloudsc2_ad", "ad", _dense_ad(False)),
    Entry("cloudsc2_ad_from_trajectory", "ad", _dense_ad(True), evap="never"),
    Entry("ad_masked", "ad", _ad("cloudsc2_ad_masked", NL_IN), evap="never", masked=True),
    Entry("ad_step", "ad", _ad("cloudsc2_ad_step", STEP_IN), evap="never", masked=True),
    Entry("ad_multi", "ad", _ad("cloudsc2_ad_multi", NL_IN, multi=True), evap="never", dirs=True, masked=True),
    Entry("ad_multi_step", "ad", _ad("cloudsc2_ad_multi_step", STEP_IN, multi=True), evap="never", dirs=True, masked=True),
    Entry("ad_ens", "ad", _ad_ens("ad_ens", NL_IN), evap="never", members=True, masked=True),
    Entry("ad_step_ens", "ad", _ad_ens("ad_step_ens", STEP_IN), evap="never", members=True, masked=True),
    Entry("ad_enss", "ad", _ad_ens("ad_enss", NL_IN, shared=True), evap="never", members=True, masked=True),
    Entry("ad_step_enss", "ad", _ad_ens("ad_step_enss", STEP_IN, shared=True), evap="never", members=True, masked=True),
    Entry("ad_evap", "ad", _ad("ad_evap", NL_IN, evap=True), evap="only", masked=True),
    Entry("ad_evap_step", "ad", _ad("ad_evap_step", STEP_IN, evap=True), evap="only", masked=True),
    Entry("ad_evap_multi", "ad", _ad("ad_evap_multi", NL_IN, multi=True, evap=True), evap="only", dirs=True, masked=True),
    Entry("ad_evap_multi_step", "ad", _ad("ad_evap_multi_step", STEP_IN, multi=True, evap=True), evap="only", dirs=True,
          masked=True),
    Entry("ad_evap_ens", "ad", _ad_ens("ad_evap_ens", NL_IN, evap=True), evap="only", members=True, masked=True),
    Entry("ad_evap_step_ens", "ad", _ad_ens("ad_evap_step_ens", STEP_IN, evap=True), evap="only", members=True, masked=True),
    Entry("ad_multi_ens", "ad", _ad_mdirs("multi", NL_IN), evap="never", members=True, dirs=True, masked=True),
    Entry("ad_multi_step_ens", "ad", _ad_mdirs("step", STEP_IN), evap="never", members=True, dirs=True, masked=True),
    Entry("saturation_ad", "ad", _saturation_ad(False), flags=False),
    Entry("saturation_ad[accumulate]", "ad", _saturation_ad(True), flags=False),
]
DERIVATIVES = [e for e in ENTRIES if e.kind != "nl"]


def flag_sets(entry):
    """the externals an entry is run under: default, LREGCL = False, for adjoints AD_TRAJ_FIX = 1, and where it has an
    evaporation form LEVAPLS2 and LDRAIN1D (an entry that has only that form: those two, and LEVAPLS2 with the others)"""
    if entry.evap == "only":
        return [L2, D1, dict(L2, **NOREG), dict(L2, **FIX)]
    sets = [BASE, NOREG] + ([FIX] if entry.kind == "ad" else [])
    return sets + ([L2, D1] if entry.evap == "any" else [])


def configurations(entry):
    """(nx, window, flags): the small size under every set of externals, the large one (a second workgroup) under the first
    and the last set, and one `lev_stride` window"""
    sets = flag_sets(entry) if entry.flags else [BASE]
    dense = [(NXS[0], False, flags) for flags in sets] + [(NXS[1], False, flags) for flags in (sets[0], sets[-1])[:len(sets)]]
    return dense if entry.misaligned else dense + [(NXS[0], True, sets[0])]


def device_case(gpu, entry, case, window=False):
    return Dev(gpu, case, window, entry.misaligned)


def label(nx, window, flags):
    return f"nx={nx}{' window' if window else ''} {'+'.join(f'{k}={v}' for k, v in sorted(flags.items())) or 'default'}"
