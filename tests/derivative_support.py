"""Scaffolding the tests of the derivative kernels share (masked, step and multi-direction TL / AD, `autodiff`): the names
and shapes they agree on, host cases computed once and never modified, device fields of one geometry (`Box`), the raw C
entries on buffers a test supplies, and the direction-by-direction comparison of a batch with the single launches.

`torch` and the package are imported inside functions, so that collecting a test module needs neither."""
import ctypes

import numpy as np

from helpers import (NL_IN, NL_OUT, assert_close, externals, from_device, increments, nl_case, nlev_of, run_oracle_nl,
                     run_oracle_tl, to_device)
from saturation_oracle import saturation_derivative

SEED = 20240807
STATE4 = ("t", "q", "ql", "qi")
TND4 = ("tnd_t", "tnd_q", "tnd_ql", "tnd_qi")
STEP_IN = tuple(n for n in NL_IN if n != "qsat")
#: (nx, nz, window): one column, a partial wave, two blocks, a column window of a wider allocation, another level count
SHAPES = [(1, 137, False), (63, 137, False), (200, 137, False), (333, 137, True), (130, 40, False)]

# ----------------------------------------------------------------------------------------------
# host cases: computed once per key, shared by every test module, never modified
# ----------------------------------------------------------------------------------------------
_host = {}


def _once(key, make):
    if key not in _host:
        _host[key] = make()
    return _host[key]


def host_case(nx, nz, dtype, seed=SEED):
    """-> fields (in_*, [level][column]), eta, dt"""
    return _once(("case", nx, nz, np.dtype(dtype), seed), lambda: nl_case(nx, nz, dtype=dtype, seed=seed))


def host_increments(nx, nz, dtype):
    """the 1 % increments of the case's inputs"""
    return _once(("increments", nx, nz, np.dtype(dtype)), lambda: increments(host_case(nx, nz, dtype)[0], 0.01))


def oracle_nl(nx, nz, dtype):
    """the oracle's NL outputs for the case"""
    return _once(("nl", nx, nz, np.dtype(dtype)), lambda: run_oracle_nl(*host_case(nx, nz, dtype), externals()))


def oracle_tl_i(nx, nz, dtype):
    """the oracle's TL outputs for the 1 % increments (TL does not depend on AD_TRAJ_FIX)"""
    def make():
        fields, eta, dt = host_case(nx, nz, dtype)
        return run_oracle_tl(fields, host_increments(nx, nz, dtype), eta, dt, externals(NLEV=nz))[1]
    return _once(("tl_i", nx, nz, np.dtype(dtype)), make)


def host_directions(nx, nz, dtype, ndir):
    """`ndir` independent directions {NL_IN name: [level][column]}: direction d is the `increments` of a state drawn with
    seed SEED + 1 + d, with factor 0.01 (d + 1); fewer directions are the first ones of more"""
    dirs = _once(("directions", nx, nz, np.dtype(dtype)), list)
    while len(dirs) < ndir:
        d = len(dirs)
        other = nl_case(nx, nz, dtype=dtype, seed=SEED + 1 + d)[0]
        dirs.append({k[3:-2]: v for k, v in increments(other, 0.01 * (d + 1)).items()})
    return dirs[:ndir]


def direction_case(nx, nz, dtype, ndir):
    """-> fields, eta, dt, the first `ndir` directions"""
    return (*host_case(nx, nz, dtype), host_directions(nx, nz, dtype, ndir))


def autodiff_case(dtype, nx=200, nz=137, **flags):
    """what the tests of `cloudsc2` / `cloudsc2_step` differentiate: host inputs (in_qsat: the oracle's saturation), a weight
    field, the oracle's NL outputs and saturation's derivative, under the externals `flags` give"""
    def make():
        ext = externals(**flags)
        fields, eta, dt = nl_case(nx, nz, dtype=dtype, ext=ext)
        w = np.random.default_rng(5).standard_normal(fields["in_t"].shape).astype(dtype)
        _, g_t, g_ap, _ = saturation_derivative(fields["in_ap"], fields["in_t"], ext)
        return dict(fields=fields, eta=eta, dt=dt, w=w, nl0=run_oracle_nl(fields, eta, dt, ext), g_t=g_t, g_ap=g_ap, ext=ext)
    return _once(("autodiff", np.dtype(dtype), nx, nz, tuple(sorted(flags.items()))), make)


def device_state(gpu, c, names, grad=()):
    """an `autodiff_case` on the device -> the state of `names` (those of `grad` requiring a gradient), eta, dt, the weight"""
    import torch

    dev = to_device(c["fields"], gpu)
    state = {n: dev["in_" + n] for n in names}
    for n in grad:
        state[n].requires_grad_(True)
    return state, torch.as_tensor(c["eta"], device=gpu), c["dt"], to_device({"w": c["w"]}, gpu)["w"]


# ----------------------------------------------------------------------------------------------
# device fields
# ----------------------------------------------------------------------------------------------
class Box:
    """device fields of one geometry - dense storages, or column windows of wider allocations (lev_stride > nx) - and
    batches of them: `slots` fields in one allocation, one behind the other.  Everything is NaN-prefilled."""

    def __init__(self, nx, nz, dtype, device, window):
        import torch

        from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage

        self.nx, self.nz, self.device, self.torch, self.storage = nx, nz, device, torch, storage
        self.dt = storage.torch_dtype(dtype)
        self.sfx = "f64" if self.dt == torch.float64 else "f32"
        self.pitch = storage.level_pitch(nx, dtype) + (192 if window else 0)
        self.col0 = 64 if window else 0
        # the C entries are given `pitch`; the package reads the same number off a field
        assert storage.field_geometry(self.nan())[2] == self.pitch

    def nan(self, slots=None):
        shape = (self.nz + 1, self.pitch) if slots is None else (slots, self.nz + 1, self.pitch)
        buf = self.torch.full(shape, float("nan"), dtype=self.dt, device=self.device)[..., self.col0:self.col0 + self.nx]
        return self.storage.logical_view(buf) if slots is None else buf.unsqueeze(2).permute(0, 3, 2, 1)

    def put(self, arr):
        f = self.nan()
        self.storage.klayout(f).copy_(self.torch.as_tensor(arr))
        return f

    def zeros(self):
        return self.put(np.zeros((self.nz + 1, self.nx)))

    def state(self, fields, names=NL_IN):
        return {n: self.put(fields["in_" + n]) for n in names}

    def batch(self, arrs, slots=None):
        """(slots, nx, 1, nz+1) with direction d = arrs[d]; further slots stay NaN"""
        f = self.nan(len(arrs) if slots is None else slots)
        for d, a in enumerate(arrs):
            self.storage.klayout(f[d]).copy_(self.torch.as_tensor(a))
        return f

    @property
    def dir_stride(self):
        return (self.nz + 1) * self.pitch

    def stencil(self, name, ext, eta, dt, **fields):
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

        compile_stencil(name, ext)(**fields, in_eta=eta, dt=dt, origin=(0, 0, 0), domain=(self.nx, 1, self.nz + 1),
                                   validate_args=True, exec_info=None)

    def nl_fluxes(self, state, ext, eta, dt):
        outs = {n: self.nan() for n in NL_OUT}
        self.stencil("cloudsc2_nl", ext, eta, dt, **{"in_" + n: f for n, f in state.items()},
                     **{"out_" + n: f for n, f in outs.items()})
        return {"fplsl": outs["fplsl"], "fplsn": outs["fplsn"]}

    def dense_ad_traj(self, state, forcing, traj, ext, eta, dt):
        adj = {n: self.nan() for n in NL_IN}
        self.stencil("cloudsc2_ad_from_trajectory", ext, eta, dt, **{"in_" + n: f for n, f in state.items()},
                     **{"in_" + n + "_i": forcing[n] for n in NL_OUT}, traj_fplsl=traj["fplsl"], traj_fplsn=traj["fplsn"],
                     **{"out_" + n + "_i": f for n, f in adj.items()})
        return adj

    def dense_tl(self, state, pert, ext, eta, dt):
        out, out_i = {n: self.nan() for n in NL_OUT}, {n: self.nan() for n in NL_OUT}
        self.stencil("cloudsc2_tl", ext, eta, dt, **{"in_" + n: f for n, f in state.items()},
                     **{"in_" + n + "_i": pert[n] for n in NL_IN}, **{"out_" + n: f for n, f in out.items()},
                     **{"out_" + n + "_i": f for n, f in out_i.items()})
        return out, out_i


# ----------------------------------------------------------------------------------------------
# the C entries themselves, on buffers the test supplies
# ----------------------------------------------------------------------------------------------
def _raw(entry, box, ext, state, dirs, dir_names, eta, dt, rest, ndir):
    """`cloudsc2_{tl,ad}_{masked,step,multi,multi_step}`: (params, nx, nz, lev_stride, state, directions, zero line, eta,
    *rest, dt, stream) and, with `ndir`, the three direction arguments"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    p = autodiff._params(ext, box.nz)
    tail = () if ndir is None else (ndir, box.dir_stride, box.dir_stride)
    rc = getattr(_lib.load(), f"{entry}_{box.sfx}")(
        ctypes.byref(p), box.nx, box.nz, box.pitch, autodiff._ptrs(state, NL_IN), _ptrs(dirs, dir_names, ndir),
        autodiff._zero_line(torch.device(box.device), box.dt).data_ptr(), eta.data_ptr(), *rest, float(dt),
        int(torch.cuda.current_stream().cuda_stream), *tail)
    _lib.check(rc, entry)


def _ptrs(fields, names, ndir):
    """the pointer array of fields or, with `ndir`, of the first direction of batches"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    return autodiff._ptrs(fields if ndir is None else {n: f[0] for n, f in fields.items()}, names)


def raw_tl(entry, box, ext, state, pert, eta, dt, out, out_i, ndir=None):
    """a TL entry: `out` is None or all ten NL outputs, `out_i` maps the wanted names to buffers; with `ndir`, `pert` and
    `out_i` map names to batches"""
    rest = (None if out is None else _ptrs(out, NL_OUT, None), _ptrs(out_i, NL_OUT, ndir))
    _raw(entry, box, ext, state, pert, NL_IN, eta, dt, rest, ndir)


def raw_ad(entry, box, ext, state, forcing, eta, dt, traj, out_adj, ndir=None):
    """an AD entry: `out_adj` maps the wanted names to buffers; with `ndir`, `forcing` and `out_adj` map names to batches"""
    rest = (traj["fplsl"].data_ptr(), traj["fplsn"].data_ptr(), _ptrs(out_adj, NL_IN, ndir))
    _raw(entry, box, ext, state, forcing, NL_OUT, eta, dt, rest, ndir)


# ----------------------------------------------------------------------------------------------
# ensembles: member-major batches and the C entries on them
# ----------------------------------------------------------------------------------------------
class Ens:
    """NaN-prefilled member-major batches of one geometry: member m of a field starts m * ms elements behind member 0"""

    def __init__(self, box, nmem, gap):
        self.box, self.nmem, self.ms, self.bufs = box, nmem, box.dir_stride + gap, []

    def nan(self):
        b = self.box
        buf = b.torch.full((self.nmem, self.ms), float("nan"), dtype=b.dt, device=b.device)
        self.bufs.append(buf)
        return buf[:, :b.dir_stride].view(self.nmem, b.nz + 1, b.pitch)[:, :, b.col0:b.col0 + b.nx].unsqueeze(2).permute(0, 3, 2, 1)

    def put(self, arrs):
        f = self.nan()
        for m, a in enumerate(arrs):
            self.box.storage.klayout(f[m]).copy_(self.box.torch.as_tensor(a))
        return f

    def gaps_untouched(self):
        return all(bool(buf[:, self.box.dir_stride:].isnan().all()) for buf in self.bufs)


def _launch(entry, ens, ext, args_of):
    """one ensemble entry; `args_of(p, geo, zero, stream)` -> the single entry's arguments"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    box = ens.box
    p = autodiff._params(ext, box.nz)
    zero = autodiff._zero_line(torch.device(box.device), box.dt)
    args = args_of(p, (box.nx, box.nz + 1, box.pitch), zero, int(torch.cuda.current_stream().cuda_stream))
    _lib.check(getattr(_lib.load(), f"cloudsc2_{entry}_{box.sfx}")(*args, ens.nmem, ens.ms), entry)
    torch.cuda.synchronize()


def _m0(fields):
    return {n: f[0] for n, f in fields.items()}


def ens_tl(entry, ens, ext, state, pert, eta, dt, out, out_i):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    _launch(entry, ens, ext, lambda p, geo, zero, stream: autodiff._tl_args(
        p, geo, _m0(state), _m0(pert), zero, eta, None if out is None else _m0(out), _m0(out_i), dt, stream))


def ens_ad(entry, ens, ext, state, forcing, eta, dt, traj, out_adj):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    _launch(entry, ens, ext, lambda p, geo, zero, stream: autodiff._ad_args(
        p, geo, _m0(state), _m0(forcing), zero, eta, _m0(traj), _m0(out_adj), dt, stream))


def ens_nl(ens, ext, state, eta, dt, out, qsat=None):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    def args(p, geo, zero, stream):
        head = (ctypes.byref(p), geo[0], geo[1] - 1, geo[2], autodiff._ptrs(_m0(state), NL_IN))
        tail = (eta.data_ptr(), autodiff._ptrs(_m0(out), NL_OUT), float(dt), stream)
        return head + tail if qsat is None else head + (None, 0.0, qsat[0].data_ptr()) + tail
    _launch("nl_ens" if qsat is None else "nl_fused_ens", ens, ext, args)


# ----------------------------------------------------------------------------------------------
# a batch of directions against the single launches
# ----------------------------------------------------------------------------------------------
def singles(single, kernel, state, dirs, eta, dt, ext, want, ndir, traj=None):
    """the single-direction launch (`kernel`) for each direction alone -> per direction {name: host array}; `single` is a
    TL call, or with `traj` an AD call"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    rows = []
    for d in range(ndir):
        one = {n: f[d] for n, f in dirs.items()}
        if traj is None:
            _, res = single(state, one, eta, dt, ext, want=want)
        else:
            res = single(state, one, eta, dt, ext, traj=traj, want=want)
        assert _lib.last_kernel() == kernel
        rows.append({n: from_device(res[n]) for n in want})
    return rows


def compare_directions(what, got_batch, rows, want, nz, dtype, ndir, levels=nlev_of):
    """direction by direction against the single launches; padding level and the slots behind `ndir` are untouched.
    `levels(name, nz)`: the levels written of a field - `nlev_of` for TL outputs, `adjoint_nlev_of` for adjoints"""
    equal = True
    for n in want:
        k = levels(n, nz)
        for d in range(ndir):
            a, b = from_device(got_batch[n][d]), rows[d][n]
            assert not np.isnan(a[:k]).any(), (what, n, d)
            assert_close(f"{what} out_{n}_i[{d}]", a[:k], b[:k], dtype)
            assert np.isnan(a[k:]).all(), f"{what} {n}[{d}]: padding level written"
            equal = equal and np.array_equal(a[:k], b[:k])
        for d in range(ndir, got_batch[n].shape[0]):
            assert np.isnan(from_device(got_batch[n][d])).all(), f"{what} {n}: slot {d} >= ndir={ndir} written"
    print(f"{what} ndir={ndir} {np.dtype(dtype).name}: bit-equal to the single launches: {equal}")
