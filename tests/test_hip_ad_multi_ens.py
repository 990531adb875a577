"""Members times directions on the GPU (C ABI `cloudsc2_ad_multi_ens_*` / `cloudsc2_ad_multi_step_ens_*`,
`autodiff.ad_multi_ens` / `ad_step_multi_ens`): every member and direction of every wanted adjoint equals what `ad_multi` /
`ad_step_multi` gives for that member alone - `assert_close` at its default, the bound the ensemble tests hold their launches
to against the singles; whether it was bit-equal is printed - and nothing else is touched.

Every member is another seeded case (`SEED + 100 + m`).  The forcing of direction d of a member is the ten perturbed outputs
of the single tangent-linear launch (`tl_masked` / `tl_step`) on the member's 1 % increments scaled by d + 1, so a wrong
member base and a wrong direction base both show; the trajectory fluxes are that launch's NL outputs.  `eta`, which the
members share, is member 0's.

Shapes `(nmem, ndir, nx, nz, window, member gap, direction gap)`, the smallest at which each index can go wrong: one member
and a partial wave; the most directions (the largest LDS) with a last block of one column per member; 8 blocks (the XCD
remap active) with an odd direction count; many one-column members; windows of wider allocations (lev_stride > nx); padded
member and direction strides.

Against the NumPy oracle: 100 x `assert_close`, the bound of tests/test_hip_ad_multi.py, for the step family chained with the
analytic derivative of `saturation` (tests/saturation_oracle.py)."""
import numpy as np
import pytest

from derivative_support import SEED, STATE4, STEP_IN, TND4, Box, Ens, host_case
from helpers import (NL_IN, NL_OUT, adjoint_nlev_of, assert_close, externals, from_device, increments, run_oracle_ad,
                     run_oracle_nl, run_oracle_tl)
from saturation_oracle import saturation_derivative

pytestmark = pytest.mark.gpu

#: family -> (C entry, the call on one member, the kernel, input names, single TL call, the thin call)
FAMILIES = {"multi": ("ad_multi_ens", "ad_multi", "cs2::ad_mdirs_kernel", NL_IN, "tl_masked", "ad_multi_ens"),
            "step": ("ad_multi_step_ens", "ad_step_multi", "cs2::ad_mdirs_step_kernel", STEP_IN, "tl_step", "ad_step_multi_ens")}
#: (nmem, ndir, nx, nz, window, member gap, direction gap)
SHAPES = [(1, 2, 63, 137, False, 0, 0), (3, 8, 257, 137, False, 0, 0), (4, 3, 300, 137, False, 0, 0), (16, 2, 1, 5, False, 0, 0),
          (2, 3, 130, 40, True, 0, 0), (3, 2, 63, 137, False, 1000, 500)]
_host = {}


def _member(nx, nz, dtype, m):
    """member m's host case and its 1 % increments, computed once"""
    key = (nx, nz, np.dtype(dtype), m)
    if key not in _host:
        fields, eta, dt = host_case(nx, nz, dtype, seed=SEED + 100 + m)
        _host[key] = (fields, eta, dt, increments(fields, 0.01))
    return _host[key]


class MD:
    """NaN-prefilled (nmem, ndir, nx, 1, nz+1) batches of one geometry, member-major: direction d of member m starts
    m * ms + d * ds elements behind the first"""

    def __init__(self, box, nmem, ndir, mgap, dgap):
        self.box, self.nmem, self.ndir, self.bufs = box, nmem, ndir, []
        self.ds = box.dir_stride + dgap
        self.ms = (ndir - 1) * self.ds + box.dir_stride + mgap

    def nan(self):
        b = self.box
        buf = b.torch.full((self.nmem * self.ms,), float("nan"), dtype=b.dt, device=b.device)
        self.bufs.append(buf)
        return buf.as_strided((self.nmem, self.ndir, b.nx, 1, b.nz + 1), (self.ms, self.ds, 1, b.dir_stride, b.pitch), b.col0)

    def put(self, arrs):
        """arrs[m][d]: [level][column]"""
        f = self.nan()
        for m in range(self.nmem):
            for d in range(self.ndir):
                self.box.storage.klayout(f[m, d]).copy_(self.box.torch.as_tensor(arrs[m][d]))
        return f

    def outside_untouched(self):
        """everything that is no element of a field - between members, between directions, beside a window - is still NaN"""
        b = self.box
        field = np.zeros((b.nz + 1, b.pitch), dtype=bool)
        field[:, b.col0:b.col0 + b.nx] = True
        covered = np.zeros((self.nmem, self.ms), dtype=bool)
        for d in range(self.ndir):
            covered[:, d * self.ds:d * self.ds + b.dir_stride] = field.reshape(-1)
        return all(bool(np.isnan(buf.cpu().numpy().reshape(self.nmem, self.ms)[~covered]).all()) for buf in self.bufs)


def _setup(gpu, family, shape, dtype, **flags):
    """-> box, ens, md, externals, eta, dt, member-major state and trajectory fluxes, the host forcing w[m][d]"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    nmem, ndir, nx, nz, window, mgap, dgap = shape
    names, tl = FAMILIES[family][3], getattr(autodiff, FAMILIES[family][4])
    box = Box(nx, nz, dtype, gpu, window)
    ens, md = Ens(box, nmem, mgap), MD(box, nmem, ndir, mgap, dgap)
    ext = externals(NLEV=nz, **flags)
    cases = [_member(nx, nz, dtype, m) for m in range(nmem)]
    eta, dt = torch.as_tensor(cases[0][1], device=gpu), cases[0][2]
    state = {n: ens.put([c[0]["in_" + n] for c in cases]) for n in names}
    traj, w = {"fplsl": ens.nan(), "fplsn": ens.nan()}, []
    for m, (fields, _, _, inc) in enumerate(cases):
        st, rows = {n: f[m] for n, f in state.items()}, []
        for d in range(ndir):
            pert = {n: box.put(((d + 1) * inc["in_" + n + "_i"]).astype(dtype)) for n in names}
            nl, out_i = tl(st, pert, eta, dt, ext, want=NL_OUT, write_nl=d == 0)
            if d == 0:
                traj["fplsl"][m].copy_(nl["fplsl"])
                traj["fplsn"][m].copy_(nl["fplsn"])
            rows.append({n: from_device(out_i[n]) for n in NL_OUT})
        w.append(rows)
    return box, ens, md, ext, eta, dt, state, traj, w


def _raw(family, box, ens, md, ext, state, forcing, eta, dt, traj, out_adj):
    """the C entry on the test's own buffers: member 0 / direction 0 pointers, the three member strides"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    entry = FAMILIES[family][0]
    p = autodiff._params(ext, box.nz)
    zero = autodiff._zero_line(torch.device(box.device), box.dt)
    m0 = lambda fields: {n: f[0] for n, f in fields.items()}          # noqa: E731
    d0 = lambda fields: {n: f[0, 0] for n, f in fields.items()}       # noqa: E731
    args = autodiff._ad_args(p, (box.nx, box.nz + 1, box.pitch), m0(state), d0(forcing), zero, eta, m0(traj), d0(out_adj), dt,
                             int(torch.cuda.current_stream().cuda_stream), (md.ndir, md.ds, md.ds),
                             members=(ens.nmem, ens.ms, md.ms, md.ms))
    _lib.check(getattr(_lib.load(), f"cloudsc2_{entry}_{box.sfx}")(*args), entry)
    torch.cuda.synchronize()
    assert _lib.last_kernel() == FAMILIES[family][2]


def _members_alone(family, state, forcing, eta, dt, ext, traj, want, nmem):
    """`ad_multi` / `ad_step_multi` on each member alone, every cotangent in one launch -> [m] {name: (ndir, nx, 1, nz+1)}"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    one = getattr(autodiff, FAMILIES[family][1])
    return [one({n: f[m] for n, f in state.items()}, {n: f[m] for n, f in forcing.items()}, eta, dt, ext,
                traj={n: f[m] for n, f in traj.items()}, want=want, width=_lib.AD_MAX_DIRS) for m in range(nmem)]


def _compare(what, got, rows, want, shape, dtype):
    nmem, ndir, nx, nz = shape[:4]
    equal = True
    for n in want:
        k = adjoint_nlev_of(n, nz)
        for m in range(nmem):
            for d in range(ndir):
                a, b = from_device(got[n][m, d]), from_device(rows[m][n][d])
                assert not np.isnan(a[:k]).any(), (what, n, m, d)
                assert_close(f"{what} out_{n}_i[{m}, {d}]", a[:k], b[:k], dtype)
                assert np.isnan(a[k:]).all(), f"{what} {n}[{m}, {d}]: padding level written"
                equal = equal and np.array_equal(a[:k], b[:k])
    print(f"{what} {shape} {np.dtype(dtype).name}: bit-equal to ad_multi on each member alone: {equal}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_full_mask_every_member_and_direction_equals_the_members_own_launch(gpu, shape, family, dtype):
    names = FAMILIES[family][3]
    nmem, ndir = shape[:2]
    box, ens, md, ext, eta, dt, state, traj, w = _setup(gpu, family, shape, dtype)
    forcing = {n: md.put([[w[m][d][n] for d in range(ndir)] for m in range(nmem)]) for n in NL_OUT}
    rows = _members_alone(family, state, forcing, eta, dt, ext, traj, names, nmem)
    live = [bool(r["t"].any()) and bool(r["aph"].any()) for r in rows]
    print(f"{FAMILIES[family][0]} {shape}: members with non-zero adjoints of t and aph: {sum(live)} of {nmem}")
    assert all(live) or shape[3] < 137       # five levels of one column may have none (14 of the 16 members have some)
    out_adj = {n: md.nan() for n in names}
    _raw(family, box, ens, md, ext, state, forcing, eta, dt, traj, out_adj)
    _compare(FAMILIES[family][0], out_adj, rows, names, shape, dtype)
    assert md.outside_untouched() and ens.gaps_untouched()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_4dvar_mask_absent_forcings_and_unwanted_adjoints(gpu, family, dtype):
    """forcing on the four tendencies (every other one is read from the zero line by every member and direction), adjoints of
    t, q, ql, qi.  An unwanted adjoint is a NULL entry of `out_adj`: the call has no storage of it to leave untouched, so what
    is asserted is that the wanted ones equal the member's own launch under the same mask and that nothing outside the
    wanted fields' elements - the gaps between members and between directions - is written"""
    shape = (3, 2, 63, 137, False, 1000, 500)
    nmem, ndir = shape[:2]
    box, ens, md, ext, eta, dt, state, traj, w = _setup(gpu, family, shape, dtype)
    forcing = {n: md.put([[w[m][d][n] for d in range(ndir)] for m in range(nmem)]) for n in TND4}
    rows = _members_alone(family, state, forcing, eta, dt, ext, traj, STATE4, nmem)
    out_adj = {n: md.nan() for n in STATE4}
    _raw(family, box, ens, md, ext, state, forcing, eta, dt, traj, out_adj)
    _compare(FAMILIES[family][0] + " [4dvar]", out_adj, rows, STATE4, shape, dtype)
    assert md.outside_untouched() and ens.gaps_untouched()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_without_lregcl(gpu, family, dtype):
    shape = (4, 3, 300, 137, False, 0, 0)
    names = FAMILIES[family][3]
    nmem, ndir = shape[:2]
    box, ens, md, ext, eta, dt, state, traj, w = _setup(gpu, family, shape, dtype, LREGCL=False)
    forcing = {n: md.put([[w[m][d][n] for d in range(ndir)] for m in range(nmem)]) for n in NL_OUT}
    rows = _members_alone(family, state, forcing, eta, dt, ext, traj, names, nmem)
    out_adj = {n: md.nan() for n in names}
    _raw(family, box, ens, md, ext, state, forcing, eta, dt, traj, out_adj)
    _compare(FAMILIES[family][0] + " LREGCL=False", out_adj, rows, names, shape, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_thin_call_serves_the_directions_in_chunks_one_launch_for_all_members(gpu, family, dtype):
    """`ad_multi_ens` / `ad_step_multi_ens` at width 8 (one launch) and at width 3, which does not divide 8 (chunks of 3, 3
    and 2); one forcing arrives packed where the others are padded and is copied; the results are packed blocks"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage

    shape = (3, 8, 257, 137, False, 1000, 500)
    nmem, ndir, nx, nz = shape[:4]
    box, ens, md, ext, eta, dt, state, traj, w = _setup(gpu, family, shape, dtype)
    forcing = {n: md.put([[w[m][d][n] for d in range(ndir)] for m in range(nmem)]) for n in TND4}
    rows = _members_alone(family, state, forcing, eta, dt, ext, traj, STATE4, nmem)
    packed = np.stack([np.stack([w[m][d]["tnd_q"].T[:, None, :] for d in range(ndir)]) for m in range(nmem)])
    given = dict(forcing, tnd_q=torch.as_tensor(packed, device=gpu))
    call = getattr(autodiff, FAMILIES[family][5])
    for width in (_lib.AD_MAX_DIRS, 3):
        adj = call(state, given, eta, dt, ext, traj=traj, want=STATE4, width=width)
        assert _lib.last_kernel() == FAMILIES[family][2]
        torch.cuda.synchronize()
        assert sorted(adj) == sorted(STATE4)
        for n in STATE4:
            assert tuple(adj[n].shape) == (nmem, ndir, nx, 1, nz + 1)
            assert storage.direction_stride(adj[n].flatten(0, 1)) == storage.direction_stride(adj[n][0])   # packed blocks
            for m in range(nmem):
                for d in range(ndir):
                    a = from_device(adj[n][m, d])
                    assert_close(f"{FAMILIES[family][5]} width {width} out_{n}_i[{m}, {d}]", a[:nz],
                                 from_device(rows[m][n][d])[:nz], dtype)
                    assert not a[nz:].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_members_and_directions_equal_the_oracle(gpu, family, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    shape = (2, 2, 63, 137, False, 0, 0)
    nmem, ndir, nx, nz = shape[:4]
    names, tl = FAMILIES[family][3], getattr(autodiff, FAMILIES[family][4])
    ext = externals(NLEV=nz, AD_TRAJ_FIX=1)
    box = Box(nx, nz, dtype, gpu, False)
    ens, md = Ens(box, nmem, 0), MD(box, nmem, ndir, 0, 0)
    cases = [_member(nx, nz, dtype, m) for m in range(nmem)]
    eta, dt = torch.as_tensor(cases[0][1], device=gpu), cases[0][2]
    state = {n: ens.put([c[0]["in_" + n] for c in cases]) for n in names}
    traj, w, want = {"fplsl": ens.nan(), "fplsn": ens.nan()}, [], []
    heta = cases[0][1]      # `eta` is shared by the members: member 0's
    for m, (fields, _, _, inc) in enumerate(cases):
        # the device's own trajectory fluxes for the launch, the oracle's own for the oracle
        nl, _ = tl({n: f[m] for n, f in state.items()}, {"t": box.put(inc["in_t_i"])}, eta, dt, ext, want=("tnd_t",),
                   write_nl=True)
        traj["fplsl"][m].copy_(nl["fplsl"])
        traj["fplsn"][m].copy_(nl["fplsn"])
        nl0 = run_oracle_nl(fields, heta, dt, ext)
        _, g_t, g_ap, _ = saturation_derivative(fields["in_ap"], fields["in_t"], ext)
        w.append([]), want.append([])
        for d in range(ndir):
            tl_i = run_oracle_tl(fields, {k: ((d + 1) * v).astype(dtype) for k, v in inc.items()}, heta, dt, ext)[1]
            adj = dict(run_oracle_ad(fields, tl_i, heta, dt, ext, traj=nl0)[1])
            if family == "step":
                q = adj["qsat"].astype(np.float64)
                adj["t"] = (adj["t"].astype(np.float64) + g_t * q).astype(dtype)
                adj["ap"] = (adj["ap"].astype(np.float64) + g_ap * q).astype(dtype)
            w[m].append(tl_i), want[m].append(adj)
    forcing = {n: md.put([[w[m][d][n] for d in range(ndir)] for m in range(nmem)]) for n in NL_OUT}
    out_adj = {n: md.nan() for n in names}
    _raw(family, box, ens, md, ext, state, forcing, eta, dt, traj, out_adj)
    failures = []
    for m in range(nmem):
        for d in range(ndir):
            for n in names:
                k = adjoint_nlev_of(n, nz)
                a, b = from_device(out_adj[n][m, d])[:k], want[m][d][n][:k]
                scale = float(np.abs(b).max())
                err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
                print(f"{FAMILIES[family][0]} vs oracle {np.dtype(dtype).name} out_{n}_i[{m}, {d}]: max |err| / scale "
                      f"{err / scale if scale else 0.0:.3e}")
                try:
                    assert_close(f"{FAMILIES[family][0]} vs oracle out_{n}_i[{m}, {d}]", a, b, dtype, rtol_mul=100.0)
                except AssertionError as exc:
                    failures.append(str(exc))
    assert not failures, "\n".join(failures)
