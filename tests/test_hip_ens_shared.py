"""The shared-state ensemble kernels on the GPU (C ABI `cloudsc2_{nl,nl_fused,tl,tl_step,ad,ad_step}_enss_*`): members that
share part of their state, and members with an `eta` each.

Every shared field of these tests is member 0 of an `nmem`-member allocation whose other members are NaN, and every shared
`eta` is row 0 of an `(nmem, stride)` buffer whose other rows are NaN: a kernel that misses a mask bit reads NaN from inside
the allocation - a wrong VALUE that the comparison catches - and never beyond it.

Held against
  * the existing `*_ens_*` entry on MATERIALISED members (every field batched, the shared ones repeated): `assert_close` at
    its default for the dtype, bit-equality printed (as tests/test_hip_ad_multi.py); outputs are NaN-prefilled and the padding
    level must stay NaN;
  * the NumPy oracle, member by member on the materialised members, for all six families on all three masks
    (`hold_to_oracle`), at the tolerances tests/test_hip_ensemble.py holds the `*_ens_*` entries to;
  * with per-member `eta`: three single calls, one per vertical grid, and the oracle on each member's own grid.

Shapes: nx = 63 (a partly filled wave) and 257 (a second workgroup per member), nz = 12 on the `uniform` grid of
tests/grid_support.py (tropopause window: levels 1 .. 4), nmem 1 and 3, both precisions, one case on a `lev_stride` window."""
import ctypes

import numpy as np
import pytest

from derivative_support import SEED, STEP_IN, Box, Ens, ens_ad, ens_nl, ens_tl
from grid_support import eta_family, tropopause_window
from helpers import (NL_IN, NL_OUT, adjoint_nlev_of, assert_close, externals, from_device, increments, nl_case, nlev_of,
                     oracle, run_oracle_ad, run_oracle_nl, run_oracle_tl)
from saturation_oracle import saturation_derivative

pytestmark = pytest.mark.gpu

NZ = 12
MEMBER_FIELDS = ("t", "q", "ql", "qi", "qsat")      # what the members of a data-assimilation ensemble differ in
MASKS = {"da": tuple(n for n in NL_IN if n not in MEMBER_FIELDS), "all": NL_IN, "none": ()}
SHAPES = [(1, 63, False), (3, 257, False), (3, 63, True)]
COLUMN_MAJOR, MEMBER_MAJOR = 1 << 32, 1 << 33
_cases = {}


def _host(nmem, nx, dtype, mask):
    """materialised members on the host: member m's own fields are drawn with seed SEED + 200 + m, the fields of `mask` are
    member 0's; `all`: identical members.  eta: the `uniform` grid (a non-empty window at nz = 12)."""
    key = (nmem, nx, np.dtype(dtype), mask)
    if key not in _cases:
        draws = [nl_case(nx, NZ, dtype=dtype, seed=SEED + 200 + m) for m in range(nmem)]
        shared = MASKS[mask]
        members = [{"in_" + n: draws[0 if n in shared else m][0]["in_" + n] for n in NL_IN} for m in range(nmem)]
        for f in members:      # qsat of the member's own (ap, t), as the step forms it
            f["in_qsat"] = np.zeros_like(f["in_t"])
            oracle.saturation(f["in_ap"], f["in_t"], f["in_qsat"], externals())
        _cases[key] = members, draws[0][2]
    return _cases[key]


class Shared:
    """the device side of one case: batches for the `*_ens_*` reference, and for the shared call member-major batches of
    the members' own fields plus member 0 of NaN-filled batches for the shared ones"""

    def __init__(self, gpu, nmem, nx, window, dtype, mask, eta_host=None, eta_stride=None, **flags):
        import torch

        self.members, self.dt = _host(nmem, nx, dtype, mask)
        self.box = Box(nx, NZ, dtype, gpu, window)
        self.ens = Ens(self.box, nmem, 0)
        self.nmem, self.dtype, self.shared = nmem, dtype, MASKS[mask]
        self.ext = externals(NLEV=NZ, **flags)
        self.full = {n: self.ens.put([m["in_" + n] for m in self.members]) for n in NL_IN}
        self.part = {}
        for n in NL_IN:
            if n in self.shared:
                f = self.ens.nan()
                self.box.storage.klayout(f[0]).copy_(torch.as_tensor(self.members[0]["in_" + n]))
                self.part[n] = f            # members 1 .. stay NaN: the launch is given member 0's pointer
            else:
                self.part[n] = self.full[n]
        self.eta_host = eta_family(NZ, dtype)["uniform"] if eta_host is None else eta_host
        rows = np.atleast_2d(self.eta_host)
        stride = NZ + 1 if eta_stride is None else eta_stride
        buf = torch.full((nmem, stride), float("nan"), dtype=self.box.dt, device=gpu)
        buf[:rows.shape[0], :NZ + 1] = torch.as_tensor(rows)
        self.eta_buf, self.eta = buf, buf[0]
        self.eta_ms = stride if rows.shape[0] > 1 else 0

    def mask_bits(self, names=NL_IN, order=0):
        return sum(1 << NL_IN.index(n) for n in self.shared if n in names) | order

    def pert_host(self, names):
        same = self.shared == NL_IN
        return {n: [increments(self.members[0 if same else m], 0.01)["in_" + n + "_i"] for m in range(self.nmem)]
                for n in ("t", "q", "ql", "qi") if n in names}


def _enss(entry, s, args_of, mask, eta_ms):
    """one `cloudsc2_<entry>_*` launch: the ensemble entry's arguments + (shared_mask, eta_member_stride)"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    box = s.box
    p = autodiff._params(s.ext, box.nz)
    zero = autodiff._zero_line(torch.device(box.device), box.dt)
    args = args_of(p, (box.nx, box.nz + 1, box.pitch), zero, int(torch.cuda.current_stream().cuda_stream))
    _lib.check(getattr(_lib.load(), f"cloudsc2_{entry}_{box.sfx}")(*args, s.nmem, s.ens.ms, mask, eta_ms), entry)
    torch.cuda.synchronize()


def _m0(fields):
    return {n: f[0] for n, f in fields.items()}


def enss_nl(s, state, out, qsat=None, order=0, eta=None, eta_ms=0):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    eta = s.eta if eta is None else eta

    def args(p, geo, zero, stream):
        head = (ctypes.byref(p), geo[0], geo[1] - 1, geo[2], autodiff._ptrs(_m0(state), NL_IN))
        tail = (eta.data_ptr(), autodiff._ptrs(_m0(out), NL_OUT), float(s.dt), stream)
        return head + tail if qsat is None else head + (None, 0.0, qsat[0].data_ptr()) + tail
    _enss("nl_enss" if qsat is None else "nl_fused_enss", s, args, s.mask_bits(tuple(state), order), eta_ms)


def enss_tl(entry, s, state, pert, out, out_i, order=0, eta=None, eta_ms=0):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    eta = s.eta if eta is None else eta
    _enss(entry, s, lambda p, geo, zero, stream: autodiff._tl_args(
        p, geo, _m0(state), _m0(pert), zero, eta, None if out is None else _m0(out), _m0(out_i), s.dt, stream),
        s.mask_bits(tuple(state), order), eta_ms)


def enss_ad(entry, s, state, forcing, traj, out_adj, order=0, eta=None, eta_ms=0):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    eta = s.eta if eta is None else eta
    _enss(entry, s, lambda p, geo, zero, stream: autodiff._ad_args(
        p, geo, _m0(state), _m0(forcing), zero, eta, _m0(traj), _m0(out_adj), s.dt, stream),
        s.mask_bits(tuple(state), order), eta_ms)


def compare(what, got, ref, names, levels, dtype, identical=False):
    """every member of every field against the reference batch; the padding level stays NaN"""
    import torch

    equal = True
    for n in names:
        k = levels(n, NZ)
        for m in range(got[n].shape[0]):
            a, b = from_device(got[n][m]), from_device(ref[n][m])
            assert not np.isnan(a[:k]).any(), (what, n, m)
            torch.testing.assert_close(torch.as_tensor(a[:k]), torch.as_tensor(b[:k]), msg=lambda t: f"{what} {n}[{m}]: {t}")
            assert np.isnan(a[k:]).all(), f"{what} {n}[{m}]: padding level written"
            equal = equal and np.array_equal(a[:k], b[:k])
            if identical:
                assert np.array_equal(a[:k], from_device(got[n][0])[:k]), f"{what} {n}: members {m} and 0 differ"
    print(f"{what} {np.dtype(dtype).name}: bit-equal to the reference: {equal}")
    return equal


def _run(gpu, shape, dtype, mask, step, order=0):
    """all three launches of one family (NL or fused NL, TL, AD) on one case -> the shared call's results"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nmem, nx, window = shape
    s = Shared(gpu, nmem, nx, window, dtype, mask)
    names = STEP_IN if step else NL_IN
    full, part = {n: s.full[n] for n in names}, {n: s.part[n] for n in names}
    same = mask == "all"
    tag = f"{'step' if step else 'masked'} {shape} mask={mask}"
    # NL
    ref, got = {n: s.ens.nan() for n in NL_OUT}, {n: s.ens.nan() for n in NL_OUT}
    ref_q, got_q = (s.ens.nan(), s.ens.nan()) if step else (None, None)
    ens_nl(s.ens, s.ext, full, s.eta, s.dt, ref, ref_q)
    enss_nl(s, part, got, got_q, order)
    assert _lib.last_kernel() == ("cs2::nl_enss_kernel<saturation>" if step else "cs2::nl_enss_kernel")
    compare(f"nl_enss {tag}", dict(got, **({"qsat": got_q} if step else {})), dict(ref, **({"qsat": ref_q} if step else {})),
            NL_OUT + (("qsat",) if step else ()), nlev_of, dtype, same)
    for m, fields in enumerate(s.members):       # the NumPy oracle, member by member on the materialised members
        want = run_oracle_nl(fields, s.eta_host, s.dt, s.ext)
        for n in NL_OUT:
            k = nlev_of(n, NZ)
            assert_close(f"nl_enss {tag} oracle {n}[{m}]", from_device(got[n][m])[:k], want[n][:k], dtype)
    # TL: perturbations on the members' own fields; absent perturbations on everything else; all outputs wanted
    pert = {n: s.ens.put(rows) for n, rows in s.pert_host(names).items()}
    ref_o, got_o = {n: s.ens.nan() for n in NL_OUT}, {n: s.ens.nan() for n in NL_OUT}
    ref_i, got_i = {n: s.ens.nan() for n in NL_OUT}, {n: s.ens.nan() for n in NL_OUT}
    ens_tl("tl_step_ens" if step else "tl_ens", s.ens, s.ext, full, pert, s.eta, s.dt, ref_o, ref_i)
    enss_tl("tl_step_enss" if step else "tl_enss", s, part, pert, got_o, got_i, order)
    assert _lib.last_kernel() == ("cs2::tl_enss_step_kernel" if step else "cs2::tl_enss_kernel")
    compare(f"tl_enss {tag} out", got_o, ref_o, NL_OUT, nlev_of, dtype, same)
    compare(f"tl_enss {tag} out_i", got_i, ref_i, NL_OUT, nlev_of, dtype, same)
    # AD: forcing = the perturbed outputs, trajectory fluxes = the NL outputs of the TL launch; every adjoint wanted
    traj = {n: ref_o[n] for n in ("fplsl", "fplsn")}
    ref_a, got_a = {n: s.ens.nan() for n in names}, {n: s.ens.nan() for n in names}
    ens_ad("ad_step_ens" if step else "ad_ens", s.ens, s.ext, full, ref_i, s.eta, s.dt, traj, ref_a)
    enss_ad("ad_step_enss" if step else "ad_enss", s, part, ref_i, traj, got_a, order)
    assert _lib.last_kernel() == ("cs2::ad_enss_step_kernel" if step else "cs2::ad_enss_kernel")
    compare(f"ad_enss {tag}", got_a, ref_a, names, adjoint_nlev_of, dtype, same)
    return dict(nl=got, tl=got_i, ad=got_a)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shared_members_equal_materialised_members(gpu, shape, mask, step, dtype):
    """the six families on the DA mask, the all-shared mask (identical members: every member's results are bit-equal to
    member 0's) and mask 0, against the `*_ens_*` entries on materialised members and, for NL, the oracle"""
    assert tropopause_window(eta_family(NZ, dtype)["uniform"], NZ)[2] > 0
    _run(gpu, shape, dtype, mask, step)


def hold_to_oracle(s, step, tag):
    """NL outputs, perturbed outputs and adjoints of every member of the shared call `s` against the NumPy oracle run member
    by member on the materialised members - for the step chained with saturation's analytic derivative - at the tolerances
    tests/test_hip_ensemble.py holds the `*_ens_*` entries to: `assert_close` at its default for NL, 100 x for TL and AD.
    Perturbations: 1 % of every input of the member (shared inputs are perturbed per member too: perturbations are not
    shared); forcing: the oracle's perturbed outputs; trajectory fluxes: the launch's own NL outputs.  AD_TRAJ_FIX = 1.
    A member's `eta` is row m of `s.eta_host` when that has rows."""
    names = STEP_IN if step else NL_IN
    dtype, ext = s.dtype, s.ext
    part = {n: s.part[n] for n in names}
    want = []
    for m, fields in enumerate(s.members):
        eta = s.eta_host[m] if np.ndim(s.eta_host) == 2 else s.eta_host
        inc = plain = increments(fields, 0.01)
        _, g_t, g_ap, _ = saturation_derivative(fields["in_ap"], fields["in_t"], ext)
        if step:       # the qsat perturbation is saturation's derivative applied to those of t and ap
            inc = dict(inc, in_qsat_i=(g_t * inc["in_t_i"].astype(np.float64) + g_ap * inc["in_ap_i"].astype(np.float64)).astype(dtype))
        nl0 = run_oracle_nl(fields, eta, s.dt, ext)
        tl_i = run_oracle_tl(fields, inc, eta, s.dt, ext)[1]
        adj = dict(run_oracle_ad(fields, tl_i, eta, s.dt, ext, traj=nl0)[1])
        if step:
            adj["t"] = (adj["t"].astype(np.float64) + g_t * adj["qsat"].astype(np.float64)).astype(dtype)
            adj["ap"] = (adj["ap"].astype(np.float64) + g_ap * adj["qsat"].astype(np.float64)).astype(dtype)
        want.append(dict(nl=nl0, tl=tl_i, ad=adj, inc=plain))
    pert = {n: s.ens.put([w["inc"]["in_" + n + "_i"] for w in want]) for n in names}
    out, out_i = {n: s.ens.nan() for n in NL_OUT}, {n: s.ens.nan() for n in NL_OUT}
    enss_tl("tl_step_enss" if step else "tl_enss", s, part, pert, out, out_i, eta_ms=s.eta_ms)
    forcing = {n: s.ens.put([w["tl"][n] for w in want]) for n in NL_OUT}
    out_adj = {n: s.ens.nan() for n in names}
    enss_ad("ad_step_enss" if step else "ad_enss", s, part, forcing, {n: out[n] for n in ("fplsl", "fplsn")}, out_adj,
            eta_ms=s.eta_ms)
    nl_out = {n: s.ens.nan() for n in NL_OUT}
    enss_nl(s, part, nl_out, s.ens.nan() if step else None, eta_ms=s.eta_ms)
    failures = []
    for m, w in enumerate(want):
        for what, got, ref, lev, mul in (("nl", nl_out, w["nl"], nlev_of, 1.0), ("tl", out_i, w["tl"], nlev_of, 100.0),
                                        ("ad", out_adj, w["ad"], adjoint_nlev_of, 100.0)):
            for n in got:
                k = lev(n, NZ)
                try:
                    assert_close(f"{what}_enss {tag} vs oracle {n}[{m}]", from_device(got[n][m])[:k], ref[n][:k], dtype, rtol_mul=mul)
                except AssertionError as exc:
                    failures.append(str(exc))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shared_members_equal_the_oracle(gpu, shape, mask, step, dtype):
    """the six families on the three masks against the NumPy oracle, member by member on materialised members"""
    nmem, nx, window = shape
    hold_to_oracle(Shared(gpu, nmem, nx, window, dtype, mask, AD_TRAJ_FIX=1), step, f"{shape} mask={mask}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("stride", [NZ + 1, NZ + 8], ids=["packed", "padded"])
def test_per_member_eta_equals_the_oracle(gpu, stride, step, dtype):
    """three members on three vertical grids (one with an empty tropopause window): NL, TL and AD against the oracle run on
    each member's own grid"""
    fam = eta_family(NZ, dtype)
    grids = np.stack([fam["uniform"], fam["no_window_above"], fam["nps_eq_klo"]])
    hold_to_oracle(Shared(gpu, 3, 257, False, dtype, "da", grids, stride, AD_TRAJ_FIX=1), step, f"per-member eta {stride}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
def test_block_orders_agree_bit_for_bit(gpu, step, dtype):
    a = _run(gpu, (3, 257, False), dtype, "da", step, MEMBER_MAJOR)
    b = _run(gpu, (3, 257, False), dtype, "da", step, COLUMN_MAJOR)
    for fam in a:
        for n in a[fam]:
            assert np.array_equal(np.asarray(a[fam][n].cpu()), np.asarray(b[fam][n].cpu()), equal_nan=True), (fam, n)


def test_absent_wanted_and_forcing_names(gpu):
    """the 4D-Var shape of a call: forcing on the four tendencies only, adjoints of t, q, ql, qi only; TL wants two outputs
    and writes no NL outputs"""
    from derivative_support import STATE4, TND4

    dtype = np.float64
    s = Shared(gpu, 3, 257, False, dtype, "da")
    full, part = {n: s.full[n] for n in STEP_IN}, {n: s.part[n] for n in STEP_IN}
    pert = {n: s.ens.put(rows) for n, rows in s.pert_host(("t", "q")).items()}
    ref_o, ref_all = {n: s.ens.nan() for n in NL_OUT}, {n: s.ens.nan() for n in NL_OUT}
    ens_tl("tl_step_ens", s.ens, s.ext, full, pert, s.eta, s.dt, ref_o, ref_all)
    ref_i, got_i = {n: s.ens.nan() for n in ("tnd_t", "clc")}, {n: s.ens.nan() for n in ("tnd_t", "clc")}
    ens_tl("tl_step_ens", s.ens, s.ext, full, pert, s.eta, s.dt, None, ref_i)
    enss_tl("tl_step_enss", s, part, pert, None, got_i)
    compare("tl_step_enss sparse", got_i, ref_i, ("tnd_t", "clc"), nlev_of, dtype)
    forcing, traj = {n: ref_all[n] for n in TND4}, {n: ref_o[n] for n in ("fplsl", "fplsn")}
    ref_a, got_a = {n: s.ens.nan() for n in STATE4}, {n: s.ens.nan() for n in STATE4}
    ens_ad("ad_step_ens", s.ens, s.ext, full, forcing, s.eta, s.dt, traj, ref_a)
    enss_ad("ad_step_enss", s, part, forcing, traj, got_a)
    compare("ad_step_enss sparse", got_a, ref_a, STATE4, adjoint_nlev_of, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("stride", [NZ + 1, NZ + 8], ids=["packed", "padded"])
def test_per_member_eta(gpu, stride, dtype):
    """three members on three vertical grids - one with an empty tropopause window - against three single calls and the
    oracle; with eta_member_stride = 0 the result is the `*_ens_*` entry's"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    fam = eta_family(NZ, dtype)
    grids = [fam["uniform"], fam["no_window_above"], fam["nps_eq_klo"]]
    assert tropopause_window(grids[1], NZ)[2] == 0 and tropopause_window(grids[2], NZ)[2] > 0
    nmem, nx = 3, 257
    s = Shared(gpu, nmem, nx, False, dtype, "da", np.stack(grids), stride)
    assert s.eta_ms == stride
    part = {n: s.part[n] for n in STEP_IN}
    got, got_q = {n: s.ens.nan() for n in NL_OUT}, s.ens.nan()
    enss_nl(s, part, got, got_q, eta_ms=s.eta_ms)
    pert = {n: s.ens.put(rows) for n, rows in s.pert_host(STEP_IN).items()}
    got_o, got_i = {n: s.ens.nan() for n in NL_OUT}, {n: s.ens.nan() for n in NL_OUT}
    enss_tl("tl_step_enss", s, part, pert, got_o, got_i, eta_ms=s.eta_ms)
    got_a = {n: s.ens.nan() for n in STEP_IN}
    enss_ad("ad_step_enss", s, part, got_i, {n: got_o[n] for n in ("fplsl", "fplsn")}, got_a, eta_ms=s.eta_ms)
    for m in range(nmem):
        eta = torch.as_tensor(grids[m], device=gpu)
        st = {n: s.full[n][m] for n in STEP_IN}
        want = run_oracle_nl(s.members[m], grids[m], s.dt, s.ext)
        for n in NL_OUT:
            k = nlev_of(n, NZ)
            assert_close(f"per-member eta oracle {n}[{m}]", from_device(got[n][m])[:k], want[n][:k], dtype)
        nl, out_i = autodiff.tl_step(st, {n: f[m] for n, f in pert.items()}, eta, s.dt, s.ext, want=NL_OUT, write_nl=True)
        adj = autodiff.ad_step(st, out_i, eta, s.dt, s.ext, traj={n: nl[n] for n in ("fplsl", "fplsn")}, want=STEP_IN)
        one, one_q = {n: s.box.nan() for n in NL_OUT}, s.box.nan()      # the NL kernels' own single form, not the TL's NL outputs
        s.box.stencil("cloudsc2_nl_saturation", s.ext, eta, s.dt, **{"in_" + n: f for n, f in st.items()}, out_qsat=one_q,
                      **{"out_" + n: f for n, f in one.items()})
        for what, g, r, names, lev in (("nl", got, one, NL_OUT, nlev_of), ("tl nl", got_o, nl, NL_OUT, nlev_of),
                                       ("tl", got_i, out_i, NL_OUT, nlev_of), ("ad", got_a, adj, STEP_IN, adjoint_nlev_of)):
            for n in names:
                k = lev(n, NZ)
                torch.testing.assert_close(torch.as_tensor(from_device(g[n][m])[:k]), torch.as_tensor(from_device(r[n])[:k]),
                                           msg=lambda t: f"per-member eta {what} {n}[{m}]: {t}")
    # stride 0: one eta for all members - the ensemble entry's result
    ref, ref_q, one, one_q = {n: s.ens.nan() for n in NL_OUT}, s.ens.nan(), {n: s.ens.nan() for n in NL_OUT}, s.ens.nan()
    ens_nl(s.ens, s.ext, {n: s.full[n] for n in STEP_IN}, s.eta, s.dt, ref, ref_q)
    enss_nl(s, part, one, one_q, eta_ms=0)
    compare("eta stride 0", one, ref, NL_OUT, nlev_of, dtype)
