"""The trajectory adjoints WITH the evaporation block (`cloudsc2_ad_evap_*`, `_step_*`, `_multi_*`, `_multi_step_*`;
`autodiff.ad_masked_evap` ... and `autodiff.EVAP_ADJOINT`) on the GPU.

Inputs: `nl_case(nx, nz, dtype, seed=SEED)` under `LEVAPLS2=True` at dt = 60 s, the shapes of `derivative_support.SHAPES`.
Every test first asserts on the CPU (the oracle's branch counters) that the evaporation block runs and, for nx >= 63, that
somewhere all precipitation evaporates, and that some column has `out_covptot > 0`: without these the cover would not matter.

Tolerance: `helpers.assert_close` with the multiplier 100 that `grid_support.hold_dense` gives the dense adjoint, in fp64 and
fp32, against the oracle (`run_oracle_ad(..., traj=<the NL kernel's fluxes>)`, AD_TRAJ_FIX = 1, in the working precision)
and against the dense `cloudsc2_ad` kernel with explicit zero fields.

Every launch is also held to its window: the columns of the underlying allocations outside [col0, col0 + nx) - the guard
columns of the window shape, the pitch padding of the others - keep their NaN prefill, in the results and in `cover`."""
import ctypes

import numpy as np
import pytest

from derivative_support import SEED, SHAPES, STATE4, STEP_IN, TND4, Box, compare_directions
from helpers import NL_IN, NL_OUT, adjoint_nlev_of, assert_close, externals, from_device, nl_case, nlev_of, run_oracle_ad
from saturation_oracle import saturation_derivative

pytestmark = pytest.mark.gpu
DT = 60.0
MUL = 100.0      # hold_dense's multiplier for the adjoints of the dense kernel
_host = {}


def _make(nx, nz, dtype, sw):
    from helpers import oracle

    ext = externals(NLEV=nz, AD_TRAJ_FIX=1, **sw)
    fields, eta, _ = nl_case(nx, nz, dtype=dtype, seed=SEED)
    F = dict(fields)
    for n in NL_OUT:
        F["out_" + n] = np.zeros_like(fields["in_ap"])
    counts = {}
    oracle.cloudsc2_nl(F, eta, DT, ext, branch_counts=counts)
    assert counts.get("evaporation", 0) > 0, counts
    if nx >= 63:
        assert counts.get("evaporation_of_all_precip", 0) > 0, counts
    assert (F["out_covptot"][:nz] > 0).any(axis=0).any()
    rng = np.random.default_rng(11)
    forcing = {n: np.zeros_like(fields["in_ap"]) for n in NL_OUT}
    for n in NL_OUT:
        k = nlev_of(n, nz)
        forcing[n][:k] = rng.standard_normal((k, nx)).astype(dtype)
    return dict(fields=fields, eta=eta, forcing=forcing, ext=ext)


def case(nx, nz, dtype, **sw):
    sw = sw or dict(LEVAPLS2=True)
    key = (nx, nz, np.dtype(dtype), tuple(sorted(sw.items())))
    if key not in _host:
        _host[key] = _make(nx, nz, dtype, sw)
    return _host[key]


def raw_evap(entry, box, ext, state, forcing, eta, traj, out_adj, cover, ready, ndir=None):
    """a `cloudsc2_ad_evap*` entry on buffers the test supplies"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    p = autodiff._params(ext, box.nz)
    d0 = (lambda f: f) if ndir is None else (lambda f: {n: t[0] for n, t in f.items()})
    head = (ctypes.byref(p), box.nx, box.nz, box.pitch, autodiff._ptrs(state, NL_IN), autodiff._ptrs(d0(forcing), NL_OUT),
            autodiff._zero_line(torch.device(box.device), box.dt).data_ptr(), eta.data_ptr(), traj["fplsl"].data_ptr(),
            traj["fplsn"].data_ptr(), autodiff._ptrs(d0(out_adj), NL_IN), DT)
    stream = int(torch.cuda.current_stream().cuda_stream)
    park = (cover.data_ptr(), int(ready))
    args = head + park + (stream,) if ndir is None else head + (stream, ndir, box.dir_stride, box.dir_stride) + park
    _lib.check(getattr(_lib.load(), f"cloudsc2_{entry}_{box.sfx}")(*args), entry)
    torch.cuda.synchronize()


def setup(gpu, nx, nz, window, dtype, **sw):
    import torch

    c = case(nx, nz, dtype, **sw)
    box = Box(nx, nz, dtype, gpu, window)
    state = box.state(c["fields"])
    eta = torch.as_tensor(c["eta"], device=gpu)
    traj = box.nl_fluxes(state, c["ext"], eta, DT)
    forcing = {n: box.put(c["forcing"][n]) for n in NL_OUT}
    return c, box, state, eta, traj, forcing


def dense(box, c, state, forcing, eta):
    """`cloudsc2_ad` with explicit zero fields for the absent forcing"""
    full = {n: forcing[n] if n in forcing else box.zeros() for n in NL_OUT}
    nl, adj = {n: box.nan() for n in NL_OUT}, {n: box.nan() for n in NL_IN}
    box.stencil("cloudsc2_ad", c["ext"], eta, DT, **{"in_" + n: f for n, f in state.items()},
                **{"in_" + n + "_i": f for n, f in full.items()}, **{"out_" + n: f for n, f in nl.items()},
                **{"out_" + n + "_i": f for n, f in adj.items()})
    return {n: from_device(f) for n, f in adj.items()}


def check(what, got, want, names, nz, dtype):
    for n in names:
        k = adjoint_nlev_of(n, nz)
        a = from_device(got[n]) if not isinstance(got[n], np.ndarray) else got[n]
        assert np.isnan(a[k:]).all(), f"{what} {n}: padding level written"
        assert_close(f"{what} out_{n}_i", a[:k], want[n][:k], dtype, rtol_mul=MUL)


def guards_untouched(box, *groups):
    """every column of the underlying allocations outside the call's window [col0, col0 + nx) still holds its NaN prefill:
    the guard columns of a window shape, the pitch padding of a dense one - of results, `cover` and inputs alike"""
    for group in groups:
        for n, f in (group.items() if isinstance(group, dict) else [("cover", group)]):
            base = f._base
            assert base is not None and base.shape[-1] == box.pitch, (n, None if base is None else tuple(base.shape))
            assert bool(base[..., :box.col0].isnan().all()), f"{n}: columns in front of the window written"
            assert bool(base[..., box.col0 + box.nx:].isnan().all()), f"{n}: columns behind the window written"


def oracle_adjoint(c, traj, have=NL_OUT, forcing=None):
    """the oracle's adjoint for the forcing on `have` (zero elsewhere), fluxes per level from the NL kernel's own outputs"""
    forcing = c["forcing"] if forcing is None else forcing
    host_f = {n: (forcing[n] if n in have else np.zeros_like(c["forcing"][n])) for n in NL_OUT}
    nl0 = {n: from_device(traj[n]) for n in ("fplsl", "fplsn")}
    return run_oracle_ad(c["fields"], host_f, c["eta"], DT, c["ext"], traj=nl0)[1]


MASKS = {"full": (NL_OUT, NL_IN), "4dvar": (TND4, STATE4)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx,nz,window", SHAPES)
@pytest.mark.parametrize("mask", ["full", "4dvar"])
def test_single_entry_matches_the_dense_kernel_and_the_oracle(gpu, nx, nz, window, dtype, mask):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    c, box, state, eta, traj, forcing = setup(gpu, nx, nz, window, dtype)
    have, want = MASKS[mask]
    f = {n: forcing[n] for n in have}
    adj, cover = {n: box.nan() for n in want}, box.nan()
    raw_evap("ad_evap", box, c["ext"], state, f, eta, traj, adj, cover, 0)
    assert _lib.last_kernel() == "cs2::ad_cover_kernel"
    cov = from_device(cover)
    assert not np.isnan(cov[:nz]).any() and np.isnan(cov[nz:]).all()          # level nz of `cover` is never touched
    assert (cov[:nz] > 0).any()
    guards_untouched(box, adj, cover)
    check(f"evap[{mask}] vs oracle", adj, oracle_adjoint(c, traj, have), want, nz, dtype)
    check(f"evap[{mask}] vs dense", adj, dense(box, c, state, f, eta), want, nz, dtype)
    # cover_ready: a second launch on the field the first left gives the same bits and leaves the field alone
    adj2 = {n: box.nan() for n in want}
    raw_evap("ad_evap", box, c["ext"], state, f, eta, traj, adj2, cover, 1)
    assert np.array_equal(from_device(cover), cov, equal_nan=True)
    guards_untouched(box, adj2, cover, state, f, traj)
    for n in want:
        assert np.array_equal(from_device(adj2[n]), from_device(adj[n]), equal_nan=True), n


@pytest.mark.parametrize("sw", [dict(LEVAPLS2=True, LREGCL=False), dict(LDRAIN1D=True)], ids=["noreg", "ldrain1d"])
def test_other_switches(gpu, sw):
    nx, nz, dtype = 200, 137, np.float64
    c, box, state, eta, traj, forcing = setup(gpu, nx, nz, False, dtype, **sw)
    adj, cover = {n: box.nan() for n in NL_IN}, box.nan()
    raw_evap("ad_evap", box, c["ext"], state, forcing, eta, traj, adj, cover, 0)
    guards_untouched(box, adj, cover)
    check(f"evap{sw} vs oracle", adj, oracle_adjoint(c, traj), NL_IN, nz, dtype)
    check(f"evap{sw} vs dense", adj, dense(box, c, state, forcing, eta), NL_IN, nz, dtype)


def total(c, adj, nz, dtype):
    """the oracle adjoint of cloudsc2 -> that of the step: saturation's derivative folded into t and ap (as
    tests/test_step_grad.py does for the step without the evaporation block)"""
    _, g_t, g_ap, _ = saturation_derivative(c["fields"]["in_ap"], c["fields"]["in_t"], c["ext"])
    ref = {n: adj[n].astype(np.float64) for n in STEP_IN}
    ref["t"][:nz] += g_t[:nz] * adj["qsat"][:nz]
    ref["ap"][:nz] += g_ap[:nz] * adj["qsat"][:nz]
    return {n: f.astype(dtype) for n, f in ref.items()}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx,nz,window", [SHAPES[2], SHAPES[3], SHAPES[4]])
def test_step_entry_is_the_composition(gpu, nx, nz, window, dtype):
    """`cloudsc2_ad_evap_step` against the oracle adjoint with saturation's derivative folded into t and ap"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    c, box, state, eta, traj, forcing = setup(gpu, nx, nz, window, dtype)
    got, cover = {n: box.nan() for n in STEP_IN}, box.nan()
    raw_evap("ad_evap_step", box, c["ext"], {n: state[n] for n in STEP_IN}, forcing, eta, traj, got, cover, 0)
    assert _lib.last_kernel() == "cs2::ad_cover_step_kernel"
    guards_untouched(box, got, cover)
    check("evap step", got, total(c, oracle_adjoint(c, traj), nz, dtype), STEP_IN, nz, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("step", [False, True], ids=["multi", "multi_step"])
@pytest.mark.parametrize("shape,ndir", [(SHAPES[2], 1), (SHAPES[2], 3), (SHAPES[2], 8), (SHAPES[3], 3)],
                         ids=["200-1", "200-3", "200-8", "window333-3"])
def test_multi_entries_match_the_single_entry_direction_by_direction(gpu, shape, ndir, dtype, step):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    nx, nz, window = shape
    c, box, state, eta, traj, forcing = setup(gpu, nx, nz, window, dtype)
    names = STEP_IN if step else NL_IN
    st = {n: state[n] for n in names}
    rng = np.random.default_rng(17)
    host = [{n: c["forcing"][n] * dtype(rng.uniform(0.5, 1.5)) for n in NL_OUT} for _ in range(ndir)]
    batch = {n: box.batch([h[n] for h in host], ndir + 1) for n in NL_OUT}
    got, cover = {n: box.nan(ndir + 1) for n in names}, box.nan()
    entry = "ad_evap_multi_step" if step else "ad_evap_multi"
    raw_evap(entry, box, c["ext"], st, batch, eta, traj, got, cover, 0, ndir)
    assert _lib.last_kernel() == ("cs2::ad_cover_dirs_step_kernel" if step else "cs2::ad_cover_dirs_kernel")
    guards_untouched(box, got, cover)
    rows = []
    for d in range(ndir):
        one, cov1 = {n: box.nan() for n in names}, box.nan()
        raw_evap("ad_evap_step" if step else "ad_evap", box, c["ext"], st, {n: batch[n][d] for n in NL_OUT}, eta, traj, one,
                 cov1, 0)
        rows.append({n: from_device(one[n]) for n in names})
    assert np.array_equal(from_device(cov1), from_device(cover), equal_nan=True)      # the cover does not depend on the forcing
    compare_directions(entry, got, rows, names, nz, dtype, ndir, levels=adjoint_nlev_of)
    # cover_ready on the field the first launch left: the same bits in every direction, the field itself unchanged
    cov = from_device(cover)
    again = {n: box.nan(ndir + 1) for n in names}
    raw_evap(entry, box, c["ext"], st, batch, eta, traj, again, cover, 1, ndir)
    assert np.array_equal(from_device(cover), cov, equal_nan=True)
    guards_untouched(box, again, cover)
    for n in names:
        for d in range(ndir + 1):
            assert np.array_equal(from_device(again[n][d]), from_device(got[n][d]), equal_nan=True), (n, d)


AD_OUT = TND4 + ("covptot",)      # the outputs the differentiated functional weighs


def _autodiff_run(gpu, fn, names, dtype, nx=200, nz=137):
    """backward of sum_n (out[n] * W[n]).sum() over AD_OUT for the case's state -> gradients of STATE4, the kernel the
    backward reported, the forward's own fluxes, the case"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    c = case(nx, nz, dtype)                      # asserts the CPU preconditions
    box = Box(nx, nz, dtype, gpu, False)
    state = box.state(c["fields"], names)
    for n in STATE4:
        state[n].requires_grad_(True)
    eta = torch.as_tensor(c["eta"], device=gpu)
    out = fn(state, eta, DT, c["ext"])
    sum((out[n] * box.put(c["forcing"][n])).sum() for n in AD_OUT).backward()
    kernel = _lib.last_kernel()
    traj = {n: out[n].detach() for n in ("fplsl", "fplsn")}
    return {n: from_device(state[n].grad) for n in STATE4}, kernel, traj, c


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("step", [False, True], ids=["cloudsc2", "cloudsc2_step"])
def test_autodiff_trajectory_mode(gpu, dtype, step, monkeypatch):
    """`EVAP_ADJOINT = "trajectory"`: `backward` runs the new kernels and agrees with the oracle; with the default value the
    dense path runs as before (`cloudsc2_ad`; for the step `saturation_ad` behind it)"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    nz = 137
    fn, names = (autodiff.cloudsc2_step, STEP_IN) if step else (autodiff.cloudsc2, NL_IN)
    assert autodiff.EVAP_ADJOINT == "dense"
    _, kernel, _, _ = _autodiff_run(gpu, fn, names, dtype)
    assert kernel == ("cs2::saturation_ad_kernel" if step else "cs2::ad_kernel"), kernel
    monkeypatch.setattr(autodiff, "EVAP_ADJOINT", "trajectory")
    got, kernel, traj, c = _autodiff_run(gpu, fn, names, dtype)
    assert kernel == ("cs2::ad_cover_step_kernel" if step else "cs2::ad_cover_kernel"), kernel
    want = oracle_adjoint(c, traj, AD_OUT)
    if step:
        want = total(c, want, nz, dtype)
    for n in STATE4:
        assert_close(f"{fn.__name__} grad {n}", got[n][:nz], want[n][:nz], dtype, rtol_mul=MUL)


def test_ensembles_loop_over_their_members_in_trajectory_mode(gpu, monkeypatch):
    """`cloudsc2_ensemble` and `vmap` over the state with the switches: no ensemble form of the cover kernels - every member is
    one `ad_cover_kernel` launch, and its gradient is the single call's"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    dtype, nx, nz = np.float64, 63, 137
    monkeypatch.setattr(autodiff, "EVAP_ADJOINT", "trajectory")
    single, kernel, _, c = _autodiff_run(gpu, autodiff.cloudsc2, NL_IN, dtype, nx, nz)
    assert kernel == "cs2::ad_cover_kernel"
    box = Box(nx, nz, dtype, gpu, False)
    eta = torch.as_tensor(c["eta"], device=gpu)
    w = {n: box.put(c["forcing"][n]) for n in AD_OUT}
    scale = (1.0, 0.5)          # member 1 weighs the functional half: its gradient is half member 0's, exactly

    def members():
        st = {n: torch.stack([f, f]) for n, f in box.state(c["fields"]).items()}
        for n in STATE4:
            st[n].requires_grad_(True)
        return st

    st = members()
    out = autodiff.cloudsc2_ensemble(st, eta, DT, c["ext"])
    sum((out[n][m] * w[n]).sum() * scale[m] for n in AD_OUT for m in range(2)).backward()
    assert _lib.last_kernel() == "cs2::ad_cover_kernel"
    for n in STATE4:
        for m in range(2):
            assert_close(f"ensemble member {m} grad {n}", from_device(st[n].grad[m])[:nz], scale[m] * single[n][:nz], dtype)
    st = members()
    out = torch.func.vmap(lambda s: autodiff.cloudsc2(s, eta, DT, c["ext"]))(st)
    sum((out[n][m] * w[n]).sum() * scale[m] for n in AD_OUT for m in range(2)).backward()
    assert _lib.last_kernel() == "cs2::ad_cover_kernel"
    for n in STATE4:
        for m in range(2):
            assert_close(f"vmap member {m} grad {n}", from_device(st[n].grad[m])[:nz], scale[m] * single[n][:nz], dtype)


def test_jacrev_runs_the_dirs_kernel_and_equals_the_looped_singles(gpu, monkeypatch):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    dtype, nx, nz = np.float64, 63, 137
    c, box, state, eta, traj, _ = setup(gpu, nx, nz, False, dtype)
    rng = np.random.default_rng(3)
    cot = {n: box.batch([rng.standard_normal((nz + 1, nx)) for _ in range(10)]) for n in TND4}
    for n in TND4:
        cot[n][:, :, :, nz] = 0.0
    got = autodiff.ad_multi_evap(state, cot, eta, DT, c["ext"], traj=traj, want=STATE4, width=8)
    assert _lib.last_kernel() == "cs2::ad_cover_dirs_kernel"
    for d in range(10):
        one = autodiff.ad_masked_evap(state, {n: cot[n][d] for n in TND4}, eta, DT, c["ext"], traj=traj, want=STATE4)
        for n in STATE4:
            assert_close(f"chunked ad_multi_evap[{d}] {n}", from_device(got[n][d])[:nz], from_device(one[n])[:nz], dtype)
    # the same through torch.func.jacrev of a ten-component functional
    monkeypatch.setattr(autodiff, "EVAP_ADJOINT", "trajectory")
    w = torch.stack([cot["tnd_t"][d] for d in range(10)])

    def f(t):
        out = autodiff.cloudsc2(dict(state, t=t), eta, DT, c["ext"])
        return (w * out["tnd_t"].unsqueeze(0)).sum(dim=(1, 2, 3))

    jac = torch.func.jacrev(f)(state["t"])
    assert _lib.last_kernel() == "cs2::ad_cover_dirs_kernel"
    ref = autodiff.ad_multi_evap(state, {"tnd_t": w}, eta, DT, c["ext"], traj=traj, want=("t",), width=1)["t"]
    for d in range(10):
        assert_close(f"jacrev row {d}", from_device(jac[d])[:nz], from_device(ref[d])[:nz], dtype)
