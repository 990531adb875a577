"""The ensemble forms of the cover kernels on the GPU (C ABI `cloudsc2_ad_evap_ens_*`, `cloudsc2_ad_evap_step_ens_*`;
kernels `cs2::ad_cover_ens_kernel`, `cs2::ad_cover_ens_step_kernel`).

Members: three states from DIFFERENT seeds (SEED + 100 + m, as tests/test_hip_ensemble.py), so a wrong member base cannot
cancel; `eta`, which an ensemble shares, is the one `nl_case` gives for SEED.  Every member is built by the case builder
of tests/test_evap_adjoint.py (`_make`, imported, with `nl_case` bound to the member's seed), so its CPU preconditions -
the evaporation block runs, somewhere all precipitation evaporates, some column has `out_covptot > 0` - hold for every
member.  Member m's forcing is that builder's, times 1 + m / 2.

Held, with no result element left out (level nz of a field that has nz levels is the documented padding level):
  * every member of every written adjoint and of `cover` against the single entry on that member alone: `assert_close`
    at its default for the dtype (bit-equality is printed, not asserted: hipcc contracts the level functions per kernel);
  * every member against the NumPy oracle adjoint (`oracle_adjoint`, for the step `total`) at MUL = 100, the multiplier
    tests/test_evap_adjoint.py holds these adjoints to;
  * results, `cover`, the gap between members (member_stride beyond a member's extent), level nz of `cover` and the pitch
    padding were NaN before the call: gap, level nz and padding still are, and no NaN reached a result;
  * a second call with cover_ready = 1: the same bits in every result, `cover` bit-unchanged.
The cases above run the kernels' <REG, FIX> = <true, true>; the last test holds the other three instantiations of each entry
and precision to the single entry (docs/TUNING_LOG.md 3.25 says why every instantiation is run)."""
import numpy as np
import pytest

import test_evap_adjoint as single
from derivative_support import SEED, STATE4, STEP_IN, Box, Ens
from helpers import NL_IN, NL_OUT, adjoint_nlev_of, assert_close, from_device, nl_case

pytestmark = pytest.mark.gpu
DT, MUL = single.DT, single.MUL
NMEM = 3
MASKS = {"full": (NL_OUT, None), "4dvar": (single.AD_OUT, STATE4)}     # forcing present, adjoints wanted (None: all)
L2, D1, BOTH = dict(LEVAPLS2=True), dict(LDRAIN1D=True), dict(LEVAPLS2=True, LDRAIN1D=True)
#: (nx, nz, window, gap, switches, mask) per precision and entry: nx 63 = a partly filled wave, 257 = a second workgroup per
#: member with one active lane; nz 137 and 8; each switch combination; both masks; a member stride beyond the extent always
CASES = [(63, 137, False, 1000, L2, "4dvar"), (257, 8, False, 24, D1, "full"), (257, 137, True, 512, BOTH, "4dvar"),
         (63, 8, False, 8, L2, "full")]
_cases = {}


def member_cases(nx, nz, dtype, sw):
    """per member the case of tests/test_evap_adjoint.py's builder on the member's own seed and the shared eta; once"""
    key = (nx, nz, np.dtype(dtype), tuple(sorted(sw.items())))
    if key not in _cases:
        eta = nl_case(nx, nz, dtype=dtype, seed=SEED)[1]
        rows = []
        for m in range(NMEM):
            def seeded(nx_, nz_, dtype=None, seed=None, _m=m):
                fields, _, dt = nl_case(nx_, nz_, dtype=dtype, seed=SEED + 100 + _m)
                return fields, eta, dt
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(single, "nl_case", seeded)
                c = single._make(nx, nz, dtype, sw)
            c["forcing"] = {n: (f * dtype(1.0 + 0.5 * m)).astype(dtype) for n, f in c["forcing"].items()}
            rows.append(c)
        _cases[key] = rows
    return _cases[key]


def raw_evap_ens(entry, ens, ext, state, forcing, eta, traj, out_adj, cover, ready):
    """a `cloudsc2_ad_evap*_ens` entry on member-major buffers the test supplies"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff

    box = ens.box
    m0 = lambda fields: {n: f[0] for n, f in fields.items()}  # noqa: E731
    p = autodiff._params(ext, box.nz)
    args = autodiff._ad_args(p, (box.nx, box.nz + 1, box.pitch), m0(state), m0(forcing),
                             autodiff._zero_line(torch.device(box.device), box.dt), eta, m0(traj), m0(out_adj), DT,
                             int(torch.cuda.current_stream().cuda_stream), cover=(cover[0].data_ptr(), int(ready)),
                             members=(ens.nmem, ens.ms))
    _lib.check(getattr(_lib.load(), f"cloudsc2_{entry}_{box.sfx}")(*args), entry)
    torch.cuda.synchronize()


def host(batch):
    """a member-major device batch -> [member][level][column]"""
    return np.stack([from_device(batch[m]) for m in range(batch.shape[0])])


def padding_untouched(ens):
    """the columns of every member-major allocation outside the window [col0, col0 + nx) still hold their NaN prefill"""
    b = ens.box
    for buf in ens.bufs:
        rows = buf[:, :b.dir_stride].view(ens.nmem, b.nz + 1, b.pitch)
        if not (bool(rows[:, :, :b.col0].isnan().all()) and bool(rows[:, :, b.col0 + b.nx:].isnan().all())):
            return False
    return True


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("nx,nz,window,gap,sw,mask", CASES,
                         ids=[f"{c[0]}x{c[1]}-{'+'.join(sorted(c[4]))}-{c[5]}" for c in CASES])
def test_every_member_equals_the_single_entry_and_the_oracle(gpu, nx, nz, window, gap, sw, mask, step, dtype):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    cases = member_cases(nx, nz, dtype, sw)
    ext = cases[0]["ext"]
    box = Box(nx, nz, dtype, gpu, window)
    ens = Ens(box, NMEM, gap)
    assert ens.ms > box.dir_stride
    eta = torch.as_tensor(cases[0]["eta"], device=gpu)
    names = STEP_IN if step else NL_IN
    have, want = MASKS[mask]
    want = names if want is None else want
    entry = "ad_evap_step" if step else "ad_evap"
    # the single entry on every member alone, on the NL kernel's own fluxes for that member
    rows, fluxes = [], []
    for c in cases:
        st = box.state(c["fields"], names)
        traj = box.nl_fluxes(box.state(c["fields"]), ext, eta, DT)
        adj, cov = {n: box.nan() for n in want}, box.nan()
        single.raw_evap(entry, box, ext, st, {n: box.put(c["forcing"][n]) for n in have}, eta, traj, adj, cov, 0)
        assert _lib.last_kernel() == ("cs2::ad_cover_step_kernel" if step else "cs2::ad_cover_kernel")
        ref = single.oracle_adjoint(c, traj, have)
        rows.append(dict(adj={n: from_device(adj[n]) for n in want}, cover=from_device(cov),
                         oracle=single.total(c, ref, nz, dtype) if step else ref))
        fluxes.append({n: from_device(traj[n]) for n in ("fplsl", "fplsn")})
    # all members in one launch, everything that is written NaN-prefilled
    state = {n: ens.put([c["fields"]["in_" + n] for c in cases]) for n in names}
    forcing = {n: ens.put([c["forcing"][n] for c in cases]) for n in have}
    traj = {n: ens.put([f[n] for f in fluxes]) for n in ("fplsl", "fplsn")}
    out_adj, cover = {n: ens.nan() for n in want}, ens.nan()
    raw_evap_ens(entry + "_ens", ens, ext, state, forcing, eta, traj, out_adj, cover, 0)
    assert _lib.last_kernel() == ("cs2::ad_cover_ens_step_kernel" if step else "cs2::ad_cover_ens_kernel")
    tag = f"{entry}_ens {nx}x{nz} {sorted(sw)} {mask} {np.dtype(dtype).name}"
    equal = True
    for m, row in enumerate(rows):
        cov = from_device(cover[m])
        assert np.isnan(cov[nz:]).all(), f"{tag}: level nz of cover[{m}] written"
        assert_close(f"{tag} cover[{m}]", cov[:nz], row["cover"][:nz], dtype)
        equal = equal and np.array_equal(cov[:nz], row["cover"][:nz])
        for n in want:
            k = adjoint_nlev_of(n, nz)
            a = from_device(out_adj[n][m])
            assert not np.isnan(a[:k]).any(), f"{tag} {n}[{m}]: NaN in a result"
            assert np.isnan(a[k:]).all(), f"{tag} {n}[{m}]: padding level written"
            assert_close(f"{tag} vs single out_{n}_i[{m}]", a[:k], row["adj"][n][:k], dtype)
            assert_close(f"{tag} vs oracle out_{n}_i[{m}]", a[:k], row["oracle"][n][:k], dtype, rtol_mul=MUL)
            equal = equal and np.array_equal(a[:k], row["adj"][n][:k])
    assert ens.gaps_untouched(), f"{tag}: the gap between members was written"
    assert padding_untouched(ens), f"{tag}: the pitch padding was written"
    print(f"{tag}: bit-equal to the single launches: {equal}")
    # cover_ready: the same bits from the field the first launch left, which stays as it is
    first = {n: host(f) for n, f in out_adj.items()}
    cov = host(cover)
    again = {n: ens.nan() for n in want}
    raw_evap_ens(entry + "_ens", ens, ext, state, forcing, eta, traj, again, cover, 1)
    assert np.array_equal(host(cover), cov, equal_nan=True), f"{tag}: cover_ready wrote cover"
    for n in want:
        assert np.array_equal(host(again[n]), first[n], equal_nan=True), f"{tag} {n}: cover_ready changed the result"
    assert ens.gaps_untouched() and padding_untouched(ens)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("flags", [dict(AD_TRAJ_FIX=0), dict(LREGCL=False), dict(LREGCL=False, AD_TRAJ_FIX=0)],
                         ids=["FIX0", "noLREGCL", "noLREGCL-FIX0"])
def test_the_other_instantiations_equal_the_single_entry(gpu, flags, step, dtype):
    """<REG, FIX> other than the <true, true> of the cases above: every member of every adjoint and of `cover` against the
    single entry (the oracle's trajectory adjoint is AD_TRAJ_FIX = 1: it is not the reference here)"""
    import torch

    nx, nz = 63, 137
    cases = member_cases(nx, nz, dtype, L2)
    ext = dict(cases[0]["ext"], **flags)
    box = Box(nx, nz, dtype, gpu, False)
    ens = Ens(box, NMEM, 64)
    eta = torch.as_tensor(cases[0]["eta"], device=gpu)
    names = STEP_IN if step else NL_IN
    entry = "ad_evap_step" if step else "ad_evap"
    rows, fluxes = [], []
    for c in cases:
        traj = box.nl_fluxes(box.state(c["fields"]), ext, eta, DT)
        adj, cov = {n: box.nan() for n in names}, box.nan()
        single.raw_evap(entry, box, ext, box.state(c["fields"], names), {n: box.put(c["forcing"][n]) for n in NL_OUT}, eta, traj,
                        adj, cov, 0)
        rows.append(dict({n: from_device(adj[n]) for n in names}, cover=from_device(cov)))
        fluxes.append({n: from_device(traj[n]) for n in ("fplsl", "fplsn")})
    state = {n: ens.put([c["fields"]["in_" + n] for c in cases]) for n in names}
    forcing = {n: ens.put([c["forcing"][n] for c in cases]) for n in NL_OUT}
    traj = {n: ens.put([f[n] for f in fluxes]) for n in ("fplsl", "fplsn")}
    out_adj, cover = {n: ens.nan() for n in names}, ens.nan()
    raw_evap_ens(entry + "_ens", ens, ext, state, forcing, eta, traj, out_adj, cover, 0)
    for m, row in enumerate(rows):
        assert_close(f"{entry}_ens {flags} cover[{m}]", from_device(cover[m])[:nz], row["cover"][:nz], dtype)
        for n in names:
            k = adjoint_nlev_of(n, nz)
            assert_close(f"{entry}_ens {flags} out_{n}_i[{m}]", from_device(out_adj[n][m])[:k], row[n][:k], dtype)
    assert ens.gaps_untouched() and padding_untouched(ens)


#: (nmem, nx) in fp64: the 65 536 columns of docs/TUNING_LOG.md 3.21 as 256 workgroups - one per CU at the fp64 kernels' one
#: wave per SIMD - and 196 608 columns as 768 workgroups, so that every CU runs several workgroups one after the other
LARGE = [(64, 1024), (8, 8192), (48, 4096)]


@pytest.mark.parametrize("step", [False, True], ids=["masked", "step"])
@pytest.mark.parametrize("nmem,nx", LARGE, ids=[f"{m}x{n}" for m, n in LARGE])
def test_a_full_chip_of_workgroups_equals_the_looped_single_launches(gpu, nmem, nx, step):
    """The shapes above against `nmem` single launches through the thin calls, fp64, full mask (every forcing, every
    adjoint): `assert_close` at its default per member, adjoint and `cover`.  The small cases above run at most six
    workgroups; docs/TUNING_LOG.md 3.25 says why `ad_cover_ens_kernel<double>` in particular is held at this size."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.synthetic import eta_levels, make_state

    nz, dtype = 137, np.float64
    ext = dict(default_externals(), NLEV=nz, AD_TRAJ_FIX=1, LEVAPLS2=True)
    new = lambda: storage.zeros_batched(nmem, nx, nz, dtype, gpu)  # noqa: E731
    s = make_state(nmem * nx, nz, dtype=dtype, device=gpu, seed=SEED)
    state = {n: new() for n in STEP_IN}
    for n in STEP_IN:      # member m = columns m * nx ... of one synthetic state
        state[n].permute(0, 3, 2, 1).squeeze(2).copy_(torch.as_tensor(s["f_" + n], device=gpu).view(nz + 1, nmem, nx).permute(1, 0, 2))
    del s
    eta = torch.as_tensor(eta_levels(nz, seed=SEED, dtype=dtype), device=gpu)
    with torch.no_grad():
        nl = autodiff.cloudsc2_step_ensemble(state, eta, DT, ext)
    traj = {n: nl[n] for n in ("fplsl", "fplsn")}
    if not step:
        state["qsat"] = nl["qsat"]
    names = STEP_IN if step else NL_IN
    gen = torch.Generator(device=gpu).manual_seed(11)
    forcing = {n: new() for n in NL_OUT}
    for n, f in forcing.items():
        f.copy_(torch.randn(f.shape, generator=gen, dtype=f.dtype, device=gpu))
        f[..., nz] = 0.0
    ens, one = (autodiff.ad_step_evap_ens, autodiff.ad_step_evap) if step else (autodiff.ad_masked_evap_ens, autodiff.ad_masked_evap)
    cover = new()
    got = ens(state, forcing, eta, DT, ext, traj=traj, want=names, cover=cover)
    assert _lib.last_kernel() == ("cs2::ad_cover_ens_step_kernel" if step else "cs2::ad_cover_ens_kernel")
    assert bool((cover > 0).any()) and not any(bool(f.isnan().any()) for f in got.values())
    member = lambda fields, m: {n: f[m] for n, f in fields.items()}  # noqa: E731
    equal = True
    for m in range(nmem):
        cov = storage.zeros(nx, nz, dtype, gpu)
        ref = one(member(state, m), member(forcing, m), eta, DT, ext, traj=member(traj, m), want=names, cover=cov)
        assert_close(f"cover[{m}]", from_device(cover[m])[:nz], from_device(cov)[:nz], dtype)
        for n in names:
            k = adjoint_nlev_of(n, nz)
            a, b = from_device(got[n][m])[:k], from_device(ref[n])[:k]
            assert_close(f"{nmem}x{nx} {'step' if step else 'masked'} out_{n}_i[{m}]", a, b, dtype)
            equal = equal and np.array_equal(a, b)
    print(f"{nmem}x{nx} fp64 {'step' if step else 'masked'}: bit-equal to the looped single launches: {equal}")
