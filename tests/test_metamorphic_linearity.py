"""Exact homogeneity of every TL and AD entry: scaling every perturbation (TL) or forcing (AD) by s = +-2^k scales every
intermediate of a linear map exactly, so `out(s d) == s out(d)` bit for bit - whatever the FMA contraction, because the same
binary runs both times.  A kernel that keeps a constant term, clamps a perturbation, branches on one, or mixes a trajectory
value into a perturbation slot breaks it.  No tolerance: tests/metamorphic_support.py `assert_bitwise`.

Entries (`metamorphic_support.DERIVATIVES`): the dense `cloudsc2_tl`, `cloudsc2_tl_incremented` (the scaled quantity is `f`),
`cloudsc2_ad`, `cloudsc2_ad_from_trajectory`; `tl_masked`, `tl_step`, `tl_multi`, `tl_multi_step`; `ad_masked`, `ad_step`,
`ad_multi`, `ad_multi_step`; the `*_ens_*` and `*_enss_*` TL and AD entries; `ad_evap`, `ad_evap_step`, their `_multi` and
`_ens` forms; `ad_multi_ens`, `ad_multi_step_ens`; `saturation_tl`, `saturation_ad` and its `accumulate` form (where what is
accumulated into scales too).  Shapes and externals: `metamorphic_support.configurations`."""
import numpy as np
import pytest

from helpers import NL_IN, NL_OUT, oracle, run_oracle_ad, run_oracle_tl
from metamorphic_support import (BASE, D1, DERIVATIVES, FIX, L2, NDIR, NMEM, NOREG, NXS, NZ, SCALES, assert_bitwise, configurations,
                                 copies_of, device_case, host_case, is_evap, label, scaled, times, zeroed)

DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
#: every set of externals a GPU test of this file or of tests/test_metamorphic_locality.py runs under
ALL_FLAGS = [BASE, NOREG, FIX, L2, D1, dict(L2, **NOREG), dict(L2, **FIX)]
DIR_FACTORS = (1.0,) + SCALES
MEMBER_FACTORS = (1.0, 8.0, -1024.0)


def _oracle(c, m, d, s, traj):
    """the oracle's TL on `s` times perturbation (m, d) and its AD on `s` times forcing (m, d), as result dicts"""
    T = c.dtype.type
    fields = {"in_" + n: c.data[("state", m, 0, n)] for n in NL_IN}
    pert = {"in_" + n + "_i": c.data[("tl", m, d, n)] * T(s) for n in NL_IN}
    nl, tl = run_oracle_tl(fields, pert, c.eta, c.dt, c.ext)
    forcing = {n: c.data[("ad", m, d, n)] * T(s) for n in NL_OUT}
    ad = run_oracle_ad(fields, forcing, c.eta, c.dt, c.ext, traj={n: c.data[("traj", m, 0, n)] for n in ("fplsl", "fplsn")} if traj else None)[1]
    res = {("nl", m, d, n): (a, NZ + 1) for n, a in nl.items()}
    res.update({("out", m, d, "tl " + n): (a, NZ + 1) for n, a in tl.items()})
    res.update({("out", m, d, "ad " + n): (a, NZ + 1) for n, a in ad.items()})
    return res


@DTYPES
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=lambda f: "+".join(sorted(f)) or "default")
@pytest.mark.parametrize("nx", NXS)
def test_the_oracle_is_exactly_homogeneous(nx, flags, dtype):
    """The precondition of the GPU tests, on the CPU: the NumPy oracle, in the same dtype on the same inputs, satisfies every
    identity they assert with 0 mismatches and no subnormal exclusion - `cloudsc2_tl` and `cloudsc2_ad` (with the trajectory
    fluxes the masked adjoints read; for member 0 also with its own forward sweep) for every scale of `SCALES`, for every
    member on direction 0 and every direction of member 0, and exactly zero results for zero perturbations / forcings.
    With an evaporation switch the evaporation block runs in the case.  No input had to be dropped: 0 of 28 cases.

    Why the float32 oracle with LEVAPLS2 is NOT bit-homogeneous at `nl_case(66, 137)` with 1 % increments: OVERFLOW, neither
    underflow nor a branch on a perturbation.  The perturbed outputs of `cloudsc2_tl` themselves leave the float32 range
    there: the largest finite one is 3.19e38 (the format ends at 3.40e38) and 88 of the 91 080 are already inf or NaN at
    s = 1; `cloudsc2_ad` forced with them returns 19 924 non-finite values of 145 728.  Under s = 8 more values overflow (93
    TL and 24 687 AD points differ from 8 times the unscaled ones), and NaN never equals NaN.  Counting only points where
    both results are finite there are 0 mismatches for TL and for AD, and scaling DOWN first does not cure it while scaling up
    makes it worse (2^20: 861, 2^40: 2 642, 2^60: 5 270 TL points), which is what overflow does and underflow does not.
    So the oracle has no perturbation-dependent branch there and the HIP adjoint shares none; the GPU tests stay at nz = 12,
    where the smallest and largest magnitudes are far inside both formats."""
    c = host_case(nx, dtype, flags)
    if is_evap(flags):
        counts = {}
        F = {"in_" + n: c.data[("state", 0, 0, n)] for n in NL_IN}
        F.update({"out_" + n: np.zeros((NZ + 1, nx), dtype) for n in NL_OUT})
        oracle.cloudsc2_nl(F, c.eta, c.dt, c.ext, branch_counts=counts)
        assert counts.get("evaporation", 0) > 0, counts
    for m, d in [(m, 0) for m in range(NMEM)] + [(0, d) for d in range(1, NDIR)]:
        for traj in (True, False) if (m, d) == (0, 0) else (True,):
            base = _oracle(c, m, d, 1.0, traj)
            for s in SCALES:
                assert_bitwise(f"oracle nx={nx} s={s} traj={traj}", _oracle(c, m, d, s, traj), times(base, s))
            zero = _oracle(c, m, d, 0.0, traj)
            for key, (a, _) in zero.items():
                if key[0] == "out":
                    assert not a.any(), key


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", DERIVATIVES, ids=lambda e: e.name)
def test_scaling_the_input_scales_the_result_exactly(gpu, entry, dtype):
    """`out(s d) == s out(d)` bitwise for every s of `SCALES`; the NL outputs a launch also writes (and `cover`) are
    bit-identical between the runs; all-zero perturbations / forcings give exactly zero.

    Found by this test: `tl_ens` in float32 under LEVAPLS2 at nx = 130, s = 1/8, member 2 gave `fhpsl` and `fplsl` 1 - 2 ulp
    off at level 10, column 69 (fplsl got -0x1.5e9288p-64, want -0x1.5e928cp-64; normal numbers, so outside the exclusion).
    `evaporated_i` (csrc/cloudsc2_common.hpp) formed `dpr * f * prtot_i * rpr * rpr` from the left: with a residual rain flux of
    5.6e-17 beside a snow flux of 1.4e-10 and prtot_i = 4.7e-12 the product of the first three is ~1e-38, subnormal once
    scaled by 1/8, before rpr^2 brings it back to 1e-19.  It now multiplies the ratios `dpr * rpr` and `f * rpr`."""
    for nx, window, flags in configurations(entry):
        c = host_case(nx, dtype, flags)
        what = f"{entry.name} {label(nx, window, flags)} {np.dtype(dtype).name}"
        base = entry.run(device_case(gpu, entry, c, window))
        assert any(a[:k].any() for (g, *_), (a, k) in base.items() if g == "out"), f"{what}: every result is zero"
        for s in SCALES:
            got = entry.run(device_case(gpu, entry, scaled(c, s), window))
            assert_bitwise(f"{what} s={s}", got, times(base, s), rescaled=(base, s))
        zero = entry.run(device_case(gpu, entry, zeroed(c), window))
        assert_bitwise(f"{what} zero input", zero, times(base, 0.0))


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", [e for e in DERIVATIVES if e.dirs or e.members], ids=lambda e: e.name)
def test_a_scale_stays_in_its_direction_and_member(gpu, entry, dtype):
    """the same in ONE launch: directions 1 .. 4 are the scaled copies of direction 0, members 1 and 2 have member 0's state
    and scaled copies of its forcing / perturbation - a direction's or member's scale cannot bleed into another's.

    The unscaled run is the same launch with UNSCALED copies in every slot, so direction d is held to direction d: the slots
    of one launch need not agree bit for bit among themselves.  Measured on an MI355X: `tl_dirs_kernel<float>` and both
    `tl_dirs_step_kernel`s give direction 0 and directions 1 .. 4 of five identical copies results that differ in the last
    1 - 4 ulp (nx = 130, default externals: fhpsl 12, fhpsn 82 - 103, fplsl 15, clc 40 of ~1 600 points; directions 1 .. 4
    agree among themselves); every other multi-direction and ensemble entry agrees across its slots.  Direction 0 is the
    iteration of the kernel's direction loop that also stores the NL outputs (`d == 0 ? want : want & ~kTLWantNL`), which the
    compiler may peel and contract on its own, as it contracts the level functions per kernel.  Whether the slots agree is
    printed, not asserted."""
    for nx, window, flags in configurations(entry):
        c = host_case(nx, dtype, flags)
        what = f"{entry.name} one launch {label(nx, window, flags)} {np.dtype(dtype).name}"
        fd = DIR_FACTORS if entry.dirs else (1.0,) * NDIR
        fm = MEMBER_FACTORS if entry.members else (1.0,) * NMEM
        ones = (1.0,) * max(NDIR, NMEM)

        def copies(fd, fm):
            c2 = copies_of(c, fd[:NDIR]) if entry.dirs else c
            return copies_of(c2, fm[:NMEM], members=True) if entry.members else c2
        same = entry.run(device_case(gpu, entry, copies(ones, ones), window))
        got = entry.run(device_case(gpu, entry, copies(fd, fm), window))
        factor = lambda k: fm[k[1]] * fd[k[2]]  # noqa: E731
        want = {k: ((a * a.dtype.type(factor(k)), lv) if k[0] == "out" else (a, lv)) for k, (a, lv) in same.items()}
        assert_bitwise(what, got, want, rescaled=(same, factor))
        agree = all(np.array_equal(a[:lv], same[(k[0], 0, 0, k[3])][0][:lv]) for k, (a, lv) in same.items())
        print(f"{what}: identical copies agree across slots: {agree}")


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", [e for e in DERIVATIVES if e.masked], ids=lambda e: e.name)
def test_a_zero_field_equals_an_absent_one(gpu, entry, dtype):
    """an all-zero perturbation / forcing passed as a field equals the same passed as absent (NULL: the zero line), bitwise"""
    keep = ("t",) if entry.name == "saturation_tl" else ("t", "q") if entry.kind == "tl" else ("tnd_t", "tnd_q")
    for nx, window, flags in configurations(entry):
        c = zeroed(host_case(nx, dtype, flags), keep)
        what = f"{entry.name} absent {label(nx, window, flags)} {np.dtype(dtype).name}"
        field = entry.run(device_case(gpu, entry, c, window))
        absent = entry.run(device_case(gpu, entry, c, window), absent=True)
        assert any(a[:k].any() for (g, *_), (a, k) in field.items() if g == "out"), f"{what}: every result is zero"
        assert_bitwise(what, absent, field)
