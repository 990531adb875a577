"""Host-side contract of the four evaporation ensemble entries (`cloudsc2_ad_evap_ens_*`, `cloudsc2_ad_evap_step_ens_*`):
exported with the header's prototypes, bound with argtypes derived from the single evaporation entries, and every refusal -
what `cloudsc2_ad_evap_*` refuses, what `cloudsc2_ad_ens_*` refuses, and a `cover` that shares storage with another field -
is settled before anything is launched, so none of this needs a GPU.

The dummy pointers are distinct per field here (the other ABI tests give every field the same one): field i of a pointer
array starts i * SPAN bytes behind BASE, SPAN being more than the whole ensemble of one field."""
import ctypes

import pytest

from abi_calls import FIELD, LS, NZ, QSAT, assert_prototype, call  # noqa: F401  (`call`: a fixture)

ENTRIES = ("cloudsc2_ad_evap_ens", "cloudsc2_ad_evap_step_ens")
NMEM = 3
BASE, SPAN = 1 << 20, 1 << 24          # NMEM * FIELD * 8 bytes = 211 968 < SPAN
IN, IN_ADJ, OUT_ADJ, ZERO, ETA, TL, TN, COVER = (BASE + i * 32 * SPAN for i in range(8))


def ptrs(c, base, n, null=()):
    return c.arr([0 if i in null else base + i * SPAN for i in range(n)])


def run(c, entry, sfx, p, nx=64, ls=LS, nmem=NMEM, ms=FIELD, cover=COVER, ready=0, zero=ZERO, eta=ETA, tl=TL, tn=TN, in_=None,
        in_adj=None, out_adj=None):
    skip = (QSAT,) if entry.endswith("step_ens") else ()
    in_ = ptrs(c, IN, 16, skip) if in_ is None else in_
    in_adj = ptrs(c, IN_ADJ, 10) if in_adj is None else in_adj
    out_adj = ptrs(c, OUT_ADJ, 16, skip) if out_adj is None else out_adj
    return getattr(c.lib, f"{entry}_{sfx}")(ctypes.byref(p), nx, NZ, ls, in_, in_adj, zero, eta, tl, tn, out_adj, 60.0, cover,
                                           ready, None, nmem, ms)


def test_the_four_symbols_are_exported_with_argtypes_derived_from_the_single_entries(hip_lib):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    assert _lib.EVAP_ENS_LAYOUTS == {"ad_evap_ens": "ad_evap", "ad_evap_step_ens": "ad_evap_step"}
    arr, ptr = POINTER(c_void_p), c_void_p
    want = [POINTER(Cloudsc2Params), c_int32, c_int32, c_int64, arr, arr, ptr, ptr, ptr, ptr, arr, c_double, ptr, c_int32, ptr,
            c_int32, c_int64]
    for ens, single in _lib.EVAP_ENS_LAYOUTS.items():
        for sfx, elem in (("f64", "double"), ("f32", "float")):
            name = f"cloudsc2_{ens}_{sfx}"
            fn = getattr(hip_lib, name)
            assert tuple(fn.argtypes) == tuple(_lib.SIGNATURES[f"cloudsc2_{single}_{sfx}"][1]) + (c_int32, c_int64)
            assert_prototype(hip_lib, name,
                             ["const Cloudsc2Params*", "int32_t", "int32_t", "int64_t", f"const {elem}* const*",
                              f"const {elem}* const*", f"const {elem}*", f"const {elem}*", f"const {elem}*", f"const {elem}*",
                              f"{elem}* const*", "double", f"{elem}*", "int32_t", "void*", "int32_t", "int64_t"], want)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_good_call_passes_every_check_and_an_empty_one_is_a_no_op(call, entry, sfx):
    import torch

    on = call.params(LEVAPLS2=True)
    assert run(call, entry, sfx, on, nx=0) == 0
    assert run(call, entry, sfx, on, nx=0, cover=None, in_=call.arr([0] * 16), in_adj=call.arr([0] * 10),
               out_adj=call.arr([0] * 16), zero=None, eta=None, tl=None, tn=None) == 0
    if not torch.cuda.is_available():      # (with a GPU this would really launch on the dummy pointers)
        assert run(call, entry, sfx, on) in (-3, -4), call.err()          # every host check passed: CLOUDSC2_E_LAUNCH


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_what_the_single_evaporation_entries_refuse(call, entry, sfx):
    on = call.params(LEVAPLS2=True)
    assert run(call, entry, sfx, on, cover=None) == -1 and "cover is NULL" in call.err()
    assert run(call, entry, sfx, call.params(LDRAIN1D=True), cover=None) == -1 and "cover is NULL" in call.err()
    assert run(call, entry, sfx, call.params()) == -2                               # neither switch
    other = "cloudsc2_ad_step_ens" if entry.endswith("step_ens") else "cloudsc2_ad_ens"
    assert "neither LEVAPLS2 nor LDRAIN1D" in call.err() and f"use {other}" in call.err(), call.err()
    assert run(call, entry, sfx, on, out_adj=call.arr([0] * 16)) == -1 and "nothing would be written" in call.err()
    assert run(call, entry, sfx, on, nx=-1) == -1 and "nx" in call.err()
    assert run(call, entry, sfx, on, nx=65) == -1 and "lev_stride" in call.err()
    assert run(call, entry, sfx, on, eta=None) == -1 and "eta" in call.err()
    assert run(call, entry, sfx, on, tl=None) == -1 and "traj_fplsl" in call.err()
    assert run(call, entry, sfx, on, in_adj=call.arr([0] * 10), zero=None) == -1 and "zero_line" in call.err()
    assert run(call, entry, sfx, on, in_=call.arr([0] * 16)) == -1 and "in" in call.err()
    assert run(call, entry, sfx, call.params(LEVAPLS2=True, ICALL=1)) == -2 and "ICALL" in call.err()
    p = call.params(LEVAPLS2=True)
    p.NLEV = NZ + 1
    assert run(call, entry, sfx, p) == -1 and "NLEV" in call.err()
    if entry.endswith("step_ens"):
        assert run(call, entry, sfx, on, out_adj=ptrs(call, OUT_ADJ, 16)) == -1 and "out_adj[NL_IN_QSAT]" in call.err()
        assert run(call, entry, sfx, call.params(LEVAPLS2=True, LPHYLIN=False)) == -2 and "LPHYLIN" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
@pytest.mark.parametrize("entry", ENTRIES)
def test_what_the_ensemble_adjoints_refuse(call, entry, sfx, big):
    on = call.params(LEVAPLS2=True)
    assert run(call, entry, sfx, on, nmem=0) == -1 and "nmem" in call.err()
    assert run(call, entry, sfx, on, nmem=-2) == -1 and "nmem" in call.err()
    assert run(call, entry, sfx, on, nx=0, nmem=0, cover=None) == -1 and "nmem" in call.err()     # for an empty call too
    assert run(call, entry, sfx, on, ms=FIELD - 1) == -1 and "member_stride" in call.err()
    assert run(call, entry, sfx, on, nx=big, ls=big, ms=(NZ + 1) * big) == -2 and "4 GiB" in call.err()
    # 2^31 / 4 members of 1 024 columns: 2^31 workgroups
    assert run(call, entry, sfx, on, nx=1024, ls=1024, nmem=2 ** 29, ms=(NZ + 1) * 1024) == -2 and "grid limit" in call.err()


@pytest.mark.parametrize("sfx,size", [("f64", 8), ("f32", 4)])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_cover_that_shares_storage_with_another_field_is_refused(call, entry, sfx, size):
    on = call.params(LEVAPLS2=True)
    member = FIELD * size                      # bytes from one member to the next at ms = FIELD
    last = (NZ * LS + 64) * size               # one member's extent in bytes: nz levels at lev_stride and nx columns more
    t_adj = OUT_ADJ + 11 * SPAN                # out_adj[NL_IN_T]
    for cover, what in ((IN, "in[0]"), (IN + 3 * SPAN, "in[3]"), (IN_ADJ + 9 * SPAN, "in_adj[9]"), (t_adj, "out_adj[11]"),
                        (TL, "traj_fplsl"), (TN, "traj_fplsl / traj_fplsn"), (ZERO, "zero_line"), (ETA, "eta"),
                        (t_adj + size, "out_adj[11]"),                              # one element in
                        (t_adj + 2 * member, "out_adj[11]"),                        # cover's member 0 is the field's member 2
                        (t_adj - 2 * member, "out_adj[11]"),                        # cover's member 2 is the field's member 0
                        (t_adj + 2 * member + last - size, "out_adj[11]"),          # one element of the last member
                        (t_adj - 2 * member - last + size, "out_adj[11]"),
                        (ZERO + 512 - size, "zero_line"), (ETA + NZ * size, "eta"), (ZERO - 2 * member - last + size, "zero_line")):
        assert run(call, entry, sfx, on, cover=cover) == -1, (what, call.err())
        assert "cover overlaps" in call.err() and what in call.err(), (what, call.err())
    import torch

    if not torch.cuda.is_available():          # disjoint by one element: past every host check (with a GPU it would launch)
        for cover in (t_adj + 2 * member + last, t_adj - 2 * member - last, ZERO + 512, ZERO - 2 * member - last,
                      ETA + (NZ + 1) * size):
            assert run(call, entry, sfx, on, cover=cover) in (-3, -4), (cover, call.err())
        # a member stride beyond the extent: a cover that lies in the other field's gaps touches none of its members
        assert run(call, entry, sfx, on, ms=4 * FIELD, cover=t_adj + 2 * member) in (-3, -4), call.err()
        assert run(call, entry, sfx, on, ms=4 * FIELD, cover=t_adj + 2 * member - size) in (-3, -4), call.err()
    assert run(call, entry, sfx, on, ms=4 * FIELD, cover=t_adj + 4 * member - size) == -1 and "cover overlaps" in call.err()
