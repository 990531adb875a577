"""Host-side contract of the twelve ensemble entries (`cloudsc2_{nl,nl_fused,tl,tl_step,ad,ad_step}_ens_*`): exported with
the header's prototypes, bound with argtypes derived from the single entries, and every argument error and refusal - the
single entry's and the ones the member arguments add - is settled before anything is launched, so none of this needs a
GPU."""
import ctypes

import pytest

from abi_calls import FIELD, LS, NZ, assert_prototype, call  # noqa: F401  (`call`: a fixture)

TL = ("cloudsc2_tl_ens", "cloudsc2_tl_step_ens")
AD = ("cloudsc2_ad_ens", "cloudsc2_ad_step_ens")
NL = ("cloudsc2_nl_ens", "cloudsc2_nl_fused_ens")
ALL = NL + TL + AD


def _run(call, entry, sfx, p, nx=64, ls=LS, nmem=3, ms=FIELD, ptrs=True, **kw):
    """an ensemble entry on dummy pointers (`ptrs=False`: every pointer NULL)"""
    a, P = call.arr, call.P if ptrs else 0
    tail = (nmem, ms)
    step = "step" in entry
    if entry in TL:
        kw.setdefault("in_", call.no_qsat(fill=P) if step else a([P] * 16))
        kw.setdefault("in_i", call.no_qsat(fill=P) if step else a([P] * 16))
        kw.setdefault("out_i", a([P] * 10))
        return call.tl(p, nx=nx, ls=ls, zero=P or None, eta=P or None, sfx=sfx, entry=entry, dirs=tail, **kw)
    if entry in AD:
        kw.setdefault("in_", call.no_qsat(fill=P) if step else a([P] * 16))
        kw.setdefault("in_adj", a([P] * 10))
        kw.setdefault("out_adj", call.no_qsat(fill=P) if step else a([P] * 16))
        return call.ad(p, nx=nx, ls=ls, zero=P or None, eta=P or None, tl=P or None, tn=P or None, sfx=sfx, entry=entry,
                       dirs=tail, **kw)
    fn = getattr(call.lib, f"{entry}_{sfx}")
    out = kw.get("out", a([P] * 10))
    if entry == "cloudsc2_nl_ens":
        return fn(ctypes.byref(p), nx, NZ, ls, kw.get("in_", a([P] * 16)), P or None, out, kw.get("dt", 3600.0), None, *tail)
    return fn(ctypes.byref(p), nx, NZ, ls, kw.get("in_", call.no_qsat(fill=P)), kw.get("in_i"), 0.0,
              kw.get("qsat_out", P or None), P or None, out, kw.get("dt", 3600.0), None, *tail)


def test_the_twelve_symbols_are_exported_with_argtypes_derived_from_the_single_entries(hip_lib):
    from ctypes import c_int32, c_int64

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    assert _lib.ENS_LAYOUTS == {"nl_ens": "nl", "nl_fused_ens": "nl_fused", "tl_ens": "tl_masked", "tl_step_ens": "tl_step",
                                "ad_ens": "ad_masked", "ad_step_ens": "ad_step"}
    for ens, single in _lib.ENS_LAYOUTS.items():
        for sfx in ("f64", "f32"):
            name = f"cloudsc2_{ens}_{sfx}"
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
            fn = getattr(hip_lib, name)
            assert fn.restype is c_int32
            assert tuple(fn.argtypes) == tuple(_lib.SIGNATURES[f"cloudsc2_{single}_{sfx}"][1]) + (c_int32, c_int64)


def test_the_headers_prototype_of_an_adjoint_entry(hip_lib):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    arr, ptr = POINTER(c_void_p), c_void_p
    want = [POINTER(Cloudsc2Params), c_int32, c_int32, c_int64, arr, arr, ptr, ptr, ptr, ptr, arr, c_double, ptr, c_int32,
            c_int64]
    for entry in AD:
        for sfx, elem in (("f64", "double"), ("f32", "float")):
            assert_prototype(hip_lib, f"{entry}_{sfx}",
                             ["const Cloudsc2Params*", "int32_t", "int32_t", "int64_t", f"const {elem}* const*",
                              f"const {elem}* const*", f"const {elem}*", f"const {elem}*", f"const {elem}*", f"const {elem}*",
                              f"{elem}* const*", "double", "void*", "int32_t", "int64_t"], want)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ALL)
def test_member_arguments_are_checked_without_a_launch(call, entry, sfx):
    p = call.params()
    assert _run(call, entry, sfx, p, nmem=0) == -1 and "nmem" in call.err()
    assert _run(call, entry, sfx, p, nmem=-2) == -1 and "nmem" in call.err()
    assert _run(call, entry, sfx, p, ms=FIELD - 1) == -1 and "member_stride" in call.err()
    # the member arguments are checked for an empty call too
    assert _run(call, entry, sfx, p, nx=0, nmem=0, ptrs=False) == -1 and "nmem" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
@pytest.mark.parametrize("entry", ALL)
def test_one_member_of_4_gib_is_refused_and_so_is_a_grid_beyond_the_limit(call, entry, sfx, big):
    p = call.params()
    assert _run(call, entry, sfx, p, nx=big, ls=big, ms=(NZ + 1) * big) == -2 and "4 GiB" in call.err()
    # 2^31 / 4 members of 1 024 columns: 2^31 workgroups
    assert _run(call, entry, sfx, p, nx=1024, ls=1024, nmem=2 ** 29, ms=(NZ + 1) * 1024) == -2 and "grid limit" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ALL)
def test_the_single_entrys_refusals_hold(call, entry, sfx):
    assert _run(call, entry, sfx, call.params(ICALL=1)) == -2 and "ICALL" in call.err()
    if entry in NL:
        assert _run(call, entry, sfx, call.params(), dt=0.0) == -1 and "dt=" in call.err()
    assert _run(call, entry, sfx, call.params(), nx=65) == -1 and "lev_stride" in call.err()
    if entry in TL + AD:
        p = call.params()
        p.NLEV = NZ + 1
        assert _run(call, entry, sfx, p) == -1 and "NLEV" in call.err()
    if "step" in entry or "fused" in entry:
        assert _run(call, entry, sfx, call.params(LPHYLIN=False)) == -2 and "LPHYLIN" in call.err()
    if entry in AD:
        for switch in ("LEVAPLS2", "LDRAIN1D"):
            assert _run(call, entry, sfx, call.params(**{switch: True})) == -2 and "LEVAPLS2 / LDRAIN1D" in call.err()
        assert _run(call, entry, sfx, call.params(), out_adj=call.arr([0] * 16)) == -1 and "nothing would be written" in call.err()
    if entry in TL:
        assert _run(call, entry, sfx, call.params(), out_i=call.arr([0] * 10)) == -1 and "nothing would be written" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_null_rules(call, sfx):
    p, a, P = call.params(), call.arr, call.P
    # a zero field needs the zero line
    assert call.tl(p, in_i=a([0] + [P] * 15), zero=None, sfx=sfx, entry="cloudsc2_tl_ens", dirs=(2, FIELD)) == -1
    assert "zero_line" in call.err()
    assert call.ad(p, in_adj=a([0] + [P] * 9), zero=None, sfx=sfx, entry="cloudsc2_ad_ens", dirs=(2, FIELD)) == -1
    assert "zero_line" in call.err()
    # the step entries form qsat themselves
    assert _run(call, "cloudsc2_tl_step_ens", sfx, p, in_i=a([P] * 16)) == -1 and "in_i[NL_IN_QSAT]" in call.err()
    assert _run(call, "cloudsc2_ad_step_ens", sfx, p, out_adj=a([P] * 16)) == -1 and "out_adj[NL_IN_QSAT]" in call.err()
    assert _run(call, "cloudsc2_nl_ens", sfx, p, in_=a([P] * 15 + [0])) == -1 and "in[15]" in call.err()
    # the fused ensemble entry is the saturation-fused form only
    assert _run(call, "cloudsc2_nl_fused_ens", sfx, p, qsat_out=None) == -1 and "qsat_out is required" in call.err()
    assert _run(call, "cloudsc2_nl_fused_ens", sfx, p, in_i=a([P] * 16)) == -1 and "in_i must" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ALL)
def test_empty_call_is_a_successful_no_op(call, entry, sfx):
    assert _run(call, entry, sfx, call.params(), nx=0, ptrs=False) == 0
