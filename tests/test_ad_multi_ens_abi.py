"""Host-side contract of the members-times-directions adjoint entries (`cloudsc2_ad_multi_ens_*`,
`cloudsc2_ad_multi_step_ens_*`): exported with the header's prototypes, bound with argtypes derived from the multi entries,
and every argument error and refusal - the multi entry's and the ones the member arguments add - is settled before
anything is launched, so none of this needs a GPU.

Not tested: the LDS bound of 160 KB.  The launcher applies it as `cloudsc2_ad_multi_*` does, but without the evaporation
block no call that passes the other checks reaches it: nz <= 4095 and ndir <= 8 ask for at most (2 * 4096 + 48 * 256) * 8
bytes = 160 KB exactly in fp64, and less in fp32."""
import pytest

from abi_calls import FIELD, LS, NZ, assert_prototype, call, max_dirs  # noqa: F401  (`call`: a fixture)

ENTRIES = ("cloudsc2_ad_multi_ens", "cloudsc2_ad_multi_step_ens")


def _run(call, entry, sfx, p, nx=64, ls=LS, ndir=2, in_ds=None, out_ds=None, nmem=3, ms=None, in_ms=None, out_ms=None,
         ptrs=True, qsat_adj=False, **kw):
    """an entry on dummy pointers (`ptrs=False`: every pointer NULL); strides default to the packed member-major layout"""
    a, P = call.arr, call.P if ptrs else 0
    field = (NZ + 1) * ls
    in_ds = field if in_ds is None else in_ds
    out_ds = field if out_ds is None else out_ds
    tail = (ndir, in_ds, out_ds, nmem, field if ms is None else ms, ndir * in_ds if in_ms is None else in_ms,
            ndir * out_ds if out_ms is None else out_ms)
    step = "step" in entry
    kw.setdefault("in_", a([P] * 16))
    kw.setdefault("in_adj", a([P] * 10))
    kw.setdefault("out_adj", call.no_qsat(fill=P) if step and not qsat_adj else a([P] * 16))
    return call.ad(p, nx=nx, ls=ls, zero=P or None, eta=P or None, tl=P or None, tn=P or None, sfx=sfx, entry=entry,
                   dirs=tail, **kw)


def test_the_four_symbols_are_exported_with_argtypes_derived_from_the_multi_entries(hip_lib):
    from ctypes import c_int32, c_int64

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    assert _lib.MULTI_ENS_LAYOUTS == {"ad_multi_ens": "ad_multi", "ad_multi_step_ens": "ad_multi_step"}
    for ens, multi in _lib.MULTI_ENS_LAYOUTS.items():
        for sfx in ("f64", "f32"):
            name = f"cloudsc2_{ens}_{sfx}"
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
            fn = getattr(hip_lib, name)
            assert fn.restype is c_int32
            assert tuple(fn.argtypes) == tuple(_lib.SIGNATURES[f"cloudsc2_{multi}_{sfx}"][1]) + (c_int32, c_int64, c_int64,
                                                                                                   c_int64)
    assert hip_lib.cloudsc2_abi_version() == 4      # purely additive


def test_the_headers_prototypes(hip_lib):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    arr, ptr = POINTER(c_void_p), c_void_p
    want = [POINTER(Cloudsc2Params), c_int32, c_int32, c_int64, arr, arr, ptr, ptr, ptr, ptr, arr, c_double, ptr,
            c_int32, c_int64, c_int64, c_int32, c_int64, c_int64, c_int64]
    for entry in ENTRIES:
        for sfx, elem in (("f64", "double"), ("f32", "float")):
            assert_prototype(hip_lib, f"{entry}_{sfx}",
                             ["const Cloudsc2Params*", "int32_t", "int32_t", "int64_t", f"const {elem}* const*",
                              f"const {elem}* const*", f"const {elem}*", f"const {elem}*", f"const {elem}*", f"const {elem}*",
                              f"{elem}* const*", "double", "void*", "int32_t", "int64_t", "int64_t", "int32_t", "int64_t",
                              "int64_t", "int64_t"], want)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_direction_arguments_are_checked_without_a_launch(call, entry, sfx):
    p = call.params()
    assert _run(call, entry, sfx, p, ndir=0) == -1 and "ndir" in call.err()
    assert _run(call, entry, sfx, p, ndir=max_dirs("ad") + 1) == -1 and "ndir" in call.err()
    assert _run(call, entry, sfx, p, in_ds=FIELD - 1) == -1 and "in_dir_stride" in call.err()
    assert _run(call, entry, sfx, p, out_ds=FIELD - 1) == -1 and "out_dir_stride" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_member_arguments_are_checked_without_a_launch(call, entry, sfx):
    p = call.params()
    assert _run(call, entry, sfx, p, nmem=0) == -1 and "nmem" in call.err()
    assert _run(call, entry, sfx, p, nmem=-2) == -1 and "nmem" in call.err()
    assert _run(call, entry, sfx, p, ms=FIELD - 1) == -1 and "member_stride" in call.err()
    # the member arguments are checked for an empty call too
    assert _run(call, entry, sfx, p, nx=0, nmem=0, ptrs=False) == -1 and "nmem" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_batches_are_member_major(call, entry, sfx):
    """a member's directions lie inside its member stride: direction-major batches (member stride = one field) are refused"""
    p = call.params()
    kw = dict(ndir=3, in_ds=FIELD + 250, out_ds=FIELD + 250)
    least = 2 * (FIELD + 250) + FIELD     # (ndir-1) * direction stride + one field
    assert _run(call, entry, sfx, p, in_ms=least - 1, **kw) == -1 and "in_member_stride" in call.err()
    assert _run(call, entry, sfx, p, out_ms=least - 1, **kw) == -1 and "out_member_stride" in call.err()
    assert _run(call, entry, sfx, p, in_ms=FIELD, **kw) == -1 and "in_member_stride" in call.err()
    assert _run(call, entry, sfx, p, out_ms=FIELD, **kw) == -1 and "out_member_stride" in call.err()
    # the least strides pass the host checks (an empty call: nothing is launched)
    assert _run(call, entry, sfx, p, nx=0, in_ms=least, out_ms=least, ptrs=False, **kw) == 0
    assert _run(call, entry, sfx, p, nx=0, in_ms=least - 1, out_ms=least, ptrs=False, **kw) == -1
    # strides whose product with ndir - 1 does not fit 64 bits are compared all the same
    huge = 2 ** 62
    assert _run(call, entry, sfx, p, ndir=3, in_ds=huge, out_ds=FIELD, in_ms=huge, out_ms=3 * FIELD) == -1
    assert "in_member_stride" in call.err()
    assert _run(call, entry, sfx, p, ndir=3, in_ds=FIELD, out_ds=huge, in_ms=3 * FIELD, out_ms=huge) == -1
    assert "out_member_stride" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("switch", ["LEVAPLS2", "LDRAIN1D"])
def test_the_evaporation_switches_are_refused(call, switch, entry, sfx):
    assert _run(call, entry, sfx, call.params(**{switch: True})) == -2 and "LEVAPLS2 / LDRAIN1D" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_step_entry_needs_lphylin_and_stores_no_qsat_adjoint(call, sfx):
    entry = "cloudsc2_ad_multi_step_ens"
    assert _run(call, entry, sfx, call.params(LPHYLIN=False)) == -2 and "LPHYLIN" in call.err()
    assert _run(call, entry, sfx, call.params(), qsat_adj=True) == -1 and "out_adj[NL_IN_QSAT]" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_multi_entrys_other_refusals_hold(call, entry, sfx):
    p, a = call.params(), call.arr
    assert _run(call, entry, sfx, call.params(ICALL=1)) == -2 and "ICALL" in call.err()
    assert _run(call, entry, sfx, p, nx=65) == -1 and "lev_stride" in call.err()
    assert _run(call, entry, sfx, p, out_adj=a([0] * 16)) == -1 and "nothing would be written" in call.err()
    assert call.ad(p, in_=a([call.P] * 16), in_adj=a([0] + [call.P] * 9), zero=None, sfx=sfx, entry=entry,
                   dirs=(2, FIELD, FIELD, 3, FIELD, 2 * FIELD, 2 * FIELD)) == -1 and "zero_line" in call.err()
    q = call.params()
    q.NLEV = NZ + 1
    assert _run(call, entry, sfx, q) == -1 and "NLEV" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
@pytest.mark.parametrize("entry", ENTRIES)
def test_4_gib_per_member_and_direction_and_the_grid_limit(call, entry, sfx, big):
    p = call.params()
    assert _run(call, entry, sfx, p, nx=big, ls=big) == -2 and "4 GiB" in call.err()
    # 2^31 / 4 members of 1 024 columns: 2^31 workgroups
    assert _run(call, entry, sfx, p, nx=1024, ls=1024, nmem=2 ** 29) == -2 and "grid limit" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_call_is_a_successful_no_op(call, entry, sfx):
    assert _run(call, entry, sfx, call.params(), nx=0, ptrs=False) == 0
