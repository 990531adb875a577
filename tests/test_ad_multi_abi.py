"""Host-side contract of the multi-direction adjoint entries (`cloudsc2_ad_multi_*`, `cloudsc2_ad_multi_step_*`): exported
with the header's prototypes, and every argument error and refusal is settled before anything is launched, so none of this
needs a GPU."""
import pytest

from abi_calls import FIELD, NZ, assert_prototype, call, max_dirs  # noqa: F401  (`call`: a fixture)

ENTRIES = ("cloudsc2_ad_multi", "cloudsc2_ad_multi_step")


def _max_dirs():
    return max_dirs("ad")


def test_the_four_symbols_are_exported_with_the_headers_prototypes(hip_lib):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    arr, ptr = POINTER(c_void_p), c_void_p
    want = [POINTER(Cloudsc2Params), c_int32, c_int32, c_int64, arr, arr, ptr, ptr, ptr, ptr, arr, c_double, ptr,
            c_int32, c_int64, c_int64]
    for entry in ENTRIES:
        for sfx, elem in (("f64", "double"), ("f32", "float")):
            name = f"{entry}_{sfx}"
            assert_prototype(hip_lib, name,
                             ["const Cloudsc2Params*", "int32_t", "int32_t", "int64_t", f"const {elem}* const*",
                              f"const {elem}* const*", f"const {elem}*", f"const {elem}*", f"const {elem}*", f"const {elem}*",
                              f"{elem}* const*", "double", "void*", "int32_t", "int64_t", "int64_t"], want)
            fn = getattr(hip_lib, name)
            # derived: the single-direction entry's arguments followed by the three direction arguments
            single = _lib.SIGNATURES["cloudsc2_" + _lib.MULTI_LAYOUTS[entry[len("cloudsc2_"):]] + "_" + sfx][1]
            assert tuple(fn.argtypes) == tuple(single) + (c_int32, c_int64, c_int64)
    assert _lib.MULTI_LAYOUTS["ad_multi"] == "ad_masked" and _lib.MULTI_LAYOUTS["ad_multi_step"] == "ad_step"


def test_the_binding_knows_the_headers_limit():
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    assert _lib.AD_MAX_DIRS == _max_dirs() == 8


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_direction_arguments_are_checked_without_a_launch(call, entry, sfx):
    p = call.params()
    assert call(entry, sfx, p, ndir=0) == -1 and "ndir" in call.err()
    assert call(entry, sfx, p, ndir=_max_dirs() + 1) == -1 and "ndir" in call.err()
    assert call(entry, sfx, p, in_ds=FIELD - 1) == -1 and "in_dir_stride" in call.err()
    assert call(entry, sfx, p, out_ds=FIELD - 1) == -1 and "out_dir_stride" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("switch", ["LEVAPLS2", "LDRAIN1D"])
def test_the_evaporation_switches_are_refused(call, switch, entry, sfx):
    assert call(entry, sfx, call.params(**{switch: True})) == -2 and "LEVAPLS2 / LDRAIN1D" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_step_entry_needs_lphylin(call, sfx):
    assert call("cloudsc2_ad_multi_step", sfx, call.params(LPHYLIN=False)) == -2 and "LPHYLIN" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_step_entry_stores_no_qsat_adjoint(call, sfx):
    assert call("cloudsc2_ad_multi_step", sfx, call.params(), qsat_adj=True) == -1 and "out_adj[NL_IN_QSAT]" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_at_least_one_adjoint_is_wanted(call, entry, sfx):
    p, a, P = call.params(), call.arr, call.P
    rc = call.ad(p, in_=a([P] * 16), out_adj=a([0] * 16), sfx=sfx, entry=entry, dirs=(2, FIELD, FIELD))
    assert rc == -1 and "nothing would be written" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
def test_fields_of_4_gib_per_direction_are_refused(call, sfx, big):
    p, a, P = call.params(), call.arr, call.P
    for entry in ENTRIES:
        out_adj = a([P] * 9 + [0] + [P] * 6)
        rc = call.ad(p, nx=big, ls=big, in_=a([P] * 16), out_adj=out_adj, sfx=sfx, entry=entry,
                     dirs=(2, (NZ + 1) * big, (NZ + 1) * big))
        assert rc == -2 and "4 GiB" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_call_is_a_successful_no_op(call, entry, sfx):
    assert call(entry, sfx, call.params(), nx=0, ptrs=False) == 0
