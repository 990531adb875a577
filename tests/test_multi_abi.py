"""Host-side contract of the multi-direction tangent-linear entries (`cloudsc2_tl_multi_*`, `cloudsc2_tl_multi_step_*`):
exported with the header's prototypes, and every argument error is settled before anything is launched, so none of this
needs a GPU."""
import pytest

from abi_calls import FIELD, NZ, assert_prototype, call, max_dirs  # noqa: F401  (`call`: a fixture)

ENTRIES = ("cloudsc2_tl_multi", "cloudsc2_tl_multi_step")


def _max_dirs():
    return max_dirs("tl")


def test_the_four_symbols_are_exported_with_the_headers_prototypes(hip_lib):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    arr, ptr = POINTER(c_void_p), c_void_p
    want = [POINTER(Cloudsc2Params), c_int32, c_int32, c_int64, arr, arr, ptr, ptr, arr, arr, c_double, ptr,
            c_int32, c_int64, c_int64]
    for entry in ENTRIES:
        for sfx, elem in (("f64", "double"), ("f32", "float")):
            assert_prototype(hip_lib, f"{entry}_{sfx}",
                             ["const Cloudsc2Params*", "int32_t", "int32_t", "int64_t", f"const {elem}* const*",
                              f"const {elem}* const*", f"const {elem}*", f"const {elem}*", f"{elem}* const*",
                              f"{elem}* const*", "double", "void*", "int32_t", "int64_t", "int64_t"], want)
    assert _lib.TL_MAX_DIRS == _max_dirs()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_direction_arguments_are_checked_without_a_launch(call, entry, sfx):
    p = call.params()
    assert call(entry, sfx, p, ndir=0) == -1 and "ndir" in call.err()
    assert call(entry, sfx, p, ndir=_max_dirs() + 1) == -1 and "ndir" in call.err()
    assert call(entry, sfx, p, in_ds=FIELD - 1) == -1 and "in_dir_stride" in call.err()
    assert call(entry, sfx, p, out_ds=FIELD - 1) == -1 and "out_dir_stride" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_step_entry_needs_lphylin(call, sfx):
    assert call("cloudsc2_tl_multi_step", sfx, call.params(LPHYLIN=False)) == -2 and "LPHYLIN" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
def test_fields_of_4_gib_per_direction_are_refused(call, sfx, big):
    p, a, P = call.params(), call.arr, call.P
    for entry in ENTRIES:
        in_i = a([P] * 9 + [0] + [P] * 6)
        rc = call.tl(p, nx=big, ls=big, in_=a([P] * 16), in_i=in_i, sfx=sfx, entry=entry,
                     dirs=(2, (NZ + 1) * big, (NZ + 1) * big))
        assert rc == -2 and "4 GiB" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_call_is_a_successful_no_op(call, entry, sfx):
    assert call(entry, sfx, call.params(), nx=0, ptrs=False) == 0
