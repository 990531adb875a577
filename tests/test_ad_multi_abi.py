"""Host-side contract of the multi-direction adjoint entries (`cloudsc2_ad_multi_*`, `cloudsc2_ad_multi_step_*`): exported
with the header's prototypes, and every argument error and refusal is settled before anything is launched, so none of this
needs a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cloudsc2_ad_multi", "cloudsc2_ad_multi_step")
NZ, LS = 137, 64
FIELD = (NZ + 1) * LS


def _header():
    return open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read()


def _max_dirs():
    return int(re.search(r"#define\s+CLOUDSC2_AD_MAX_DIRS\s+(\d+)", _header()).group(1))


@pytest.fixture()
def call(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    class Call:
        P = 4096                  # a non-NULL, 16-byte aligned dummy pointer: never dereferenced on these paths
        err = staticmethod(_lib.last_error)

        def params(self, **over):
            return make_params(dict(default_externals(), NLEV=NZ, **over))

        def __call__(self, entry, sfx, p, nx=64, ndir=2, in_ds=FIELD, out_ds=FIELD, ptrs=True, qsat_adj=None):
            a = _lib.ptr_array
            # the step entry stores no qsat adjoint
            with_qsat = not entry.endswith("step") if qsat_adj is None else qsat_adj
            out_adj = [self.P if n != "qsat" or with_qsat else 0 for n in _lib.NL_IN]
            return getattr(hip_lib, f"{entry}_{sfx}")(
                ctypes.byref(p), nx, NZ, LS, a([self.P] * 16 if ptrs else [0] * 16), a([self.P] * 10 if ptrs else [0] * 10),
                self.P if ptrs else None, self.P if ptrs else None, self.P if ptrs else None, self.P if ptrs else None,
                a(out_adj if ptrs else [0] * 16), 3600.0, None, ndir, in_ds, out_ds)

    return Call()


def test_the_four_symbols_are_exported_with_the_headers_prototypes(hip_lib):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    arr, ptr = POINTER(c_void_p), c_void_p
    want = [POINTER(Cloudsc2Params), c_int32, c_int32, c_int64, arr, arr, ptr, ptr, ptr, ptr, arr, c_double, ptr,
            c_int32, c_int64, c_int64]
    for entry in ENTRIES:
        for sfx, elem in (("f64", "double"), ("f32", "float")):
            name = f"{entry}_{sfx}"
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
            params = re.search(rf"int32_t\s+{name}\s*\(([^)]*)\)\s*;", header).group(1)
            types = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", x.strip())).strip() for x in params.split(",")]
            assert types == ["const Cloudsc2Params*", "int32_t", "int32_t", "int64_t", f"const {elem}* const*",
                             f"const {elem}* const*", f"const {elem}*", f"const {elem}*", f"const {elem}*", f"const {elem}*",
                             f"{elem}* const*", "double", "void*", "int32_t", "int64_t", "int64_t"], (name, types)
            fn = getattr(hip_lib, name)
            assert fn.restype is c_int32 and list(fn.argtypes) == want, (name, fn.argtypes)
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
def test_at_least_one_adjoint_is_wanted(hip_lib, call, entry, sfx):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    p, a, P = call.params(), _lib.ptr_array, call.P
    rc = getattr(hip_lib, f"{entry}_{sfx}")(ctypes.byref(p), 64, NZ, LS, a([P] * 16), a([P] * 10), P, P, P, P, a([0] * 16),
                                              3600.0, None, 2, FIELD, FIELD)
    assert rc == -1 and "nothing would be written" in call.err()


@pytest.mark.parametrize("sfx,big", [("f64", 4_000_000), ("f32", 8_000_000)])
def test_fields_of_4_gib_per_direction_are_refused(hip_lib, call, sfx, big):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    p, a, P = call.params(), _lib.ptr_array, call.P
    for entry in ENTRIES:
        out_adj = a([P] * 9 + [0] + [P] * 6)
        rc = getattr(hip_lib, f"{entry}_{sfx}")(ctypes.byref(p), big, NZ, big, a([P] * 16), a([P] * 10), P, P, P, P, out_adj,
                                                  3600.0, None, 2, (NZ + 1) * big, (NZ + 1) * big)
        assert rc == -2 and "4 GiB" in call.err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_call_is_a_successful_no_op(call, entry, sfx):
    assert call(entry, sfx, call.params(), nx=0, ptrs=False) == 0
