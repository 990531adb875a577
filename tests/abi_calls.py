"""The derivative entries of the C ABI called with dummy pointers: every argument error is settled before anything is
launched, so the host-only tests (`test_*_abi.py`) need no GPU.  They import the `call` fixture by name."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NZ, LS = 137, 64
FIELD = (NZ + 1) * LS
QSAT = 9     # NL_IN_QSAT


def header():
    return open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read()


def max_dirs(kind):
    """CLOUDSC2_TL_MAX_DIRS / CLOUDSC2_AD_MAX_DIRS of the header; kind: "tl" or "ad" """
    return int(re.search(rf"#define\s+CLOUDSC2_{kind.upper()}_MAX_DIRS\s+(\d+)", header()).group(1))


def assert_prototype(hip_lib, name, c_types, ctypes_types):
    """`name` is exported, declared in the header with the parameter types `c_types`, and bound with `ctypes_types`"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    params = re.search(rf"int32_t\s+{name}\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header(), flags=re.S)).group(1)
    types = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", x.strip())).strip() for x in params.split(",")]
    assert types == c_types, (name, types)
    fn = getattr(hip_lib, name)
    assert fn.restype is ctypes.c_int32 and list(fn.argtypes) == ctypes_types, (name, fn.argtypes)


class Call:
    """`tl` / `ad`: `cloudsc2_{tl,ad}_<family>` with `family` masked or step by default, any entry by name, and with `dirs`
    = (ndir, in_dir_stride, out_dir_stride) a multi entry; calling the object itself is the multi form.  A step entry's
    default arrays have a NULL qsat slot, except the trajectory of a multi entry."""
    P = 4096                  # a non-NULL, 16-byte aligned dummy pointer: never dereferenced on these paths

    def __init__(self, hip_lib, family):
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

        self.lib, self.family, self.arr, self.err = hip_lib, family, _lib.ptr_array, _lib.last_error

    def params(self, **over):
        from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

        return make_params(dict(default_externals(), NLEV=NZ, **over))

    def no_qsat(self, n=16, fill=None):
        fill = self.P if fill is None else fill
        return self.arr([0 if i == QSAT else fill for i in range(n)])

    def _in16(self, entry):
        return self.no_qsat() if entry.endswith("step") else self.arr([self.P] * 16)

    def tl(self, p, nx=64, ls=LS, in_=None, in_i=None, zero=P, eta=P, out=None, out_i=None, sfx="f64", entry=None, dirs=()):
        entry = entry or "cloudsc2_tl_" + self.family
        return getattr(self.lib, f"{entry}_{sfx}")(
            ctypes.byref(p), nx, NZ, ls, self._in16(entry) if in_ is None else in_, self._in16(entry) if in_i is None else in_i,
            zero, eta, out, self.arr([self.P] * 10) if out_i is None else out_i, 3600.0, None, *dirs)

    def ad(self, p, nx=64, ls=LS, in_=None, in_adj=None, zero=P, eta=P, tl=P, tn=P, out_adj=None, sfx="f64", entry=None,
           dirs=()):
        entry = entry or "cloudsc2_ad_" + self.family
        return getattr(self.lib, f"{entry}_{sfx}")(
            ctypes.byref(p), nx, NZ, ls, self._in16(entry) if in_ is None else in_,
            self.arr([self.P] * 10) if in_adj is None else in_adj, zero, eta, tl, tn,
            self._in16(entry) if out_adj is None else out_adj, 3600.0, None, *dirs)

    def __call__(self, entry, sfx, p, nx=64, ndir=2, in_ds=FIELD, out_ds=FIELD, ptrs=True, qsat_adj=None):
        """a multi entry; `ptrs=False`: every pointer NULL; `qsat_adj`: whether a qsat adjoint is asked for (by default
        not from a step entry, which stores none)"""
        a, all16 = self.arr, self.arr([self.P] * 16)
        kw = dict(nx=nx, sfx=sfx, entry=entry, dirs=(ndir, in_ds, out_ds))
        if "_tl_" in entry:
            if not ptrs:
                return self.tl(p, in_=a([0] * 16), in_i=a([0] * 16), zero=None, eta=None, out_i=a([0] * 10), **kw)
            return self.tl(p, in_=all16, **kw)
        if not ptrs:
            return self.ad(p, in_=a([0] * 16), in_adj=a([0] * 10), zero=None, eta=None, tl=None, tn=None, out_adj=a([0] * 16),
                           **kw)
        out_adj = None if qsat_adj is None else all16 if qsat_adj else self.no_qsat()
        return self.ad(p, in_=all16, out_adj=out_adj, **kw)

    def sat_tl(self, p, nx=64, ap=P, t=P, ap_i=P, t_i=P, qsat=P, qsat_i=P, sfx="f64"):
        return getattr(self.lib, "cloudsc2_saturation_tl_" + sfx)(ctypes.byref(p), nx, NZ, max(nx, 64), ap, t, ap_i, t_i,
                                                                  qsat, qsat_i, None)

    def sat_ad(self, p, nx=64, ap=P, t=P, q=P, ap_adj=P, t_adj=P, acc=0, sfx="f64"):
        return getattr(self.lib, "cloudsc2_saturation_ad_" + sfx)(ctypes.byref(p), nx, NZ, max(nx, 64), ap, t, q, ap_adj,
                                                                  t_adj, acc, None)


@pytest.fixture()
def call(hip_lib, request):
    """the dummy caller; a module's `FAMILY` ("masked", "step") names the entries its `tl` / `ad` mean by default"""
    return Call(hip_lib, getattr(request.module, "FAMILY", None))
