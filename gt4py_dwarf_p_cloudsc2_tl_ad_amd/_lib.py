"""ctypes binding of libcloudsc2_hip.so (the C ABI declared in include/cloudsc2_hip.h).

There is NO fallback: if the shared library is missing or stale this module raises, and every
stencil object built on top of it is unusable.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C gt4py_dwarf_p_cloudsc2_tl_ad_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_void_p
from typing import Any, Dict, NamedTuple, Optional, Sequence, Tuple

from .params import ABI_VERSION, Cloudsc2Params

LIB_NAME = "libcloudsc2_hip.so"
#: CLOUDSC2_HIP_LIB overrides the library file (dev / A-B builds made by profiles/build_variants.sh); same checks apply
LIB_PATH = os.environ.get("CLOUDSC2_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

# gtscript parameter names in C-ABI order (include/cloudsc2_hip.h enums)
NL_IN = ("ap", "aph", "lu", "lude", "mfd", "mfu", "q", "qi", "ql", "qsat", "supsat", "t",
         "tnd_cml_q", "tnd_cml_qi", "tnd_cml_ql", "tnd_cml_t")
NL_OUT = ("clc", "covptot", "fhpsl", "fhpsn", "fplsl", "fplsn", "tnd_q", "tnd_qi", "tnd_ql", "tnd_t")
INC = ("aph", "ap", "q", "qsat", "t", "ql", "qi", "lude", "lu", "mfu", "mfd",
       "tnd_cml_t", "tnd_cml_q", "tnd_cml_ql", "tnd_cml_qi", "supsat")


class Arg(NamedTuple):
    """One argument of a stencil's C prototype after `(params, nx, nz, lev_stride)`; `stencils.HipStencil` builds the call
    from these and `SIGNATURES` the ctypes `argtypes`.  Kinds:
      ptrs      array of field pointers; `key`: the call keyword of every slot (None: a NULL slot; empty: the whole array is
                NULL); `unless`: the scalar keyword whose presence replaces the array (it is then NULL and its keywords
                are not accepted)
      field     one field pointer; `key`: its keyword (None: NULL)
      eta       the `in_eta` level vector
      scalar    a double; `key`: its keyword (None: always `default`); `default`: the value when the keyword is absent
                (None: the keyword is required)
      partials  `out_partials`: float64 device buffer of taylor_blocks(nx) x [len(fs) x] len(NL_OUT) elements
      fs        the step sizes: `(int32 count, const double* values)` - TWO C arguments
      stream    the HIP stream"""
    kind: str
    key: Any = None
    unless: Optional[str] = None
    default: Optional[float] = None


def _ptrs(fmt: str, base: Sequence[str], null: Optional[str] = None, unless: Optional[str] = None) -> Arg:
    return Arg("ptrs", tuple(None if n == null else fmt.format(n) for n in base), unless)


class Layout(NamedTuple):
    entry: str                    # C entry points cloudsc2_<entry>_{f64,f32}
    args: Tuple[Arg, ...]
    nlev_offset: int = 1          # domain[2] = nz + nlev_offset
    sets_nlev: bool = False       # external NLEV is checked against / taken from the storages (TL, AD)


_IN, _IN_I = _ptrs("in_{}", NL_IN), _ptrs("in_{}_i", NL_IN)
_OUT, _OUT_I, _REF = _ptrs("out_{}", NL_OUT), _ptrs("out_{}_i", NL_OUT), _ptrs("ref_{}", NL_OUT)
_NO_PTRS, _ETA, _DT, _F, _STREAM = Arg("ptrs", key=()), Arg("eta"), Arg("scalar", "dt"), Arg("scalar", "f"), Arg("stream")

#: THE description of every registered stencil: the argument order of its prototype in include/cloudsc2_hip.h.  Keyword
#: set, pointer arrays, argtypes, exported symbols, "needs in_eta" and "sets NLEV" all follow from an entry here.
#: Keyed by the names the reference registers with `@stencil_collection(name)`; the others are BUILD EXTENSIONS.
LAYOUTS: Dict[str, Layout] = {
    # nonlinear/_stencils/cloudsc2.py:24-60 (signature), :93-399 (body)
    "cloudsc2_nl": Layout("nl", (_IN, _ETA, _OUT, _DT, _STREAM)),
    # `saturation` + `cloudsc2_nl` in one launch: arguments of `cloudsc2_nl` minus `in_qsat`, plus `out_qsat`
    "cloudsc2_nl_saturation": Layout("nl_fused", (_ptrs("in_{}", NL_IN, null="qsat"), _NO_PTRS, Arg("scalar", default=0.0),
                                                  Arg("field", "out_qsat"), _ETA, _OUT, _DT, _STREAM)),
    # `perturbed_state` + `cloudsc2_nl` in one launch (inputs read as in_X + f * in_X_i): plus the 16 `in_*_i` and `f`
    "cloudsc2_nl_perturbed": Layout("nl_fused", (_IN, _IN_I, _F, Arg("field", key=None), _ETA, _OUT, _DT, _STREAM)),
    # perturbed NL run + the Taylor test's reduction in one launch: `ref_*` are the 10 unperturbed outputs (read-only);
    # `out_partials` receives, per workgroup, sum(NL(in + f in_i) - ref) in NL_OUT order.  Nothing else is written.
    "cloudsc2_nl_taylor": Layout("nl_taylor", (_IN, _IN_I, _F, _ETA, _REF, Arg("partials"), _DT, _STREAM)),
    # the same for ALL step sizes `fs` (up to 5 share one pass over the 42 words of a level); `out_partials` is
    # (taylor_blocks(nx), len(fs), 10).  With `f_inc=<factor>` instead of the 16 `in_*_i` fields, `state_increment` is fused in
    # as well: the increments are formed in the kernel as f_inc * in (external IGNORE_SUPSAT zeroes the supsat increment).
    "cloudsc2_nl_taylor_multi": Layout("nl_taylor_multi", (_IN, _ptrs("in_{}_i", NL_IN, unless="f_inc"),
                                                           Arg("scalar", "f_inc", default=0.0), Arg("fs"), _ETA, _REF,
                                                           Arg("partials"), _DT, _STREAM)),
    # tangent_linear/_stencils/cloudsc2.py:23-90 (signature), :124-774 (body)
    "cloudsc2_tl": Layout("tl", (_IN, _IN_I, _ETA, _OUT, _OUT_I, _DT, _STREAM), sets_nlev=True),
    # `state_increment` + `cloudsc2_tl` in one launch: the perturbations are f * in_X, formed in the kernel (external
    # IGNORE_SUPSAT: the supsat perturbation is 0): arguments of `cloudsc2_tl` minus the 16 `in_*_i`, plus `f`
    "cloudsc2_tl_incremented": Layout("tl_incremented", (_IN, _F, _ETA, _OUT, _OUT_I, _DT, _STREAM), sets_nlev=True),
    # adjoint/_stencils/cloudsc2.py:24-90 (signature), :124-996 (body)
    "cloudsc2_ad": Layout("ad", (_IN, _ptrs("in_{}_i", NL_OUT), _ETA, _OUT, _ptrs("out_{}_i", NL_IN), _DT, _STREAM),
                          sets_nlev=True),
    # `cloudsc2_ad` without its forward sweep: minus the ten `out_*` NL outputs, plus `traj_fplsl` / `traj_fplsn`, the flux
    # outputs of a cloudsc2_nl / cloudsc2_tl call on the same state (read-only).  Only the 16 `out_*_i` adjoints are written.
    # Driver switches only (no evaporation block).
    "cloudsc2_ad_from_trajectory": Layout("ad_from_trajectory", (
        _IN, _ptrs("in_{}_i", NL_OUT), _ETA, Arg("field", "traj_fplsl"), Arg("field", "traj_fplsn"),
        _ptrs("out_{}_i", NL_IN), _DT, _STREAM), sets_nlev=True),
    # common/_stencils/saturation.py:23-42; domain (nx, 1, nz)
    "saturation": Layout("saturation", (Arg("field", "in_ap"), Arg("field", "in_t"), Arg("field", "out_qsat"), _STREAM),
                         nlev_offset=0),
    # common/_stencils/state_increment.py:22-80
    "state_increment": Layout("state_increment", (_ptrs("in_{}", INC), _ptrs("out_{}_i", INC), _F, _STREAM)),
    # common/_stencils/perturbed_state.py:22-91
    "perturbed_state": Layout("perturbed_state", (_ptrs("in_{}", INC), _ptrs("in_{}_i", INC), _ptrs("out_{}", INC), _F,
                                                  _STREAM)),
}

#: the multi-direction TL / AD entries (autodiff.tl_multi / tl_step_multi / ad_multi / ad_step_multi call them directly, like
#: the masked entries they extend): name -> the single-direction entry whose argument list they repeat, followed by `ndir`,
#: `in_dir_stride` and `out_dir_stride` (elements)
MULTI_LAYOUTS: Dict[str, str] = {"tl_multi": "tl_masked", "tl_multi_step": "tl_step",
                                 "ad_multi": "ad_masked", "ad_multi_step": "ad_step"}
#: the trajectory adjoints WITH the evaporation block (LEVAPLS2 / LDRAIN1D; autodiff.ad_masked_evap / ad_step_evap /
#: ad_multi_evap / ad_step_multi_evap call them directly), one entry per stencil: name -> the entry whose argument list they
#: repeat, followed by `cover` (a caller-owned device field) and `cover_ready` - in front of `stream` for the single entries,
#: behind the direction arguments for the multi entries
EVAP_LAYOUTS: Dict[str, str] = {"ad_evap": "ad_masked", "ad_evap_step": "ad_step",
                                "ad_evap_multi": "ad_multi", "ad_evap_multi_step": "ad_multi_step"}
#: the ensemble entries (autodiff calls them directly): name -> the single entry whose argument list they repeat, followed by
#: `nmem` and `member_stride` (elements; one stride for every field of the call)
ENS_LAYOUTS: Dict[str, str] = {"nl_ens": "nl", "nl_fused_ens": "nl_fused", "tl_ens": "tl_masked", "tl_step_ens": "tl_step",
                               "ad_ens": "ad_masked", "ad_step_ens": "ad_step"}
#: ensembles that share part of their state (autodiff calls them directly): name -> the `ENS_LAYOUTS` entry whose argument
#: list they repeat, followed by `shared_mask` (bit i: state input NL_IN[i] is one field for all members; `ENSS_COLUMN_MAJOR` /
#: `ENSS_MEMBER_MAJOR` choose the block order) and `eta_member_stride` (elements; 0: one `eta` for all members)
ENSS_LAYOUTS: Dict[str, str] = {ens.replace("_ens", "_enss"): ens for ens in ENS_LAYOUTS}
#: CLOUDSC2_ENSS_COLUMN_MAJOR / CLOUDSC2_ENSS_MEMBER_MAJOR of include/cloudsc2_hip.h
ENSS_COLUMN_MAJOR, ENSS_MEMBER_MAJOR = 1 << 32, 1 << 33
#: the ensemble forms of the two single evaporation entries (autodiff.ad_masked_evap_ens / ad_step_evap_ens call them
#: directly): name -> the `EVAP_LAYOUTS` entry whose argument list they repeat, followed by `nmem` and `member_stride`;
#: `cover` is batched over the members like every other field of the call
EVAP_ENS_LAYOUTS: Dict[str, str] = {"ad_evap_ens": "ad_evap", "ad_evap_step_ens": "ad_evap_step"}
#: members times directions (autodiff.ad_multi_ens / ad_step_multi_ens call them directly): name -> the `MULTI_LAYOUTS` entry
#: whose argument list they repeat, followed by `nmem`, `member_stride` (state and trajectory fluxes), `in_member_stride`
#: (batched forcings) and `out_member_stride` (batched adjoints), all in elements
MULTI_ENS_LAYOUTS: Dict[str, str] = {"ad_multi_ens": "ad_multi", "ad_multi_step_ens": "ad_multi_step"}
#: CLOUDSC2_TL_MAX_DIRS of include/cloudsc2_hip.h
TL_MAX_DIRS = 8
#: CLOUDSC2_AD_MAX_DIRS of include/cloudsc2_hip.h
AD_MAX_DIRS = 8

_PARR = POINTER(c_void_p)      # device pointers travel as integers (void*), never dereferenced on the host
_CTYPES = {"ptrs": (_PARR,), "field": (c_void_p,), "eta": (c_void_p,), "scalar": (c_double,), "partials": (c_void_p,),
           "fs": (c_int32, POINTER(c_double)), "stream": (c_void_p,)}


def _signatures() -> Dict[str, Tuple[Any, Tuple[Any, ...]]]:
    """symbol -> (restype, argtypes) of every entry point include/cloudsc2_hip.h declares"""
    sig: Dict[str, Tuple[Any, Tuple[Any, ...]]] = {
        "cloudsc2_abi_version": (c_int32, ()), "cloudsc2_params_sizeof": (c_int32, ()),
        "cloudsc2_last_error": (c_char_p, ()), "cloudsc2_last_kernel": (c_char_p, ()),
        "cloudsc2_device_count": (c_int32, ()), "cloudsc2_nl_taylor_blocks": (c_int32, (c_int32,)),
        "cloudsc2_field_sums_blocks": (c_int32, (c_int32, c_int32)), "cloudsc2_column_dots_chunks": (c_int32, (c_int32,)),
    }
    reduction = (c_int32, c_int32, c_int64, c_int32, _PARR, _PARR, c_void_p)
    # the masked TL / AD entries (autodiff.py calls them directly: NULL entries are not something a stencil call has)
    head = (POINTER(Cloudsc2Params), c_int32, c_int32, c_int64)
    tl_masked = head + (_PARR, _PARR, c_void_p, c_void_p, _PARR, _PARR, c_double, c_void_p)
    ad_masked = head + (_PARR, _PARR, c_void_p, c_void_p, c_void_p, c_void_p, _PARR, c_double, c_void_p)
    # the derivative rules of `saturation` and of the whole step (autodiff.py too): NULL fields again
    sat_tl = head + (c_void_p,) * 6 + (c_void_p,)
    sat_ad = head + (c_void_p,) * 5 + (c_int32, c_void_p)
    for sfx in ("f64", "f32"):
        sig[f"cloudsc2_tl_masked_{sfx}"] = (c_int32, tl_masked)
        sig[f"cloudsc2_ad_masked_{sfx}"] = (c_int32, ad_masked)
        sig[f"cloudsc2_tl_step_{sfx}"] = (c_int32, tl_masked)
        sig[f"cloudsc2_ad_step_{sfx}"] = (c_int32, ad_masked)
        for multi, single in MULTI_LAYOUTS.items():
            sig[f"cloudsc2_{multi}_{sfx}"] = (c_int32, sig[f"cloudsc2_{single}_{sfx}"][1] + (c_int32, c_int64, c_int64))
        for evap, base in EVAP_LAYOUTS.items():
            args = sig[f"cloudsc2_{base}_{sfx}"][1]
            extra = (c_void_p, c_int32)
            sig[f"cloudsc2_{evap}_{sfx}"] = (c_int32, args + extra if base in MULTI_LAYOUTS else args[:-1] + extra + args[-1:])
        sig[f"cloudsc2_saturation_tl_{sfx}"] = (c_int32, sat_tl)
        sig[f"cloudsc2_saturation_ad_{sfx}"] = (c_int32, sat_ad)
        sig[f"cloudsc2_field_sums_{sfx}"] = (c_int32, reduction + (c_void_p,))
        sig[f"cloudsc2_column_dots_{sfx}"] = (c_int32, reduction + (c_int32, c_void_p))
        for lay in LAYOUTS.values():
            sig[f"cloudsc2_{lay.entry}_{sfx}"] = (c_int32, (POINTER(Cloudsc2Params), c_int32, c_int32, c_int64)
                                                  + tuple(t for a in lay.args for t in _CTYPES[a.kind]))
        for ens, single in {**ENS_LAYOUTS, **EVAP_ENS_LAYOUTS}.items():
            sig[f"cloudsc2_{ens}_{sfx}"] = (c_int32, sig[f"cloudsc2_{single}_{sfx}"][1] + (c_int32, c_int64))
        for enss, ens in ENSS_LAYOUTS.items():
            sig[f"cloudsc2_{enss}_{sfx}"] = (c_int32, sig[f"cloudsc2_{ens}_{sfx}"][1] + (c_int64, c_int64))
        for ens, multi in MULTI_ENS_LAYOUTS.items():
            sig[f"cloudsc2_{ens}_{sfx}"] = (c_int32, sig[f"cloudsc2_{multi}_{sfx}"][1] + (c_int32, c_int64, c_int64, c_int64))
    return sig


SIGNATURES = _signatures()
#: every symbol include/cloudsc2_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = tuple(SIGNATURES)

_lib: Optional[ctypes.CDLL] = None


class Cloudsc2LibraryError(RuntimeError):
    pass


def _declare(lib: ctypes.CDLL) -> None:
    for symbol, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, symbol)
        fn.restype, fn.argtypes = restype, list(argtypes)


def load() -> ctypes.CDLL:
    """Load (once) and return the library; raises `Cloudsc2LibraryError` if it cannot be used."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Cloudsc2LibraryError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run `make -C gt4py_dwarf_p_cloudsc2_tl_ad_amd/csrc` or `__graft_entry__.build()`). "
            "There is no CPU fallback."
        )
    # torch ships its own libamdhip64 (same soname as /opt/rocm's): import it first so that the
    # kernels, torch's allocator and torch's streams all live in ONE HIP runtime.
    import torch  # noqa: F401

    try:
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    except OSError as exc:  # pragma: no cover - depends on the machine
        raise Cloudsc2LibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    missing = [s for s in EXPORTED_SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise Cloudsc2LibraryError(f"{LIB_PATH} lacks symbols {missing}: stale build, rebuild it")
    _declare(lib)
    if lib.cloudsc2_abi_version() != ABI_VERSION:
        raise Cloudsc2LibraryError(
            f"ABI version mismatch: library {lib.cloudsc2_abi_version()}, python {ABI_VERSION}"
        )
    if lib.cloudsc2_params_sizeof() != ctypes.sizeof(Cloudsc2Params):
        raise Cloudsc2LibraryError(
            f"Cloudsc2Params size mismatch: library {lib.cloudsc2_params_sizeof()}, "
            f"python {ctypes.sizeof(Cloudsc2Params)}"
        )
    _lib = lib
    return lib


def last_error() -> str:
    return load().cloudsc2_last_error().decode("utf-8", "replace")


def last_kernel() -> str:
    """Name of the kernel the last stencil call of this thread launched (diagnostics, e.g. for bench.py's record)."""
    return load().cloudsc2_last_kernel().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    """Map a C-ABI return code to the exception the reference's stencil call would raise."""
    if rc == 0:
        return
    msg = f"{what}: {last_error()} (code {rc})"
    if rc in (-1, -2):
        raise ValueError(msg)
    raise RuntimeError(msg)


def ptr_array(ptrs) -> ctypes.Array:
    return (c_void_p * len(ptrs))(*ptrs)
