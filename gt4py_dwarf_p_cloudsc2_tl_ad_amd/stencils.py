"""Stencil objects of the MI355X build: the counterpart of what the reference obtains from
``self.compile_stencil(name, externals)`` (nonlinear/microphysics.py:79, tangent_linear/microphysics.py:92,
adjoint/microphysics.py:89, common/saturation.py:54, common/increment.py:47-49,146 under
/root/reference/src/cloudsc2_gt4py/physics/).

A stencil object is called exactly like a GT4Py `StencilObject`: keyword field arguments named as
in the gtscript signature, then ``dt=`` (or ``f=``), ``origin=``, ``domain=``, ``validate_args=``,
``exec_info=``; it returns ``None`` and writes its outputs in place.  Each call is one launch of a
hand-written gfx950 kernel through the C ABI of libcloudsc2_hip.so.  There is no CPU path: without
the library (or without a GPU) the call raises.

Error behaviour mirrors GT4Py's: argument problems found with ``validate_args=True`` raise
`ValueError` / `TypeError` before anything is launched; launch failures raise `RuntimeError`.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Mapping, Optional

import torch

from . import _lib
from ._lib import INC, LAYOUTS, NL_IN, NL_OUT, Layout  # noqa: F401 - the field lists are part of this module's API
from .params import make_params
from .storage import field_geometry

_SFX = {torch.float64: "f64", torch.float32: "f32"}

#: scratch / bookkeeping arguments of the gtscript signatures that the native kernels keep in
#: registers (accepted for call compatibility, never touched)
_IGNORED_PREFIX = "tmp_"


def _windows_overlap(pa: int, pb: int, itemsize: int, nx: int, nlev: int, ls: int) -> bool:
    """Do two [level][column] windows (nx columns, nlev levels, level stride ls elements) that start at byte
    addresses pa / pb share an element?  Exact for windows of one allocation (column windows with lev_stride > nx
    interleave without touching); a misaligned pair is judged by its byte ranges."""
    d = pb - pa
    if d % itemsize:
        span = ((nlev - 1) * ls + nx) * itemsize
        return pa < pb + span and pb < pa + span
    q, r = divmod(d // itemsize, ls)            # d = q * ls + r, 0 <= r < ls
    return (r < nx and abs(q) < nlev) or (ls - r < nx and abs(q + 1) < nlev)


def _current_stream_ptr(device: torch.device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def checked_nlev(name: str, externals: Mapping[str, Any], nz: int, validate: bool) -> int:
    """`NLEV` is an external of the TL / AD stencils (tangent_linear/microphysics.py:85: the grid's nz).  When the
    caller supplied one it must agree with the storages (checked with validate_args=True; otherwise the storages
    win, as they must for the kernels' bounds); when it did not, it is derived from them."""
    given = externals.get("NLEV")
    if given is not None and int(given) != nz and validate:
        raise ValueError(f"{name}: external NLEV={int(given)} does not match the storages (nz={nz})")
    return nz


class HipStencil:
    """The callable stencil object: a function of its externals and of its entry in `_lib.LAYOUTS` (one subclass per
    entry, made by `_stencil_class`).  Nothing of a call is kept on the object but the memo of the disjointness check."""

    name: str = ""
    layout: Layout = Layout("", ())
    scalar_name: str = "dt"   # the stencil's own scalar: the last keyword scalar of the layout ("" if there is none)
    nlev_offset: int = 1      # domain[2] = nz + nlev_offset
    # derived from the layout, once per stencil (`_stencil_class`)
    _kinds: frozenset = frozenset()
    _scalars: tuple = ()        # the keyword scalars
    _field_groups: tuple = ()   # (scalar keyword that replaces the group or None, field keywords), in layout order

    def __init__(self, externals: Mapping[str, Any]):
        self.externals = dict(externals)
        self.params = make_params(self.externals)
        self._lib = _lib.load()  # raises if the HIP library is missing: no fallback
        self._entry = {dtype: getattr(self._lib, f"cloudsc2_{self.layout.entry}_{sfx}") for dtype, sfx in _SFX.items()}

    # -- argument handling ---------------------------------------------------------------
    def _geometry(self, fields: Mapping[str, torch.Tensor], domain, origin, validate: bool):
        first = next(iter(fields.values()))
        nx, nlev, ls = field_geometry(first)
        nz = nlev - 1
        if origin is not None and tuple(origin) != (0, 0, 0):
            raise ValueError(f"{self.name}: only origin=(0, 0, 0) is supported, got {tuple(origin)}")
        if domain is not None:
            d = tuple(int(x) for x in domain)
            if d != (nx, 1, nz + self.nlev_offset):
                raise ValueError(
                    f"{self.name}: domain {d} does not match the storages "
                    f"(expected {(nx, 1, nz + self.nlev_offset)})"
                )
        if validate:
            dev, dt = first.device, first.dtype
            if dev.type != "cuda":
                raise ValueError(f"{self.name}: fields must live on the GPU, got device {dev}")
            if dt not in _SFX:
                raise TypeError(f"{self.name}: unsupported dtype {dt}")
            for n, f in fields.items():
                if not isinstance(f, torch.Tensor):
                    raise TypeError(f"{self.name}: argument {n} is not a torch.Tensor")
                if f.device != dev or f.dtype != dt:
                    raise TypeError(f"{self.name}: argument {n} has device/dtype {f.device}/{f.dtype}, "
                                    f"expected {dev}/{dt}")
                g = field_geometry(f)
                if g != (nx, nlev, ls):
                    raise ValueError(f"{self.name}: argument {n} has (nx, nlev, lev_stride) = {g}, "
                                     f"expected {(nx, nlev, ls)}")
            self._check_disjoint(fields, nx, nlev, ls, first.element_size())
        elif nlev > 1:
            # ALWAYS checked, validate_args or not (a few microseconds): the C ABI takes ONE level stride for every field of
            # the call, and storages may carry a padded level pitch (storage.level_pitch) - a field allocated another way
            # (a dense torch tensor beside storage.zeros fields at a ragged nx) would be addressed with the wrong stride
            for n, f in fields.items():
                if f.stride(2) != ls:
                    raise ValueError(f"{self.name}: argument {n} has level stride {f.stride(2)}, the call's is {ls} - "
                                     "allocate every field of a call the same way (storage.zeros / storage.from_klayout)")
        return nx, nz, ls, first.dtype, first.device

    def _check_disjoint(self, fields: Mapping[str, torch.Tensor], nx: int, nlev: int, ls: int, itemsize: int) -> None:
        """Debug check (validate_args=True): an output of a call must not share storage with any other field of the
        same call.  The kernels stream level by level and cloudsc2_ad re-reads its inputs in the backward sweep, so an
        in-place call would silently compute from overwritten data (SURVEY.md 5 "race detection"; the reference's
        drivers never alias inputs and outputs of one call, adjoint/validation.py:149-150 rebinds TL outputs as AD
        *inputs* only)."""
        if nx == 0:
            return
        ptrs = {n: f.data_ptr() for n, f in fields.items()}
        # the O(n^2) window test (26 outputs x 72 fields for cloudsc2_ad: ~1 ms of host Python) runs once per distinct set
        # of storages; the drivers call a stencil on the same storages run after run
        key = (tuple(ptrs.items()), nx, nlev, ls, itemsize)
        seen = self.__dict__.setdefault("_disjoint_ok", set())
        if key in seen:
            return
        outs = [n for n in fields if n.startswith("out_")]
        for o in outs:
            for n, p in ptrs.items():
                if n == o or (n in outs and n < o):      # every unordered pair once
                    continue
                if _windows_overlap(ptrs[o], p, itemsize, nx, nlev, ls):
                    raise ValueError(f"{self.name}: output '{o}' overlaps '{n}' in memory - inputs and outputs of "
                                     "one call must be disjoint storages")
        if len(seen) >= 64:
            seen.clear()
        seen.add(key)

    def _kvec(self, v: Any, nz: int, dtype, device, validate: bool) -> torch.Tensor:
        if validate:
            if not isinstance(v, torch.Tensor) or v.dim() != 1 or v.shape[0] < nz + 1:
                raise ValueError(f"{self.name}: in_eta must be a 1-D tensor with >= {nz + 1} entries")
            if v.dtype != dtype or v.device != device or not v.is_contiguous():
                raise TypeError(f"{self.name}: in_eta must be contiguous {dtype} on {device}")
        return v

    def __call__(self, **kwargs: Any) -> None:
        origin = kwargs.pop("origin", None)
        domain = kwargs.pop("domain", None)
        validate = bool(kwargs.pop("validate_args", True))
        exec_info: Optional[dict] = kwargs.pop("exec_info", None)
        scalars: Dict[str, Optional[float]] = {}
        for a in self._scalars:
            v = kwargs.pop(a.key, None)
            if v is None and a.default is None:
                raise TypeError(f"{self.name}: missing scalar argument '{a.key}'")
            scalars[a.key] = None if v is None else float(v)
        fs = part = None
        if "fs" in self._kinds:
            if "fs" not in kwargs:
                raise TypeError(f"{self.name}: missing argument 'fs'")
            fs = [float(x) for x in kwargs.pop("fs")]
        if "partials" in self._kinds:
            if "out_partials" not in kwargs:
                raise TypeError(f"{self.name}: missing argument 'out_partials'")
            part = kwargs.pop("out_partials")
        eta = kwargs.pop("in_eta", None)
        fields: Dict[str, torch.Tensor] = {}
        try:
            for unless, names in self._field_groups:
                if unless is None or scalars[unless] is None:
                    for n in names:
                        fields[n] = kwargs.pop(n)
        except KeyError:
            raise TypeError(f"{self.name}: missing field argument '{n}'") from None
        if kwargs:
            unexpected = sorted(n for n in kwargs if not n.startswith(_IGNORED_PREFIX))
            if unexpected:
                raise TypeError(f"{self.name}: unexpected arguments {unexpected}")
        nx, nz, ls, dtype, device = self._geometry(fields, domain, origin, validate)
        if "eta" in self._kinds:
            if eta is None:
                raise TypeError(f"{self.name}: missing field argument 'in_eta'")
            eta = self._kvec(eta, nz, dtype, device, validate)
        if part is not None:
            need = taylor_blocks(nx) * (1 if fs is None else len(fs)) * len(NL_OUT)
            if (not isinstance(part, torch.Tensor) or part.dtype != torch.float64 or not part.is_contiguous()
                    or part.device != device or part.numel() < need):
                raise ValueError(f"{self.name}: out_partials must be a contiguous float64 device tensor with >= {need} "
                                 f"elements (taylor_blocks(nx) x [len(fs) x] {len(NL_OUT)})")
        if self.layout.sets_nlev:
            self.params.NLEV = checked_nlev(self.name, self.externals, nz, validate)
        ev = None
        if exec_info is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        with torch.cuda.device(device):
            c_args: list = [ctypes.byref(self.params), nx, nz, ls]
            for kind, key, unless, default in self.layout.args:
                if kind == "ptrs":
                    absent = not key or (unless is not None and scalars[unless] is not None)
                    c_args.append(None if absent else _lib.ptr_array([fields[n].data_ptr() if n else 0 for n in key]))
                elif kind == "field":
                    c_args.append(fields[key].data_ptr() if key else None)
                elif kind == "scalar":
                    v = scalars[key] if key else None
                    c_args.append(default if v is None else v)
                elif kind == "eta":
                    c_args.append(eta.data_ptr())
                elif kind == "partials":
                    c_args.append(part.data_ptr())
                elif kind == "fs":
                    c_args += [len(fs), (ctypes.c_double * max(len(fs), 1))(*fs)]
                else:
                    c_args.append(_current_stream_ptr(device))
            rc = self._entry[dtype](*c_args)
        _lib.check(rc, self.name)
        if ev is not None:
            ev[1].record()
            rec = exec_info.setdefault(self.name, {"ncalls": 0, "events": []})
            rec["ncalls"] += 1
            rec["events"].append(ev)


def taylor_blocks(nx: int) -> int:
    """Number of per-workgroup partial rows `cloudsc2_nl_taylor` writes for nx columns."""
    return int(_lib.load().cloudsc2_nl_taylor_blocks(int(nx)))


def _stencil_class(name: str, layout: Layout) -> type:
    scalars = tuple(a for a in layout.args if a.kind == "scalar" and a.key)
    groups: list = []           # runs of field keywords that are present or absent together
    for a in layout.args:
        if a.kind in ("ptrs", "field"):
            names = tuple(n for n in (a.key if a.kind == "ptrs" else (a.key,)) if n)
            if groups and groups[-1][0] == a.unless:
                groups[-1] = (a.unless, groups[-1][1] + names)
            elif names:
                groups.append((a.unless, names))
    return type("".join(w.capitalize() for w in name.split("_")) + "Stencil", (HipStencil,), {
        "name": name, "layout": layout, "nlev_offset": layout.nlev_offset,
        "scalar_name": scalars[-1].key if scalars else "", "_kinds": frozenset(a.kind for a in layout.args),
        "_scalars": scalars, "_field_groups": tuple(groups),
        "__doc__": f"`{name}`: see its entry in `_lib.LAYOUTS`."})


#: registry keyed by the names the reference registers with `@stencil_collection(name)` (+ the build extensions)
STENCILS: Dict[str, type] = {name: _stencil_class(name, layout) for name, layout in LAYOUTS.items()}


def compile_stencil(name: str, externals: Optional[Mapping[str, Any]] = None) -> HipStencil:
    """Counterpart of the components' ``self.compile_stencil(name, externals)``.

    Nothing is compiled at run time: the externals select a prebuilt kernel instantiation
    (boolean switches) and fill the `Cloudsc2Params` struct (numeric values); unknown externals are
    ignored, as GT4Py ignores externals a stencil does not import."""
    try:
        cls = STENCILS[name]
    except KeyError:
        raise KeyError(f"unknown stencil '{name}'; available: {sorted(STENCILS)}") from None
    return cls(externals or {})


def finalize_exec_info(exec_info: Optional[dict]) -> None:
    """Resolve the recorded HIP events into `total_run_time` (seconds) per stencil."""
    if not exec_info:
        return
    if not any(isinstance(r, dict) and r.get("events") for r in exec_info.values()):
        return
    torch.cuda.synchronize()
    for rec in exec_info.values():
        if isinstance(rec, dict) and "events" in rec:
            tot = rec.get("total_run_time", 0.0)
            for a, b in rec["events"]:
                tot += a.elapsed_time(b) * 1e-3
            rec["total_run_time"] = tot
            rec["events"] = []
