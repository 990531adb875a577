"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every
symbol include/cloudsc2_hip.h declares; argument validation rejects bad calls before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    header = open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read()
    declared = set(re.findall(r"\b(cloudsc2_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    for s in declared:
        assert hasattr(hip_lib, s), s


def test_header_prototypes_match_the_declared_argtypes(hip_lib):
    """Argument types AND their order: every `int32_t cloudsc2_*_f64(...)` prototype of the header, read as text, against
    the `argtypes` the loaded library carries (derived from `_lib.LAYOUTS`), for both suffixes.  The header's types alone
    do not tell a host array (`pf`) from a device array (`eta`), so "a pointer" is satisfied by `c_void_p` or
    `POINTER(c_double)`; everything else must match exactly."""
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import Cloudsc2Params

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read(), flags=re.S)
    protos = re.findall(r"int32_t\s+(cloudsc2_\w+)_f64\s*\(([^)]*)\)\s*;", header)
    assert len(protos) >= 12, protos
    any_pointer = (c_void_p, POINTER(c_double))

    def kind(param):
        ctype = " ".join(param.split()[:-1]) if not param.strip().endswith("*") else " ".join(param.split())
        ctype = re.sub(r"\s*\*\s*", "* ", ctype).strip()          # "const double* const*", "void*", "double"
        if ctype == "const Cloudsc2Params*":
            return (POINTER(Cloudsc2Params),)
        if ctype in ("int32_t", "int64_t", "double"):
            return ({"int32_t": c_int32, "int64_t": c_int64, "double": c_double}[ctype],)
        if re.fullmatch(r"(const )?(double|float)\* const\*", ctype):
            return (POINTER(c_void_p),)
        assert ctype.endswith("*") and "* " not in ctype[:-1], f"unrecognised parameter type {ctype!r}"
        return any_pointer

    for base, params in protos:
        want = [kind(x) for x in params.split(",")]
        for sfx in ("f64", "f32"):
            fn = getattr(hip_lib, f"{base}_{sfx}")
            assert fn.restype is c_int32
            got = list(fn.argtypes)
            assert len(got) == len(want), (base, sfx, got)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g in w, f"{base}_{sfx}: argument {i} is declared {g}, the header says {params.split(',')[i].strip()!r}"


def test_params_struct_matches(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import ABI_VERSION, Cloudsc2Params

    assert hip_lib.cloudsc2_abi_version() == ABI_VERSION
    assert hip_lib.cloudsc2_params_sizeof() == ctypes.sizeof(Cloudsc2Params)
    header = open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read()
    body = header[header.index("typedef struct Cloudsc2Params {"):header.index("} Cloudsc2Params;")]
    names = []
    for line in body.splitlines()[1:]:
        line = line.split("/*")[0].strip().rstrip(";")
        if line.startswith(("double", "int32_t")):
            names += [n.strip() for n in line.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in Cloudsc2Params._fields_]


def test_bad_arguments_are_rejected_without_launch(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    p = make_params(default_externals())
    null = _lib.ptr_array([0] * 16)
    nullo = _lib.ptr_array([0] * 10)
    rc = hip_lib.cloudsc2_nl_f64(ctypes.byref(p), 64, 137, 64, null, 0, nullo, 3600.0, None)
    assert rc == -1 and "NULL" in _lib.last_error()
    rc = hip_lib.cloudsc2_nl_f64(ctypes.byref(p), -5, 137, 64, null, 0, nullo, 3600.0, None)
    assert rc == -1 and "nx" in _lib.last_error()
    rc = hip_lib.cloudsc2_nl_f64(ctypes.byref(p), 64, 137, 32, null, 0, nullo, 3600.0, None)
    assert rc == -1 and "lev_stride" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "cloudsc2_nl")


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.Cloudsc2LibraryError):
        _lib.load()
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

    with pytest.raises(_lib.Cloudsc2LibraryError):
        compile_stencil("cloudsc2_nl", {})


def test_stencil_rejects_cpu_tensors(hip_lib):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import compile_stencil

    st = compile_stencil("saturation", {})
    a = storage.zeros(8, 4, torch.float64, "cpu")
    with pytest.raises(ValueError, match="GPU"):
        st(in_ap=a, in_t=a, out_qsat=a, origin=(0, 0, 0), domain=(8, 1, 4), validate_args=True, exec_info=None)
    with pytest.raises(ValueError, match="domain"):
        st(in_ap=a, in_t=a, out_qsat=a, origin=(0, 0, 0), domain=(8, 1, 5), validate_args=True, exec_info=None)
    with pytest.raises(KeyError):
        compile_stencil("no_such_stencil", {})


def test_size_limits_and_empty_calls(hip_lib):
    """Edge sizes are settled on the host, before any launch.  Fields beyond 4 GiB (r04): the plain stencils accept them
    (their 64-bit-offset instantiation; without a GPU the call then ends in a launch / no-device error, never in
    CLOUDSC2_E_UNSUPPORTED), the fused build extensions keep 32-bit byte offsets and refuse them with a message that says
    what to do; nx = 0 is a successful no-op."""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    p = make_params(dict(default_externals(), NLEV=137))
    ins, ins_i = _lib.ptr_array([4096] * 16), _lib.ptr_array([4096] * 16)      # never dereferenced on these paths
    outs, outs_i = _lib.ptr_array([4096] * 10), _lib.ptr_array([4096] * 10)
    big = 4_000_000                                                              # x 138 levels x 8 B > 2^32
    import torch

    if not torch.cuda.is_available():      # (with a GPU these would really launch on the dummy pointers)
        assert hip_lib.cloudsc2_nl_f64(ctypes.byref(p), big, 137, big, ins, 4096, outs, 3600.0, None) not in (0, -2)
        assert hip_lib.cloudsc2_tl_f64(ctypes.byref(p), big, 137, big, ins, ins_i, 4096, outs, outs_i, 3600.0, None) not in (0, -2)
        assert hip_lib.cloudsc2_ad_f64(ctypes.byref(p), big, 137, big, ins, outs, 4096, outs, ins_i, 3600.0, None) not in (0, -2)
    # perturbed_state fused into NL, state_increment fused into TL: 32-bit offsets, refused before anything is launched
    assert hip_lib.cloudsc2_nl_fused_f64(ctypes.byref(p), big, 137, big, ins, ins_i, 0.01, None, 4096, outs, 3600.0, None) == -2
    assert "2^32" in _lib.last_error() and "cloudsc2_nl / _tl / _ad have no such limit" in _lib.last_error()
    assert hip_lib.cloudsc2_tl_incremented_f64(ctypes.byref(p), big, 137, big, ins, 0.01, 4096, outs, outs_i, 3600.0, None) == -2
    with pytest.raises(ValueError, match="2\\^32"):
        _lib.check(-2, "cloudsc2_nl_fused")
    # fp32 halves the footprint: the same shape is accepted by the size check (and would launch on a GPU)
    for fn, args in (("cloudsc2_nl_f64", (ins, 4096, outs, 3600.0, None)),
                     ("cloudsc2_tl_f64", (ins, ins_i, 4096, outs, outs_i, 3600.0, None)),
                     ("cloudsc2_ad_f64", (ins, outs, 4096, outs, ins_i, 3600.0, None)),
                     ("cloudsc2_saturation_f64", (4096, 4096, 4096, None)),
                     ("cloudsc2_state_increment_f64", (ins, ins_i, 0.01, None)),
                     ("cloudsc2_perturbed_state_f64", (ins, ins_i, ins, 0.001, None))):
        assert getattr(hip_lib, fn)(ctypes.byref(p), 0, 137, 64, *args) == 0, fn


def test_stencil_call_signature_errors(hip_lib):
    """The stencil objects keep the GT4Py call discipline: keyword arguments by gtscript parameter name, scalars present,
    nothing unknown, `tmp_*` scratch arguments accepted and ignored, mismatched storages refused - all before any launch."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import INC, NL_IN, NL_OUT, compile_stencil

    nx, nz = 8, 4
    z = lambda: storage.zeros(nx, nz, torch.float64, "cpu")  # noqa: E731
    eta = torch.zeros(nz + 1, dtype=torch.float64)
    nl = compile_stencil("cloudsc2_nl", {"NLEV": nz})
    good = {**{"in_" + n: z() for n in NL_IN}, **{"out_" + n: z() for n in NL_OUT}}
    com = dict(in_eta=eta, origin=(0, 0, 0), domain=(nx, 1, nz + 1), validate_args=True, exec_info=None)
    with pytest.raises(TypeError, match="in_qsat"):
        nl(**{k: v for k, v in good.items() if k != "in_qsat"}, dt=3600.0, **com)
    with pytest.raises(TypeError, match="dt"):
        nl(**good, **com)
    with pytest.raises(TypeError, match="unexpected"):
        nl(**good, dt=3600.0, in_bogus=z(), **com)
    with pytest.raises(ValueError, match="origin"):
        nl(**good, dt=3600.0, **{**com, "origin": (1, 0, 0)})
    # scratch arguments of the gtscript signature are accepted (and never touched): the call gets as far as the device check
    with pytest.raises(ValueError, match="GPU"):
        nl(**good, dt=3600.0, tmp_aph_s=None, tmp_covptot=None, tmp_rfl=None, tmp_sfl=None, tmp_trpaus=None, **com)
    inc = compile_stencil("state_increment", {"IGNORE_SUPSAT": True})
    with pytest.raises(TypeError, match="'f'"):
        inc(**{"in_" + n: z() for n in INC}, **{"out_" + n + "_i": z() for n in INC}, origin=(0, 0, 0),
            domain=(nx, 1, nz + 1), validate_args=True, exec_info=None)


def test_outputs_must_not_alias_other_fields(hip_lib):
    """Debug check of validate_args=True (SURVEY.md 5 "race detection"): an output that shares storage with another
    field of the same call is refused before anything is launched; column windows of ONE allocation that merely
    interleave (lev_stride > nx) are legal."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import NL_IN, NL_OUT, _windows_overlap, compile_stencil

    # the window arithmetic: nx = 4 columns, 3 levels, level stride 10 elements of 8 bytes
    assert _windows_overlap(1000, 1000, 8, 4, 3, 10)
    assert _windows_overlap(1000, 1000 + 3 * 8, 8, 4, 3, 10)              # columns [0,4) and [3,7): share column 3
    assert not _windows_overlap(1000, 1000 + 4 * 8, 8, 4, 3, 10)          # columns [0,4) and [4,8): disjoint windows
    assert not _windows_overlap(1000 + 4 * 8, 1000, 8, 4, 3, 10)
    assert _windows_overlap(1000, 1000 + 10 * 8, 8, 4, 3, 10)             # shifted by one level: levels 1,2 shared
    assert not _windows_overlap(1000, 1000 + 30 * 8, 8, 4, 3, 10)         # shifted by all 3 levels: disjoint
    assert _windows_overlap(1000, 1000 + 4, 8, 4, 3, 10)                  # misaligned pair: byte ranges decide
    nx, nz = 8, 4
    z = lambda: storage.zeros(nx, nz, torch.float64, "cpu")  # noqa: E731
    nl = compile_stencil("cloudsc2_nl", {"NLEV": nz})
    good = {**{"in_" + n: z() for n in NL_IN}, **{"out_" + n: z() for n in NL_OUT}}
    nl._check_disjoint(good, nx, nz + 1, nx, 8)                           # distinct storages pass
    with pytest.raises(ValueError, match="out_tnd_t.*overlaps.*in_t"):
        nl._check_disjoint({**good, "out_tnd_t": good["in_t"]}, nx, nz + 1, nx, 8)            # in-place update
    with pytest.raises(ValueError, match="overlaps"):
        nl._check_disjoint({**good, "out_clc": good["out_covptot"]}, nx, nz + 1, nx, 8)       # two outputs, one buffer
    # two windows of one allocation: columns [0, 8) and [8, 16) with lev_stride 16 interleave but never touch
    # (every field of a call shares ONE level stride - HipStencil._geometry refuses anything else - so the other fields
    # of this call are windows of 2*nx-wide buffers too: judging a dense field by a stride that is not its own makes the
    # verdict depend on where malloc happened to put it)
    big = torch.zeros((nz + 1, 2 * nx), dtype=torch.float64)
    wa, wb = storage.logical_view(big[:, :nx]), storage.logical_view(big[:, nx:])
    wide = {n: storage.logical_view(torch.zeros((nz + 1, 2 * nx), dtype=torch.float64)[:, :nx]) for n in good}
    nl._check_disjoint({**wide, "in_t": wa, "out_tnd_t": wb}, nx, nz + 1, 2 * nx, 8)
    with pytest.raises(ValueError, match="overlaps"):
        nl._check_disjoint({**wide, "in_t": wa, "out_tnd_t": storage.logical_view(big[:, nx - 1:2 * nx - 1])},
                           nx, nz + 1, 2 * nx, 8)                                           # windows share column nx-1
    ad = compile_stencil("cloudsc2_ad", {"NLEV": nz})
    ad_fields = {**{"in_" + n: z() for n in NL_IN}, **{"in_" + n + "_i": z() for n in NL_OUT},
                 **{"out_" + n: z() for n in NL_OUT}, **{"out_" + n + "_i": z() for n in NL_IN}}
    ad._check_disjoint(ad_fields, nx, nz + 1, nx, 8)
    with pytest.raises(ValueError, match="out_tnd_t'? overlaps"):                              # AD re-reads its forcing
        ad._check_disjoint({**ad_fields, "out_tnd_t": ad_fields["in_tnd_t_i"]}, nx, nz + 1, nx, 8)


def test_nlev_external_must_match_the_storages(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import STENCILS, checked_nlev, compile_stencil

    assert [n for n, c in STENCILS.items() if c.layout.sets_nlev] == [
        "cloudsc2_tl", "cloudsc2_tl_incremented", "cloudsc2_ad", "cloudsc2_ad_from_trajectory"]
    tl = compile_stencil("cloudsc2_tl", {"NLEV": 137})
    assert checked_nlev(tl.name, tl.externals, 137, True) == 137
    with pytest.raises(ValueError, match="NLEV=137 does not match"):
        checked_nlev(tl.name, tl.externals, 90, True)
    # validate_args=False: the storages decide (the kernels' bounds depend on it)
    assert checked_nlev(tl.name, tl.externals, 90, False) == 90
    ad = compile_stencil("cloudsc2_ad", {})     # no NLEV given: derived from the storages
    assert checked_nlev(ad.name, ad.externals, 60, True) == 60


def test_nlev_reaches_the_params_struct(hip_lib, monkeypatch):
    """what `checked_nlev` returns is what the kernel is given: a call (host storages, the entry point replaced by a
    function that returns 0) leaves it in `params.NLEV`, whether the external was absent or disagreed"""
    import contextlib

    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import stencils, storage
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import NL_IN, NL_OUT, compile_stencil

    monkeypatch.setattr(stencils, "_current_stream_ptr", lambda device: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())

    def call(st, nz, names):
        seen = []
        st._entry = {dt: (lambda *a: seen.append(a[0]._obj.NLEV) or 0) for dt in st._entry}
        st(**{n: storage.zeros(8, nz, torch.float64, "cpu") for n in names}, in_eta=torch.zeros(nz + 1, dtype=torch.float64),
           dt=3600.0, origin=(0, 0, 0), domain=(8, 1, nz + 1), validate_args=False, exec_info=None)
        return seen

    ad = compile_stencil("cloudsc2_ad", {})     # no NLEV given: derived from the storages
    ad_names = (["in_" + n for n in NL_IN] + ["in_" + n + "_i" for n in NL_OUT] + ["out_" + n for n in NL_OUT]
                + ["out_" + n + "_i" for n in NL_IN])
    assert call(ad, 60, ad_names) == [60] and ad.params.NLEV == 60
    tl = compile_stencil("cloudsc2_tl", {"NLEV": 137})
    tl_names = (["in_" + n for n in NL_IN] + ["in_" + n + "_i" for n in NL_IN] + ["out_" + n for n in NL_OUT]
                + ["out_" + n + "_i" for n in NL_OUT])
    assert tl.params.NLEV == 137
    assert call(tl, 90, tl_names) == [90] and tl.params.NLEV == 90      # validate_args=False: the storages decide


def test_level_limit_is_an_argument_error_not_a_launch_failure(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    p = make_params(dict(default_externals(), NLEV=4096))
    ins, outs = _lib.ptr_array([4096] * 16), _lib.ptr_array([4096] * 10)
    assert hip_lib.cloudsc2_nl_f64(ctypes.byref(p), 64, 4096, 64, ins, 4096, outs, 3600.0, None) == -1
    assert "nz=4096" in _lib.last_error()
    assert isinstance(_lib.last_kernel(), str)   # diagnostics entry point answers without a launch ("" then)
