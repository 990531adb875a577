"""CPU-side checks of the shared-state ensemble entries (C ABI `cloudsc2_*_enss_*`): the symbols exist in the header and the
library with the argtypes derived from the ensemble table, bad calls are refused on the host before any launch, each with
its message, the Python calls refuse what they document, and the new kernels' assembly passes the project's ISA guard."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NZ, LS = 64, 12, 64
FIELD = (NZ + 1) * LS


def test_symbols_and_derived_argtypes(hip_lib):
    from ctypes import c_int64

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    header = open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read()
    assert sorted(_lib.ENSS_LAYOUTS) == sorted(e.replace("_ens", "_enss") for e in _lib.ENS_LAYOUTS)
    for enss, ens in _lib.ENSS_LAYOUTS.items():
        for sfx in ("f64", "f32"):
            name = f"cloudsc2_{enss}_{sfx}"
            assert re.search(rf"\bint32_t\s+{name}\s*\(", header), name
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
            assert tuple(getattr(hip_lib, name).argtypes) == _lib.SIGNATURES[f"cloudsc2_{ens}_{sfx}"][1] + (c_int64, c_int64)
    assert f"CLOUDSC2_ENSS_COLUMN_MAJOR (INT64_C(1) << {_lib.ENSS_COLUMN_MAJOR.bit_length() - 1})" in header
    assert f"CLOUDSC2_ENSS_MEMBER_MAJOR (INT64_C(1) << {_lib.ENSS_MEMBER_MAJOR.bit_length() - 1})" in header


def _ad_step(hip_lib, mask, eta_ms, ins=None, outs=None, nmem=3, dt=3600.0, eta=4096):
    """a `cloudsc2_ad_step_enss_f64` call on pointers that are never dereferenced: every call here is refused on the host"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    p = make_params(dict(default_externals(), NLEV=NZ))
    base = 1 << 30
    ins = [base + i * 4 * FIELD * 8 for i in range(16)] if ins is None else ins
    outs = [base + (32 + i) * 4 * FIELD * 8 for i in range(16)] if outs is None else outs
    forcing = [base + (64 + i) * 4 * FIELD * 8 for i in range(10)]
    rc = hip_lib.cloudsc2_ad_step_enss_f64(ctypes.byref(p), NX, NZ, LS, _lib.ptr_array(ins), _lib.ptr_array(forcing), 4096, eta,
                                           4096, 4096, _lib.ptr_array(outs), dt, None, nmem, FIELD, mask, eta_ms)
    return rc, _lib.last_error()


def test_refusals_without_a_launch(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    qsat = _lib.NL_IN.index("qsat")
    base = 1 << 30
    ins = [base + i * 4 * FIELD * 8 for i in range(16)]
    ins[qsat] = 0
    rc, msg = _ad_step(hip_lib, 1 << qsat, 0, ins=ins)                      # a mask bit on a NULL field
    assert rc == -1 and f"in[{qsat}] is NULL" in msg and "cannot be shared" in msg, msg
    rc, msg = _ad_step(hip_lib, 1 << 16, 0)                                 # a bit beyond the family's count
    assert rc == -1 and "shared_mask bit 16" in msg and "beyond the 16 state inputs" in msg, msg
    rc, msg = _ad_step(hip_lib, _lib.ENSS_COLUMN_MAJOR | _lib.ENSS_MEMBER_MAJOR, 0)
    assert rc == -1 and "both block orders" in msg, msg
    for bad in (1, NZ, -1):                                                 # 0 < eta_member_stride < nz + 1
        rc, msg = _ad_step(hip_lib, 1, bad)
        assert rc == -1 and f"eta_member_stride={bad}" in msg and f"nz + 1 = {NZ + 1}" in msg, msg
    # a result that overlaps a shared input in member 2 of 3: out_adj[t] starts two member strides in front of in[ap]
    ap, t = _lib.NL_IN.index("ap"), _lib.NL_IN.index("t")
    outs = [base + (32 + i) * 4 * FIELD * 8 for i in range(16)]
    outs[qsat] = 0
    outs[t] = ins[ap] - 2 * FIELD * 8
    rc, msg = _ad_step(hip_lib, 1 << ap, 0, ins=ins, outs=outs)
    assert rc == -1 and f"out_adj[{t}] overlaps the shared input in[{ap}]" in msg, msg
    # the other side of the range arithmetic: these pass the overlap check and are refused by a LATER check (dt = 0), so
    # nothing launches.  Member 2 of out_adj[t] ends where in[ap] begins; out_adj[t] begins where in[ap] ends; three strides in
    # front no member reaches it; and with one member fewer the two-strides case is clear as well
    ext = (NZ * LS + NX) * 8                                                # bytes one member of a field spans
    for start, nmem in ((ins[ap] - 2 * FIELD * 8 - ext, 3), (ins[ap] + ext, 3), (ins[ap] - 3 * FIELD * 8, 3),
                        (ins[ap] - 2 * FIELD * 8, 2)):
        outs[t] = start
        rc, msg = _ad_step(hip_lib, 1 << ap, 0, ins=ins, outs=outs, nmem=nmem, dt=0.0)
        assert rc == -1 and "dt=0 must be > 0" in msg, (start - ins[ap], nmem, msg)
    for start in (ins[ap] - 2 * FIELD * 8 - ext + 8, ins[ap] + ext - 8):   # one element inside either end: refused as overlap
        outs[t] = start
        rc, msg = _ad_step(hip_lib, 1 << ap, 0, ins=ins, outs=outs, dt=0.0)
        assert rc == -1 and f"out_adj[{t}] overlaps the shared input in[{ap}]" in msg, (start - ins[ap], msg)
    # per-member eta rows are read for the whole launch too: a written field that reaches into them is refused
    outs[t] = base + (32 + t) * 4 * FIELD * 8
    eta = outs[t] + 2 * FIELD * 8 + 64                                      # inside member 2 of out_adj[t]
    rc, msg = _ad_step(hip_lib, 1 << ap, NZ + 1, ins=ins, outs=outs, dt=0.0, eta=eta)
    assert rc == -1 and f"out_adj[{t}] overlaps eta" in msg, msg
    rc, msg = _ad_step(hip_lib, 1 << ap, NZ + 1, ins=ins, outs=outs, dt=0.0, eta=outs[t] + 3 * FIELD * 8)   # behind member 2
    assert rc == -1 and "dt=0 must be > 0" in msg, msg
    # NL: qsat_out against a shared input
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    p = make_params(dict(default_externals(), NLEV=NZ))
    nl_out = [base + (32 + i) * 4 * FIELD * 8 for i in range(10)]
    rc = hip_lib.cloudsc2_nl_fused_enss_f64(ctypes.byref(p), NX, NZ, LS, _lib.ptr_array(ins), None, 0.0, ins[ap] - FIELD * 8, 4096,
                                            _lib.ptr_array(nl_out), 3600.0, None, 3, FIELD, 1 << ap, 0)
    assert rc == -1 and f"qsat_out[0] overlaps the shared input in[{ap}]" in _lib.last_error(), _lib.last_error()


def test_python_contract(hip_lib, monkeypatch):
    """a name in both `states` and `shared`, a wrong shape of a shared field, an `eta` with nmem - 1 rows: ValueError, each
    before anything is launched (host tensors stand in for device tensors up to the device check)"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff, storage

    nmem, nx, nz = 3, 8, 4
    names = autodiff.STEP_IN
    own = ("t", "q", "ql", "qi")
    states = {n: storage.zeros_batched(nmem, nx, nz, torch.float64, "cpu") for n in own}
    shared = {n: storage.zeros(nx, nz, torch.float64, "cpu") for n in names if n not in own}
    eta = torch.zeros(nz + 1, dtype=torch.float64)
    pert = {"t": states["t"]}
    with pytest.raises(ValueError, match="exactly one of `states` and `shared`.*in both \\['t'\\]"):
        autodiff.tl_step_ens(states, pert, eta, 3600.0, want=("tnd_t",), shared=dict(shared, t=shared["ap"]))
    with pytest.raises(ValueError, match="in neither \\['ap'\\]"):
        autodiff.tl_step_ens(states, pert, eta, 3600.0, want=("tnd_t",), shared={n: f for n, f in shared.items() if n != "ap"})
    with pytest.raises(ValueError, match="shared field ap must be a plain"):
        autodiff.tl_step_ens(states, pert, eta, 3600.0, want=("tnd_t",),
                             shared=dict(shared, ap=storage.zeros(nx + 1, nz, torch.float64, "cpu")))
    with pytest.raises(ValueError, match="exactly one of"):
        autodiff.cloudsc2_step_ensemble(states, eta, 3600.0, shared=dict(shared, q=shared["ap"]))
    with pytest.raises(ValueError, match="members for this call"):
        autodiff._call(autodiff._AD_STEP_EVAP, False, states, pert, eta, 3600.0, None, ("t",), traj={}, ens=True, shared=shared)
    assert autodiff._eta_members("x", torch.zeros(nmem, nz + 1, dtype=torch.float64), nz, nmem, torch.float64,
                                 torch.device("cpu"))[1] == nz + 1
    assert autodiff._eta_members("x", torch.zeros(nmem, nz + 9, dtype=torch.float64)[:, :nz + 1], nz, nmem, torch.float64,
                                 torch.device("cpu"))[1] == nz + 9
    with pytest.raises(ValueError, match="per-member eta must be a \\(3, >= 5\\)"):
        autodiff._eta_members("x", torch.zeros(nmem - 1, nz + 1, dtype=torch.float64), nz, nmem, torch.float64, torch.device("cpu"))


# ---- the compiled assembly of the new instantiations (csrc/check_ring_isa.py), as tests/test_ensemble_isa.py holds the others
sys.path.insert(0, os.path.join(ROOT, "gt4py_dwarf_p_cloudsc2_tl_ad_amd", "csrc"))
import check_ring_isa as isa  # noqa: E402

FAMILIES = {"nl_enss_kernelI": ("cloudsc2_nl.hip", 16), "tl_enss_kernelI": ("cloudsc2_tl.hip", 8),
            "tl_enss_step_kernelI": ("cloudsc2_tl.hip", 8), "ad_enss_kernelI": ("cloudsc2_ad.hip", 8),
            "ad_enss_step_kernelI": ("cloudsc2_ad.hip", 8)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("hipcc not available on this machine (the prebuilt library travelled with the snapshot)")
    out = str(tmp_path_factory.mktemp("isa"))
    return {src: isa.compile_to_asm(src, out) for src in ("cloudsc2_nl.hip", "cloudsc2_tl.hip", "cloudsc2_ad.hip")}


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_new_instantiations_no_scratch_and_prefetch(asm, prefix):
    src, count = FAMILIES[prefix]
    names = [n for n, _ in isa._kernels(asm[src], prefix)]
    assert len(names) == count and len(set(names)) == count, names
    for n in names:
        assert isa.kernel_resources(asm[src], n)["ScratchSize"] == 0, (n, "spills to scratch")
        assert isa.check_prefetch_distance(asm[src], n) >= 1, (n, "level loop not seen")
    # the twin: the ensemble kernel of the same template arguments - the same number of prefetch batches, no scratch either
    twin = prefix.replace("_enss_", "_ens_")
    for n in names:
        args = re.search(re.escape(prefix) + r"((?:[df]|Lb[01]E|Li\d+E)+)E", n)
        assert args, n
        twins = [k for k, _ in isa._kernels(asm[src], twin + args.group(1) + "E")]
        assert len(twins) == 1, (n, twins)
        assert isa.check_prefetch_distance(asm[src], n) == isa.check_prefetch_distance(asm[src], twins[0]), (n, twins[0])
        r, r0 = isa.kernel_resources(asm[src], n), isa.kernel_resources(asm[src], twins[0])
        print(f"{n}: {r}   twin: {r0}")
        # Occupancy is held to what the kernels ASK for in `__launch_bounds__`, as tests/test_ensemble_isa.py holds the
        # ensemble kernels: the fp32 instantiations ask for several waves per SIMD and must not fall below their twin; the
        # fp64 ones ask for one wave per SIMD (they are built for one), so any allocation up to the whole register file
        # meets it.  Two fp64 instantiations sit on that edge: nl_enss_kernel<double, EVAP=1, LIN=0, FUSE 0 and 1> take
        # 255 VGPRs + 2 AGPRs where their twins take exactly 256 + 0, which the compiler reports as occupancy 1 against 2
        # (printed above; every other instantiation reports its twin's occupancy or better).
        assert r["Occupancy"] >= (r0["Occupancy"] if args.group(1)[0] == "f" else 1), (n, r, r0)
