"""The whole Python path from a component call to the C ABI, pinned as a trace (CPU only, no built library needed).

A recorder (this file, run as a subprocess because the fakes of tests/run_reference_on_recording_hip.py monkey-patch
`torch.cuda`) calls

  1. every stencil of `stencils.STENCILS`, in both dtypes, directly on host storages with `validate_args=False` - the build
     extensions with their extra keywords, `cloudsc2_nl_taylor_multi` in both of its call shapes (`in_*_i` fields, `f_inc`);
  2. the three in-repo drivers end to end on 64 synthetic columns, under every flag set of `DRIVER_RUNS`;

and records, per stencil call, what `recording_call` sees (keyword names, scalar values and their Python type, origin,
domain, validate_args, the integer externals, the geometry of every field) and the C-ABI calls it produced (entry point,
every positional argument, the `Cloudsc2Params` fields).  Data pointers are replaced by the keyword under which the
storage was passed (`null` for NULL), so the trace does not depend on where malloc put things.  On host tensors the
validation reductions take their host path and do not appear.

The trace must equal tests/golden/abi_trace.json as a whole.  The fixture is written by `python tests/test_abi_trace.py
--regenerate`; it was generated before the binding layer was made table-driven and is not to be regenerated for a change
that claims to leave the call path as it is."""
import contextlib
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_trace.json")

# this test's own statement of the field lists (C-ABI order does not matter here: they only name keywords)
NL_IN = ("ap", "aph", "lu", "lude", "mfd", "mfu", "q", "qi", "ql", "qsat", "supsat", "t",
         "tnd_cml_q", "tnd_cml_qi", "tnd_cml_ql", "tnd_cml_t")
NL_OUT = ("clc", "covptot", "fhpsl", "fhpsn", "fplsl", "fplsn", "tnd_q", "tnd_qi", "tnd_ql", "tnd_t")
INC = ("aph", "ap", "q", "qsat", "t", "ql", "qi", "lude", "lu", "mfu", "mfd",
       "tnd_cml_t", "tnd_cml_q", "tnd_cml_ql", "tnd_cml_qi", "supsat")


def _names(fmt, base):
    return [fmt.format(n) for n in base]


#: stencil -> list of call shapes: (field keywords, needs in_eta, scalar keywords, extra: "partials" / "partials_fs")
DIRECT_CALLS = {
    "cloudsc2_nl": [(_names("in_{}", NL_IN) + _names("out_{}", NL_OUT), True, {"dt": 3600.0}, None)],
    "cloudsc2_nl_saturation": [([n for n in _names("in_{}", NL_IN) if n != "in_qsat"] + ["out_qsat"]
                                + _names("out_{}", NL_OUT), True, {"dt": 3600.0}, None)],
    "cloudsc2_nl_perturbed": [(_names("in_{}", NL_IN) + _names("in_{}_i", NL_IN) + _names("out_{}", NL_OUT), True,
                               {"dt": 3600.0, "f": 0.125}, None)],
    "cloudsc2_nl_taylor": [(_names("in_{}", NL_IN) + _names("in_{}_i", NL_IN) + _names("ref_{}", NL_OUT), True,
                            {"dt": 3600.0, "f": 0.125}, "partials")],
    "cloudsc2_nl_taylor_multi": [
        (_names("in_{}", NL_IN) + _names("in_{}_i", NL_IN) + _names("ref_{}", NL_OUT), True, {"dt": 3600.0}, "partials_fs"),
        (_names("in_{}", NL_IN) + _names("ref_{}", NL_OUT), True, {"dt": 3600.0, "f_inc": 0.25}, "partials_fs"),
        # and again with the fields: what a call accepts must not depend on the call before it
        (_names("in_{}", NL_IN) + _names("in_{}_i", NL_IN) + _names("ref_{}", NL_OUT), True, {"dt": 3600.0}, "partials_fs"),
    ],
    "cloudsc2_tl": [(_names("in_{}", NL_IN) + _names("in_{}_i", NL_IN) + _names("out_{}", NL_OUT)
                     + _names("out_{}_i", NL_OUT), True, {"dt": 3600.0}, None)],
    "cloudsc2_tl_incremented": [(_names("in_{}", NL_IN) + _names("out_{}", NL_OUT) + _names("out_{}_i", NL_OUT), True,
                                 {"dt": 3600.0, "f": 0.125}, None)],
    "cloudsc2_ad": [(_names("in_{}", NL_IN) + _names("in_{}_i", NL_OUT) + _names("out_{}", NL_OUT)
                     + _names("out_{}_i", NL_IN), True, {"dt": 3600.0}, None)],
    "cloudsc2_ad_from_trajectory": [(_names("in_{}", NL_IN) + _names("in_{}_i", NL_OUT) + ["traj_fplsl", "traj_fplsn"]
                                     + _names("out_{}_i", NL_IN), True, {"dt": 3600.0}, None)],
    "saturation": [(["in_ap", "in_t", "out_qsat"], False, {}, None)],
    "state_increment": [(_names("in_{}", INC) + _names("out_{}_i", INC), False, {"f": 0.125}, None)],
    "perturbed_state": [(_names("in_{}", INC) + _names("in_{}_i", INC) + _names("out_{}", INC), False, {"f": 0.125}, None)],
}

_COMMON = ["--num-cols", "64", "--input", "synthetic", "--num-runs", "1"]
DRIVER_RUNS = (
    ("run_taylor_test", []), ("run_taylor_test", ["--fused"]), ("run_taylor_test", ["--fused-norms"]),
    ("run_taylor_test", ["--fused-stored"]), ("run_taylor_test", ["--fused-all"]),
    ("run_taylor_test", ["--precision", "single"]),
    ("run_symmetry_test", []), ("run_symmetry_test", ["--fused"]), ("run_symmetry_test", ["--fused", "--ad-traj-fix"]),
    ("run_symmetry_test", ["--precision", "single"]),
    ("run_nonlinear", []), ("run_nonlinear", ["--fused"]), ("run_nonlinear", ["--precision", "single"]),
)


# ------------------------------------------------------------------------------------------------ the recorder
class _Interned:
    """the big repeated values of a trace (params, field geometries, keyword lists) are stored once"""

    def __init__(self):
        self.table, self._index = [], {}

    def __call__(self, value):
        key = json.dumps(value, sort_keys=True)
        if key not in self._index:
            self._index[key] = len(self.table)
            self.table.append(value)
        return self._index[key]


def _normalised(stencil_calls, abi_calls, intern):
    out = []
    for c in stencil_calls:
        by_ptr = {}
        for k in sorted(c["fields"]):
            by_ptr.setdefault(c["fields"][k]["ptr"], k)

        def name(p):
            if isinstance(p, bool) or not isinstance(p, int):
                return p
            if p in by_ptr:
                return by_ptr[p]
            assert p < 1 << 20, f"{c['stencil']}: an address reached the ABI that no keyword of the call carries"
            return p

        abi = []
        for a in abi_calls[c["abi_first"]:c["abi_last"]]:
            args = []
            for i, x in enumerate(a["args"]):
                if isinstance(x, dict):
                    args.append({"params": intern(x["params"])})
                elif isinstance(x, list) and not any(isinstance(y, float) for y in x):
                    args.append({"ptrs": intern([None if y == 0 else name(y) for y in x])})
                elif i >= 4:
                    args.append(name(x))
                else:
                    args.append(x)                       # nx, nz, lev_stride
            abi.append({"entry": a["entry"], "args": args})
        rec = {k: c[k] for k in ("stencil", "scalars", "origin", "domain", "validate_args") if k in c}
        rec["externals"] = intern(c["externals"])
        rec["kwargs"] = intern(c["kwargs"])
        rec["fields"] = intern({k: [v["shape"], v["strides"], v["dtype"]] for k, v in c["fields"].items()})
        rec["abi"] = abi
        out.append(rec)
    return out


def record():
    """runs under the fakes: returns the trace"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import run_reference_on_recording_hip as fake
    import torch

    fake.install_fakes()
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import drivers, storage  # noqa: F401
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.stencils import STENCILS, compile_stencil, taylor_blocks

    intern = _Interned()

    def drain():
        got = _normalised(fake.STENCIL_CALLS, fake.ABI_CALLS, intern)
        del fake.STENCIL_CALLS[:], fake.ABI_CALLS[:]
        return got

    nx, nz = 96, 12
    assert sorted(DIRECT_CALLS) == sorted(STENCILS)
    direct = {}
    for stencil in sorted(STENCILS):
        for dtype in (torch.float64, torch.float32):
            st = compile_stencil(stencil, dict(default_externals(), NLEV=nz))
            for fields, eta, scalars, extra in DIRECT_CALLS[stencil]:
                kw = {n: storage.zeros(nx, nz, dtype, "cpu") for n in fields}
                if eta:
                    kw["in_eta"] = torch.zeros(nz + 1, dtype=dtype)
                kw.update(scalars)
                if extra == "partials":
                    kw["out_partials"] = torch.zeros((taylor_blocks(nx), len(NL_OUT)), dtype=torch.float64)
                elif extra == "partials_fs":
                    kw["fs"] = [0.1, 0.01]
                    kw["out_partials"] = torch.zeros((taylor_blocks(nx), 2, len(NL_OUT)), dtype=torch.float64)
                st(**kw, origin=(0, 0, 0), domain=(nx, 1, nz + st.nlev_offset), validate_args=False, exec_info=None)
            direct[f"{stencil}/{str(dtype).split('.')[1]}"] = drain()
    runs = {}
    for driver, flags in DRIVER_RUNS:
        module = __import__("gt4py_dwarf_p_cloudsc2_tl_ad_amd.drivers." + driver, fromlist=["main"])
        with contextlib.redirect_stdout(io.StringIO()):
            module.main(_COMMON + flags)
        runs[" ".join([driver] + flags)] = drain()
    return {"interned": intern.table, "direct": direct, "drivers": runs}


def _record_in_subprocess(path):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--record", str(path)], capture_output=True, text=True,
                       timeout=1800, cwd=ROOT, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]


def _dump(trace, path):
    with open(path, "w") as fh:
        json.dump(trace, fh, sort_keys=True, indent=0, separators=(",", ":"))
        fh.write("\n")


# ------------------------------------------------------------------------------------------------ the test
def test_call_path_reaches_the_abi_as_recorded(tmp_path):
    _record_in_subprocess(tmp_path / "trace.json")
    got = json.loads((tmp_path / "trace.json").read_text())
    want = json.loads(open(FIXTURE).read())
    assert sorted(got) == sorted(want) == ["direct", "drivers", "interned"]
    assert sorted(got["direct"]) == sorted(want["direct"]) and len(got["direct"]) == 24
    assert sorted(got["drivers"]) == sorted(want["drivers"]) == sorted(" ".join([d] + f) for d, f in DRIVER_RUNS)
    for part in ("direct", "drivers"):
        for key in want[part]:
            g, w = got[part][key], want[part][key]
            assert [c["stencil"] for c in g] == [c["stencil"] for c in w], key
            for i, (cg, cw) in enumerate(zip(g, w)):
                assert cg == cw, f"{key}: stencil call {i} ({cw['stencil']}) differs"
    assert got == want                                     # the whole trace, interned tables included


def test_recorded_sequences_are_the_documented_ones():
    """what the fixture itself holds: one ABI call per stencil call, and the drivers' sequences"""
    want = json.loads(open(FIXTURE).read())
    for part in ("direct", "drivers"):
        for key, calls in want[part].items():
            assert calls and all(len(c["abi"]) == 1 for c in calls), key
    seq = {k: [c["stencil"] for c in v] for k, v in want["drivers"].items()}
    head = ["saturation", "cloudsc2_nl", "state_increment", "cloudsc2_tl"]
    assert seq["run_taylor_test"] == 2 * (head + 10 * ["perturbed_state", "cloudsc2_nl"])
    assert seq["run_taylor_test --fused"] == seq["run_taylor_test --fused-norms"] == 2 * (head + 10 * ["cloudsc2_nl_taylor"])
    assert seq["run_taylor_test --fused-stored"] == 2 * (head + 10 * ["cloudsc2_nl_perturbed"])
    assert seq["run_taylor_test --fused-all"] == 2 * ["saturation", "cloudsc2_nl", "cloudsc2_tl_incremented",
                                                      "cloudsc2_nl_taylor_multi"]
    assert [len(seq["run_symmetry_test" + f]) for f in ("", " --fused", " --fused --ad-traj-fix")] == [8, 7, 7]
    assert seq["run_symmetry_test --fused"][-1] == "cloudsc2_ad"
    assert seq["run_symmetry_test --fused --ad-traj-fix"][-1] == "cloudsc2_ad_from_trajectory"
    assert len(seq["run_nonlinear"]) == 4 and len(seq["run_nonlinear --fused"]) == 3


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        _dump(record(), sys.argv[2])
    elif sys.argv[1:] == ["--regenerate"]:
        _record_in_subprocess(FIXTURE)
        print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
    else:
        raise SystemExit("usage: python tests/test_abi_trace.py --regenerate")
