"""What the masked TL / AD family of the C ABI refuses, pinned as a table (CPU only: every call here is refused before a
launch, or is an empty call, so nothing is launched).

All eighteen derivative entries, in both precisions, are called through ctypes with the dummy caller's arguments
(tests/abi_calls.py: pointer 4096, NZ, LS, FIELD) and

  1. one defect at a time: every check `tl_masked_impl` / `ad_masked_impl` (csrc/cloudsc2_capi.hip) makes that applies to
     the entry, in source order (`checks` below);
  2. two defects at once, one from each of two neighbouring checks, so that the ORDER of the checks is pinned: the earlier
     one must answer.  A pair that cannot be formed (both defects need the same argument) is left out, except where only
     `lev_stride` / `member_stride` are shared: there the earlier check's value stands and both defects remain;
  3. one empty call (`nx = 0`).

Recorded per call: the return code and the `cloudsc2_last_error()` text (it holds no addresses), the entry's own name
replaced by `{fn}`; for the empty call the return code alone (the message buffer still holds the previous call's text).
The table must equal tests/golden/masked_refusals.json as a whole.  The fixture is written by `python
tests/test_masked_refusals.py --regenerate` (CLOUDSC2_HIP_LIB selects the library file); it was generated from the library
as it was before the call descriptor of the masked family was introduced and is not to be regenerated for a change that
claims to leave the refusals as they are."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from abi_calls import FIELD, LS, NZ, QSAT, Call, max_dirs  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "masked_refusals.json")
P = Call.P
FAR = 1 << 40            # `cover` of the dummy caller: far from every other field (they all sit at P)
BIG_LS = 1 << 25         # (NZ + 1) * BIG_LS * 4 bytes = 17.25 GiB: a field of 4 GiB or more in both precisions
BIG_FIELD = (NZ + 1) * BIG_LS
GRID_NX = 257            # two column blocks per member: INT32_MAX members of them exceed the grid limit

ENTRIES = ("tl_masked", "tl_step", "tl_multi", "tl_multi_step", "tl_ens", "tl_step_ens",
           "ad_masked", "ad_step", "ad_multi", "ad_multi_step", "ad_ens", "ad_step_ens",
           "ad_evap", "ad_evap_step", "ad_evap_multi", "ad_evap_multi_step", "ad_evap_ens", "ad_evap_step_ens")


def form(entry):
    """(tl, step, multi, ens, evap) of an entry, from its name"""
    return entry.startswith("tl"), "step" in entry, "multi" in entry, entry.endswith("ens"), "evap" in entry


def base(entry):
    """the dummy caller's arguments: a call that would pass every check.  `p`: the externals beside the defaults (None:
    NULL params); pointer arrays are lists (None: the array itself is NULL)"""
    tl, step, multi, ens, evap = form(entry)
    a = dict(p={"NLEV": NZ}, nx=64, nz=NZ, ls=LS, in_=[P] * 16, zero=P, eta=P, dt=3600.0)
    if tl:
        a.update(in_i=[P] * 16, out=[P] * 10, out_i=[P] * 10)
    else:
        a.update(in_adj=[P] * 10, traj_l=P, traj_n=P, out_adj=[P] * 16)
    if step:
        a["in_i" if tl else "out_adj"][QSAT] = 0
    if multi:
        a.update(ndir=2, in_ds=FIELD, out_ds=FIELD)
    if ens:
        a.update(nmem=2, ms=FIELD)
    if evap:
        a.update(cover=FAR, ready=0)
        a["p"]["LEVAPLS2"] = True
    return a


def checks(entry):
    """[(check, [(label, edits), ...]), ...] in the source order of the impl function; an edit's target is an argument, or
    (argument, slot) for one slot of a pointer array or one external"""
    tl, step, multi, ens, evap = form(entry)
    big = {"ls": BIG_LS}
    if multi:
        big.update(in_ds=BIG_FIELD, out_ds=BIG_FIELD)
    if ens:
        big.update(ms=BIG_FIELD)
    four_gib = ("field size", [("a field of 4 GiB", big)])
    out = [("params", [("params NULL", {"p": None})]),
           ("nx", [("nx=-1", {"nx": -1})]),
           ("nz", [("nz=1", {"nz": 1}), ("nz=4096", {"nz": 4096})]),
           ("lev_stride", [("lev_stride=63", {"ls": 63})])]
    if multi:
        out += [("ndir", [("ndir=0", {"ndir": 0}), ("ndir=max+1", {"ndir": max_dirs("tl" if tl else "ad") + 1})]),
                ("direction strides", [("in_dir_stride short", {"in_ds": FIELD - 1}),
                                       ("out_dir_stride short", {"out_ds": FIELD - 1})])]
    if ens:
        out += [("nmem", [("nmem=0", {"nmem": 0})]),
                ("member_stride", [("member_stride short", {"ms": FIELD - 1})]),
                four_gib,
                ("grid limit", [("grid limit", {"nmem": 2 ** 31 - 1, "nx": GRID_NX, "ls": 320, "ms": (NZ + 1) * 320})])]
    out += [("in", [("in NULL", {"in_": None}), ("in[3] NULL", {("in_", 3): 0})])]
    arr = "in_i" if tl else "in_adj"
    masked_in = (arr, [(arr + " NULL", {arr: None}), (arr + "[3] NULL, no zero line", {(arr, 3): 0, "zero": None}),
                       ("zero line misaligned", {"zero": P + 8})])
    if tl:
        if step:
            out += [("in_i qsat", [("in_i[qsat] given", {("in_i", QSAT): P})])]
        out += [masked_in,
                ("out", [("out[3] NULL", {("out", 3): 0})]),
                ("out_i", [("out_i NULL", {"out_i": None}), ("out_i all NULL", {"out_i": [0] * 10})]),
                ("eta", [("eta NULL", {"eta": None})])]
    else:
        out += [masked_in]
        if step:
            out += [("out_adj qsat", [("out_adj[qsat] given", {("out_adj", QSAT): P})])]
        out += [("out_adj", [("out_adj NULL", {"out_adj": None}), ("out_adj all NULL", {"out_adj": [0] * 16})]),
                ("eta / traj", [("eta NULL", {"eta": None}), ("traj_fplsl NULL", {"traj_l": None}),
                                ("traj_fplsn NULL", {"traj_n": None})])]
        if evap:
            out += [("cover", [("cover NULL", {"cover": None})])]
    out += [("ICALL", [("ICALL=1", {("p", "ICALL"): 1})])]
    if evap:
        out += [("switches", [("no evaporation switch", {("p", "LEVAPLS2"): False})])]
    elif not tl:
        out += [("switches", [("LEVAPLS2 set", {("p", "LEVAPLS2"): True}), ("LDRAIN1D set", {("p", "LDRAIN1D"): True})])]
    out += [("dt", [("dt=0", {"dt": 0.0}), ("dt=-1", {"dt": -1.0})]),
            ("NLEV", [("NLEV != nz", {("p", "NLEV"): NZ + 1})])]
    if step:
        out += [("LPHYLIN", [("not LPHYLIN", {("p", "LPHYLIN"): False})])]
    if not ens:
        out += [four_gib]
    if evap and ens:
        out += [("cover overlap", [("cover over in[0]", {"cover": P}), ("cover over in[7]", {("in_", 7): FAR}),
                                   ("cover over out_adj[5]", {("out_adj", 5): FAR}),
                                   ("cover over in_adj[2]", {("in_adj", 2): FAR}), ("cover over traj_fplsl", {"traj_l": FAR}),
                                   ("cover over traj_fplsn", {"traj_n": FAR}), ("cover over zero_line", {"zero": FAR}),
                                   ("cover over eta", {"eta": FAR})])]
    return out


GEOMETRY = ("ls", "ms")  # what a 4 GiB field changes beside: in a pair the earlier check's value stands, both defects remain


def _compatible(e1, e2):
    root = lambda t: t[0] if isinstance(t, tuple) else t  # noqa: E731
    return not any(root(t1) == root(t2) and (t1 == t2 or not (isinstance(t1, tuple) and isinstance(t2, tuple)))
                   for t1 in e1 for t2 in e2 if t1 not in GEOMETRY)


def calls(entry):
    """[(label, edits), ...]: the single defects, the neighbouring pairs, the empty call"""
    table = checks(entry)
    out = [d for _, defects in table for d in defects]
    for (_, first), (_, second) in zip(table, table[1:]):
        pair = next(((l1 + " + " + l2, {**e2, **e1}) for l1, e1 in first for l2, e2 in second if _compatible(e1, e2)), None)
        if pair:
            out.append(pair)
    assert len({label for label, _ in out}) == len(out), entry
    return out + [("empty call", {"nx": 0})]


_PARAMS = {}


def _params(externals):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd.params import default_externals, make_params

    key = json.dumps(externals, sort_keys=True)
    if key not in _PARAMS:
        _PARAMS[key] = make_params(dict(default_externals(), **externals))
    return _PARAMS[key]


def invoke(lib, entry, sfx, edits):
    """the C call of `entry` with the dummy caller's arguments under `edits`: argument order of include/cloudsc2_hip.h"""
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd._lib import ptr_array

    tl, step, multi, ens, evap = form(entry)
    a = base(entry)
    for target, value in edits.items():
        if isinstance(target, tuple):
            a[target[0]][target[1]] = value
        else:
            a[target] = value
    arr = lambda v: None if v is None else ptr_array(v)  # noqa: E731
    args = [None if a["p"] is None else ctypes.byref(_params(a["p"])), a["nx"], a["nz"], a["ls"], arr(a["in_"])]
    if tl:
        args += [arr(a["in_i"]), a["zero"], a["eta"], arr(a["out"]), arr(a["out_i"]), a["dt"]]
    else:
        args += [arr(a["in_adj"]), a["zero"], a["eta"], a["traj_l"], a["traj_n"], arr(a["out_adj"]), a["dt"]]
    dirs = [a["ndir"], a["in_ds"], a["out_ds"]] if multi else []
    members = [a["nmem"], a["ms"]] if ens else []
    cover = [a["cover"], a["ready"]] if evap else []
    # `cover` stands in front of `stream` in the single evaporation entries, behind the directions in the multi ones
    args += cover + [None] + members if evap and not multi else [None] + dirs + members + cover
    return getattr(lib, f"cloudsc2_{entry}_{sfx}")(*args)


def record(lib, sfx):
    """{entry: {label: [return code, message]}}; the message of the empty call is None"""
    out = {}
    for entry in ENTRIES:
        fn, rows = f"cloudsc2_{entry}_{sfx}", {}
        for label, edits in calls(entry):
            rc = invoke(lib, entry, sfx, edits)
            if label == "empty call":
                rows[label] = [rc, None]
            else:
                # -1 / -2: refused by a check.  Anything else would have reached a launcher, on the dummy pointers.
                assert rc in (-1, -2), (fn, label, rc, lib.cloudsc2_last_error())
                rows[label] = [rc, lib.cloudsc2_last_error().decode().replace(fn, "{fn}")]
        out[entry] = rows
    return out


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_refusals_are_the_recorded_ones(hip_lib, sfx):
    got = record(hip_lib, sfx)
    want = json.loads(open(FIXTURE).read())
    rows = {entry: {label: want["outcomes"][i] for label, i in calls_.items()} for entry, calls_ in want[sfx].items()}
    assert sorted(rows) == sorted(ENTRIES)
    for entry in ENTRIES:
        assert list(got[entry]) == list(rows[entry]), entry                 # the same calls, in the same order
        for label in got[entry]:
            assert got[entry][label] == rows[entry][label], f"cloudsc2_{entry}_{sfx}: {label}"
    assert got == rows


def test_the_fixture_holds_every_check_of_every_entry():
    """what the fixture itself holds: the calls of `calls`, refusals only, no addresses"""
    want = json.loads(open(FIXTURE).read())
    assert sorted(want) == ["f32", "f64", "outcomes"]
    for sfx in ("f64", "f32"):
        for entry in ENTRIES:
            rows = want[sfx][entry]
            assert list(rows) == [label for label, _ in calls(entry)], (entry, sfx)
            for label, i in rows.items():
                rc, msg = want["outcomes"][i]
                if label == "empty call":
                    assert (rc, msg) == (0, None)
                else:
                    assert rc in (-1, -2) and msg.startswith("{fn}: ") and "0x" not in msg, (entry, sfx, label)


def _regenerate():
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    lib, outcomes, fixture = _lib.load(), [], {}
    for sfx in ("f64", "f32"):
        fixture[sfx] = {}
        for entry, rows in record(lib, sfx).items():
            fixture[sfx][entry] = {}
            for label, outcome in rows.items():
                if outcome not in outcomes:
                    outcomes.append(outcome)
                fixture[sfx][entry][label] = outcomes.index(outcome)
    fixture["outcomes"] = outcomes
    with open(FIXTURE, "w") as fh:
        json.dump(fixture, fh, indent=0, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes, {len(outcomes)} distinct outcomes) from {_lib.LIB_PATH}")


if __name__ == "__main__":
    if sys.argv[1:] == ["--regenerate"]:
        sys.path.insert(0, ROOT)
        _regenerate()
    else:
        raise SystemExit("usage: python tests/test_masked_refusals.py --regenerate")
