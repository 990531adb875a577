"""What the eight thin calls of `autodiff` promise beside their numbers (`tl_masked`, `tl_step`, `tl_multi`, `tl_step_multi`,
`ad_masked`, `ad_step`, `ad_multi`, `ad_step_multi`), and what no other test states:

  * the errors they raise BEFORE any launch - exception type and the distinctive part of the message, behind the call's own
    prefix - with every C entry replaced by one that fails the test if it is reached;
  * the chunk plan of the multi calls: which entry is launched with how many directions, in which order (a chunk of one
    direction is the SINGLE-direction entry), and that `write_nl` hands the NL outputs to the first launch only.  The
    launches are real: every direction is compared with the single call on that direction alone, `assert_close` at its
    default."""
import re

import numpy as np
import pytest

from derivative_support import STATE4, STEP_IN, TND4, direction_case
from helpers import NL_IN, NL_OUT, assert_close, externals, from_device

pytestmark = pytest.mark.gpu

#: public name -> (kind, takes a batch of directions, the prefix of its messages, the names of its state)
CALLS = {"tl_masked": ("tl", False, "tl_masked", NL_IN), "tl_step": ("tl", False, "tl_step", STEP_IN),
         "tl_multi": ("tl", True, "tl_multi", NL_IN), "tl_step_multi": ("tl", True, "tl_multi_step", STEP_IN),
         "ad_masked": ("ad", False, "ad_masked", NL_IN), "ad_step": ("ad", False, "ad_step", STEP_IN),
         "ad_multi": ("ad", True, "ad_multi", NL_IN), "ad_step_multi": ("ad", True, "ad_multi_step", STEP_IN)}
ENTRIES = tuple(f"cloudsc2_{e}_{sfx}" for e in ("tl_masked", "tl_step", "tl_multi", "tl_multi_step", "ad_masked", "ad_step",
                                                  "ad_multi", "ad_multi_step") for sfx in ("f64", "f32"))
NX, NZ = 4, 3
#: case -> (the calls it applies to: "all", "multi", "single" or "ad", exception, distinctive part of the message with
#: {noun} = perturbation / forcing, {width} = the width given and {most} = the kind's `_lib.*_MAX_DIRS`; None: the message is
#: Python's own)
ERRORS = {
    "want empty": ("all", ValueError, "`want` must name at least one of"),
    "want unknown": ("all", ValueError, "`want` must name at least one of"),
    "field unknown": ("all", ValueError, "unknown field names ['nope']"),
    "on the cpu": ("all", ValueError, "lives on cpu; fields must live on the GPU (there is no host path)"),
    "eta short": ("all", ValueError, "eta must be a contiguous 1-D"),
    "none given": ("multi", ValueError, "no {noun} given"),
    "mixed shapes": ("multi", ValueError, "every {noun} must be a tensor of one shape (ndir, 4, 1, 4), got"),
    "ndir 0": ("multi", ValueError, "every {noun} must be a tensor of one shape (ndir, 4, 1, 4), got"),
    "width 0": ("multi", ValueError, "width={width} outside [1, {most}]"),
    "width MAX_DIRS+1": ("multi", ValueError, "width={width} outside [1, {most}]"),
    "other dtype": ("single", ValueError, "(nx, nlev, lev_stride) / dtype / device"),
    "traj empty": ("ad", ValueError, "missing fields ['fplsl', 'fplsn']"),
    "traj omitted": ("ad", TypeError, None),
}


def _applies(case, name):
    kind, multi, _, _ = CALLS[name]
    return {"all": True, "multi": multi, "single": not multi, "ad": kind == "ad"}[ERRORS[case][0]]


@pytest.fixture
def no_launch(hip_lib, monkeypatch):
    def reached(*args):
        raise AssertionError("a C entry was launched")

    for e in ENTRIES:
        monkeypatch.setattr(hip_lib, e, reached)


@pytest.mark.parametrize("case,name", [(c, n) for c in ERRORS for n in CALLS if _applies(c, n)])
def test_errors_are_raised_before_any_launch(gpu, no_launch, case, name):
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib, autodiff, storage

    kind, multi, what, names = CALLS[name]
    most = _lib.AD_MAX_DIRS if kind == "ad" else _lib.TL_MAX_DIRS
    _, exc, text = ERRORS[case]
    new = lambda dtype=np.float64: storage.zeros(NX, NZ, dtype, gpu)  # noqa: E731
    batch = lambda ndir, device=gpu: torch.zeros((ndir, NX, 1, NZ + 1), dtype=torch.float64, device=device)  # noqa: E731
    one = (lambda: batch(2)) if multi else new
    have, want = ("tnd_t", ("t",)) if kind == "ad" else ("t", ("tnd_t",))
    dirs = {have: one()}
    eta = torch.zeros(NZ + 1, dtype=torch.float64, device=gpu)
    kw = {}
    if kind == "ad":
        kw["traj"] = {"fplsl": new(), "fplsn": new()}
    if case == "want empty":
        want = ()
    elif case == "want unknown":
        want = ("nope",)
    elif case == "field unknown":
        dirs = {"nope": one()}
    elif case == "on the cpu":
        dirs = {have: batch(2, "cpu") if multi else torch.zeros((NX, 1, NZ + 1), dtype=torch.float64)}
    elif case == "eta short":
        eta = eta[:NZ]
    elif case == "none given":
        dirs = {}
    elif case == "mixed shapes":
        dirs = {have: batch(2), ("tnd_q" if kind == "ad" else "q"): batch(3)}
    elif case == "ndir 0":
        dirs = {have: batch(0)}
    elif case.startswith("width"):
        kw["width"] = 0 if case == "width 0" else most + 1
    elif case == "other dtype":
        dirs = {have: new(np.float32)}
    elif case == "traj empty":
        kw["traj"] = {}
    elif case == "traj omitted":
        del kw["traj"]
    if kind == "tl":
        kw["write_nl"] = True
    noun = "forcing" if kind == "ad" else "perturbation"
    match = "traj"
    if text is not None:
        match = "^" + re.escape(what + ": ") + ".*" + re.escape(text.format(noun=noun, width=kw.get("width"), most=most))
    with pytest.raises(exc, match=match):
        getattr(autodiff, name)({n: new() for n in names}, dirs, eta, 3600.0, externals(NLEV=NZ), want=want, **kw)


# ---- the chunk plan ---------------------------------------------------------------------------------------------------------
NDIR = 11
#: (ndir, width) -> the launches: the number of directions of each, 1 = the single-direction entry
PLANS = {(11, 5): (5, 5, 1), (3, 1): (1, 1, 1), (8, 8): (8,)}


@pytest.fixture(scope="module")
def cases():
    """what `_case` has computed, kept for this module's tests only"""
    kept = {}
    yield kept
    kept.clear()


def _case(cases, gpu, kind, dtype):
    """63 columns x 137 levels (138 stored; one partial workgroup), 11 independent directions on the 4D-Var mask, and what
    the single call gives for each direction alone: computed once per kind and precision, never modified.
    TL: the masked family, perturbations = the directions of `derivative_support.direction_case`;
    AD: the step family, forcing = the perturbed outputs of `tl_step` on those (tests/test_hip_ad_multi.py)."""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff, storage

    key = (kind, np.dtype(dtype))
    if key in cases:
        return cases[key]
    nx, nz = 63, 137
    fields, eta, dt, others = direction_case(nx, nz, dtype, NDIR)
    names = NL_IN if kind == "tl" else STEP_IN
    state = {n: storage.from_klayout(fields["in_" + n], dtype, gpu) for n in names}
    eta = torch.as_tensor(eta, device=gpu)
    ext = externals(NLEV=nz)
    pert = {n: storage.zeros_batched(NDIR, nx, nz, dtype, gpu) for n in STATE4}
    for d, other in enumerate(others):
        for n in STATE4:
            storage.klayout(pert[n][d]).copy_(torch.as_tensor(other[n]))
    single_tl = autodiff.tl_masked if kind == "tl" else autodiff.tl_step
    nl, rows = None, []
    for d in range(NDIR):
        o, out_i = single_tl(state, {n: f[d] for n, f in pert.items()}, eta, dt, ext, want=TND4, write_nl=d == 0)
        nl = o if d == 0 else nl
        rows.append(out_i)
    if kind == "tl":
        cases[key] = dict(state=state, eta=eta, dt=dt, ext=ext, dirs=pert, want=TND4, kw={},
                           rows=[{n: from_device(r[n]) for n in TND4} for r in rows], nl=from_device(nl["tnd_t"]))
        return cases[key]
    forcing = {n: storage.zeros_batched(NDIR, nx, nz, dtype, gpu) for n in TND4}
    for d in range(NDIR):
        for n in TND4:
            forcing[n][d].copy_(rows[d][n])
    traj = {"fplsl": nl["fplsl"], "fplsn": nl["fplsn"]}
    adj = [autodiff.ad_step(state, {n: f[d] for n, f in forcing.items()}, eta, dt, ext, traj=traj, want=STATE4)
           for d in range(NDIR)]
    cases[key] = dict(state=state, eta=eta, dt=dt, ext=ext, dirs=forcing, want=STATE4, kw=dict(traj=traj),
                       rows=[{n: from_device(r[n]) for n in STATE4} for r in adj])
    return cases[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["tl", "ad"])
def test_chunk_plan(gpu, hip_lib, monkeypatch, cases, kind, dtype):
    """`tl_multi` (masked family) and `ad_step_multi` (step family): the (entry, ndir) sequence of every plan of `PLANS`;
    TL with `write_nl`: exactly the first launch is given the NL outputs"""
    import torch

    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import autodiff

    c = _case(cases, gpu, kind, dtype)
    nz = 137
    sfx = "f64" if np.dtype(dtype) == np.float64 else "f32"
    family = ("masked", "multi") if kind == "tl" else ("step", "multi_step")
    single, multi = (f"cloudsc2_{kind}_{f}_{sfx}" for f in family)
    log = []

    def recording(entry, real):
        def shim(*args):
            # behind (params, nx, nz, lev_stride): TL 8 arguments with `out` the fifth, AD 9; then ndir and the two strides
            tail = args[4 + (8 if kind == "tl" else 9):]
            log.append((entry, tail[0] if tail else 1, kind == "tl" and args[8] is not None))
            return real(*args)
        return shim

    for k in ("tl", "ad"):                          # the eight entries of the family, both kinds and both precisions
        for f in family:
            for s in ("f64", "f32"):
                entry = f"cloudsc2_{k}_{f}_{s}"
                monkeypatch.setattr(hip_lib, entry, recording(entry, getattr(hip_lib, entry)))
    call = autodiff.tl_multi if kind == "tl" else autodiff.ad_step_multi
    for (ndir, width), plan in PLANS.items():
        del log[:]
        dirs = {n: f[:ndir] for n, f in c["dirs"].items()}
        kw = dict(c["kw"], write_nl=True) if kind == "tl" else c["kw"]
        got = call(c["state"], dirs, c["eta"], c["dt"], c["ext"], want=c["want"], width=width, **kw)
        torch.cuda.synchronize()
        assert [(e, n) for e, n, _ in log] == [(single if n == 1 else multi, n) for n in plan], (ndir, width)
        if kind == "tl":
            assert [o for _, _, o in log] == [True] + [False] * (len(plan) - 1), (ndir, width)
            nl, got = got
            assert sorted(nl) == sorted(NL_OUT)
            assert_close(f"{multi} {ndir}/{width} NL out_tnd_t", from_device(nl["tnd_t"])[:nz], c["nl"][:nz], dtype)
        assert sorted(got) == sorted(c["want"])
        for n in c["want"]:
            assert tuple(got[n].shape) == (ndir, 63, 1, nz + 1)
            for d in range(ndir):
                a = from_device(got[n][d])
                assert_close(f"{multi} {ndir}/{width} {n}[{d}]", a[:nz], c["rows"][d][n][:nz], dtype)
                assert not a[nz:].any()
