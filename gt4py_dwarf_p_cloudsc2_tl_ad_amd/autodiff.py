"""CLOUDSC2 as a differentiable PyTorch operation (C ABI `cloudsc2_tl_masked_*`, `cloudsc2_ad_masked_*`, and for the
whole step `cloudsc2_saturation_tl_*` / `_ad_*`, `cloudsc2_tl_step_*` / `cloudsc2_ad_step_*`).

`cloudsc2(state, eta, dt)` is one `cloudsc2_nl` step whose gradients PyTorch can take: reverse mode (`backward`,
`torch.autograd.grad`) runs the adjoint kernel, forward mode (`torch.autograd.forward_ad`) the tangent-linear kernel.  A
derivative rule has perturbations / forcing on a few fields only and wants a few results only, so both go through the
MASKED kernels: fields a call does not have are NULL entries that move no HBM words (include/cloudsc2_hip.h).

`cloudsc2` differentiates `cloudsc2_nl` alone: `qsat` is one of its 16 independent inputs.  The step the drivers run is
`saturation` + `cloudsc2_nl`, where `qsat` is a function of `ap` and `t`: `cloudsc2_step(state, eta, dt)` is that step with
the TOTAL derivative (the path t, ap -> qsat -> cloudsc2 included), `saturation(ap, t)` its first half on its own.

`tl_masked` / `ad_masked`, `tl_step` / `ad_step` and `saturation_tl` / `saturation_ad` are the thin calls underneath, usable
on their own (a variational cost, a sensitivity study).  GPU tensors only - there is no host path.

MANY derivatives on one trajectory.  `tl_multi` / `tl_step_multi` push `ndir` perturbations through one linearisation (C ABI
`cloudsc2_tl_multi_*` / `cloudsc2_tl_multi_step_*`: one launch reads the state once for up to `width` directions; the default
width per precision, `MULTI_WIDTH`, is 1 - single launches; docs/TUNING_LOG.md 3.18 has the measurement).  `ad_multi` /
`ad_step_multi` pull `ndir` cotangents back through it (C ABI `cloudsc2_ad_multi_*` / `cloudsc2_ad_multi_step_*`: one
launch reads the state and recomputes each level's nonlinear trajectory once for up to `width` cotangents; the default
width per precision is `AD_MULTI_WIDTH`, set from the measurement of docs/TUNING_LOG.md 3.19).
`cloudsc2`, `cloudsc2_step` and `saturation` work under `torch.func`: `jvp`, `vjp`, `grad`, `jacfwd`, `jacrev`, and `vmap`
over TANGENTS or COTANGENTS (`vmap` of `jvp`, which is what `jacfwd` is; `vmap` of a `vjp` function, which is what `jacrev`
is).  Batched tangents run `tl_multi` / `tl_step_multi`; batched cotangents run `ad_multi` / `ad_step_multi` (the
non-LPHYLIN step, which has no multi-direction kernel, loops over its single-cotangent fallback, and so does `saturation`,
which is pointwise).

THE EVAPORATION SWITCHES (LEVAPLS2 / LDRAIN1D) in the adjoint.  `ad_masked_evap` / `ad_step_evap` / `ad_multi_evap` /
`ad_step_multi_evap` are `ad_masked` / `ad_step` / `ad_multi` / `ad_step_multi` for them (C ABI `cloudsc2_ad_evap_*`): one launch
that first parks the precipitation cover entering each level in a `cover` field and then runs the masked sweep with the
evaporation block; `cover_ready=True` reuses a filled field.  The derivative rules use them only when the module-level
`EVAP_ADJOINT` is `"trajectory"`; with its default `"dense"` a backward with the switches is the dense `cloudsc2_ad`, and
batched cotangents loop over it, as before (docs/TUNING_LOG.md 3.22).

ENSEMBLES: many states, one launch.  `cloudsc2_ensemble` / `cloudsc2_step_ensemble` are the two Functions on member-major
`(nmem, nx, 1, nz+1)` fields - the layout of `storage.zeros_batched`, of `torch.stack` and of every `*_multi` result; `eta`,
`dt` and the externals are shared - and `tl_masked_ens` / `tl_step_ens` / `ad_masked_ens` / `ad_step_ens` the thin calls (C ABI
`cloudsc2_{nl,nl_fused,tl,tl_step,ad,ad_step}_ens_*`: one workgroup serves one column block of one member; a tensor in
another layout is copied once).  `vmap` over the STATE of `cloudsc2` / `cloudsc2_step` runs them - `vmap(f)`,
`vmap(grad(cost))`, `grad` through `vmap`, `vmap` of `jvp` over states and tangents - for a WHOLE state: every field batched (a state batched in part is refused as
before: `expand` the fields the members share), unbatched tangents / cotangents expanded.  What
has no ensemble kernel loops over the members through the single paths: the non-LPHYLIN step, `saturation` with its
derivatives (pointwise), and BY DEFAULT the evaporation switches in the adjoint, in either `EVAP_ADJOINT` mode.
docs/TUNING_LOG.md 3.21 has the measurement.

ENSEMBLES WITH THE EVAPORATION SWITCHES.  `ad_masked_evap_ens` / `ad_step_evap_ens` are `ad_masked_evap` / `ad_step_evap` for all
members in one launch (C ABI `cloudsc2_ad_evap_ens_*` / `cloudsc2_ad_evap_step_ens_*`; `cover` is member-major like every other
tensor).  The derivative rules - `backward` of `cloudsc2_ensemble` / `cloudsc2_step_ensemble`, `vmap(grad(cost))` and `grad`
through `vmap` over the state - use them only when the module-level `EVAP_ENSEMBLE` is true AND `EVAP_ADJOINT` is
`"trajectory"`.  `EVAP_ENSEMBLE` is False by default: the looped launches are what shipped, and tests pin their kernel
names under the existing settings; docs/TUNING_LOG.md 3.25 has the measurement of the one launch against the loop.

ENSEMBLE JACOBIANS: members TIMES directions.  `ad_multi_ens` / `ad_step_multi_ens` are `ad_multi` / `ad_step_multi` for all
members of an ensemble (C ABI `cloudsc2_ad_multi_ens_*` / `cloudsc2_ad_multi_step_ens_*`): states and trajectory fluxes
member-major `(nmem, nx, 1, nz+1)`, forcings and results `(nmem, ndir, nx, 1, nz+1)`, every chunk of `width` cotangents ONE
launch for all members.  Under `torch.func` they are opt-in: with the module-level `ENSEMBLE_JACOBIANS` False, the default,
nested `vmap` over states and directions raises the `NotImplementedError` it always has.  With it True, `vmap(jacrev(f))`
and `vmap(vmap(vjp_fn))` over stacked states run those launches (LPHYLIN, no evaporation switches; with the switches, in
either `EVAP_ADJOINT` mode, and for the non-LPHYLIN step the multi-direction path runs member by member), and
`vmap(jacfwd(f))` / `vmap(vmap(jvp))` one `tl_masked_ens` / `tl_step_ens` launch per direction.  The STATE must be the outer
batch level: `jacrev` / `jacfwd` applied OUTSIDE `cloudsc2_ensemble` (directions outer, members inner) stays refused, and so
do a state batched in part, two batch levels over the state or over the directions, and `saturation` on its own under
nesting.  docs/TUNING_LOG.md 3.26.

ENSEMBLES THAT SHARE PART OF THEIR STATE.  The members of an ensemble usually differ in a few fields (`t, q, ql, qi`) and share
the rest.  `tl_masked_ens`, `tl_step_ens`, `ad_masked_ens`, `ad_step_ens`, `cloudsc2_ensemble` and `cloudsc2_step_ensemble` take
`shared={name: plain (nx, 1, nz+1) field}` beside `states`, and an `eta` of shape `(nmem, nz+1)`: C ABI `cloudsc2_*_enss_*`,
the ensemble kernels with a per-field choice of the member base and a per-member level table.  No field is copied per
member.  `BLOCK_ORDER` chooses how workgroups are dealt to (member, column block) pairs (docs/TUNING_LOG.md 3.27).  The
evaporation ensembles, members times directions, the non-LPHYLIN step and `saturation` keep whole members: there shared
fields are expanded and copied, or the members looped, as before.  Under `torch.func.vmap` a state batched in part and a
batched `eta` are refused (`NotImplementedError`) unless the module-level `SHARED_STATE` is True: then `vmap` over `cloudsc2` /
`cloudsc2_step` with some state fields at `in_dims=None` runs these launches with those fields shared, and a batched `eta`
with one level vector per member (`vmap(f)`, `vmap(grad(cost))`, `grad` through `vmap`, `vmap(jvp)`), and an `expand`ed field
in `states` is recognised as shared.

Not supported: `torch.autograd.grad(..., is_grads_batched=True)` (the legacy vmap, which knows no `vmap` rule of a
Function), second derivatives."""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Iterable, Mapping, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import NL_IN, NL_OUT
from .params import default_externals, make_params
from .storage import direction_stride, field_geometry, level_pitch, zeros, zeros_batched

_SFX = {torch.float64: "f64", torch.float32: "f32"}
#: the inputs of the step: those of `cloudsc2_nl` without `qsat`, which the step forms from `ap` and `t`
STEP_IN = tuple(n for n in NL_IN if n != "qsat")
#: directions per launch of the multi-direction TL, per precision: the measured width with the best time per direction.
#: 1 = that precision loops over single `tl_masked` / `tl_step` launches.  The measurement (profiles/bench_tl_multi.py,
#: docs/TUNING_LOG.md 3.18) has been taken; no width has been enabled from it yet; `width=` of `tl_multi` reaches the kernel.
MULTI_WIDTH: Dict[torch.dtype, int] = {torch.float64: 1, torch.float32: 1}
#: cotangents per launch of the multi-direction AD, per precision, by the rule of docs/TUNING_LOG.md 3.19: the measured
#: width with the best median time per direction, if that beats the looped single launches by more than the looped case's
#: own min-max spread in the same run; otherwise 1 = that precision loops over single `ad_masked` / `ad_step` launches.
#: `width=` of `ad_multi` / `ad_step_multi` reaches the kernel in any case.  Measured on an MI355X (profiles/bench_ad_multi.py,
#: 4D-Var mask of the step family, microseconds per direction, looped singles -> one launch; looped min-max spread):
#:   fp64  65 536 columns   D=2 547 -> 458   D=4 538 -> 350   D=8 528 -> 301   (8 launches 4 221 us +- 76, one 2 406 us)
#:   fp32 524 288 columns   D=2 1 896 -> 1 889   D=4 1 865 -> 1 441   D=8 1 823 -> 2 086   (4 launches 7 458 us +- 273, one 5 765 us)
#: fp32 loses at 8: its 83 KB of LDS leave one workgroup per CU where 4 directions (59 KB) leave two.
AD_MULTI_WIDTH: Dict[torch.dtype, int] = {torch.float64: 8, torch.float32: 4}
#: how `backward` of `cloudsc2` / `cloudsc2_step` (and `jacrev` over them) runs with LEVAPLS2 / LDRAIN1D; read at backward time.
#:   "dense"       the dense `cloudsc2_ad` (plus `saturation_ad` for the step), one launch per cotangent: what shipped before
#:                 the trajectory kernels of the evaporation block existed, and still the default
#:   "trajectory"  `ad_masked_evap` / `ad_step_evap`, batched cotangents `ad_multi_evap` / `ad_step_multi_evap`
#: docs/TUNING_LOG.md 3.22 says when to set it.  Ensembles loop over their members either way, unless `EVAP_ENSEMBLE` is set.
EVAP_ADJOINT = "dense"
#: whether an ENSEMBLE's backward with LEVAPLS2 / LDRAIN1D is ONE launch for all members (`ad_masked_evap_ens` /
#: `ad_step_evap_ens`); read at backward time, and only under `EVAP_ADJOINT = "trajectory"` (the kernels are the trajectory
#: kernels' ensemble forms).  False, the default: the members are looped, one `ad_masked_evap` launch each, as before these
#: kernels existed.  docs/TUNING_LOG.md 3.25 has the measurement.
EVAP_ENSEMBLE = False
#: whether members TIMES directions is served (`vmap(jacrev(f))`, `vmap(vmap(vjp_fn))`, `vmap(jacfwd(f))` over stacked states)
#: instead of refused; read when the derivative rule runs.  False, the default: the `NotImplementedError` that shipped, which
#: tests pin.  True: cotangents run `ad_multi_ens` / `ad_step_multi_ens` - one launch per `AD_MULTI_WIDTH` cotangents for ALL
#: members - where the adjoint is one launch of the family (LPHYLIN, no evaporation switches), and the multi-direction path
#: member by member elsewhere; tangents run one `tl_masked_ens` / `tl_step_ens` launch per direction (`MULTI_WIDTH` is 1).
#: docs/TUNING_LOG.md 3.26 says for which shapes the one launch pays.
ENSEMBLE_JACOBIANS = False
#: how the shared-state ensemble launches (`shared=` / a per-member `eta`; C ABI `cloudsc2_*_enss_*`) deal workgroups to
#: (member, column block) pairs; read at launch time.  None: the library's default (member-major, docs/TUNING_LOG.md 3.27);
#: "member" / "column": member-major / column-block-major.  The results do not depend on it; it exists for the measurement.
BLOCK_ORDER: Optional[str] = None
#: whether `torch.func.vmap` over PART of the state of `cloudsc2` / `cloudsc2_step`, or over `eta`, is served instead of refused;
#: read when the `vmap` rule runs.  False, the default: the two `NotImplementedError`s that shipped, which tests pin, and a
#: stride-0 `expand`ed field in `states` is copied per member as before.  True: the fields at `in_dims=None` are passed as
#: SHARED to the shared-state launches (`cloudsc2_*_enss_*`), a batched `eta` as one level vector per member, and a field of
#: `states` that is an `expand` over the members (stride 0 over dimension 0) is recognised and passed as shared - for `vmap(f)`,
#: `vmap(grad(cost))`, `grad` through `vmap` and `vmap(jvp)`.  Nesting, the evaporation switches in the adjoint, the non-LPHYLIN
#: step and `saturation` stay refused or keep whole members as before.
SHARED_STATE = False


class _Family(NamedTuple):
    """one of the four kernel families behind the eight thin calls"""
    single: str                      # the C entry `cloudsc2_<single>_{f64,f32}`: one direction per launch
    multi: str                       # its multi-direction form (`_lib.MULTI_LAYOUTS`): the same arguments + (ndir, strides)
    names: Tuple[str, ...]           # the fields of the state
    width: Dict[torch.dtype, int]    # directions per launch by default, per precision
    max_dirs: int                    # the most one launch takes
    adjoint: bool = False            # forcing (`NL_OUT` names) and `traj` in, adjoints of `names` out; else the tangent-linear
    ens: str = ""                    # its ensemble form (`_lib.ENS_LAYOUTS`, `_lib.EVAP_ENS_LAYOUTS`): + (nmem, member_stride)
    mens: str = ""                   # members times directions (`_lib.MULTI_ENS_LAYOUTS`): the multi form + (nmem, 3 strides)


_TL_MASKED = _Family("tl_masked", "tl_multi", NL_IN, MULTI_WIDTH, _lib.TL_MAX_DIRS, ens="tl_ens")
_TL_STEP = _Family("tl_step", "tl_multi_step", STEP_IN, MULTI_WIDTH, _lib.TL_MAX_DIRS, ens="tl_step_ens")
_AD_MASKED = _Family("ad_masked", "ad_multi", NL_IN, AD_MULTI_WIDTH, _lib.AD_MAX_DIRS, adjoint=True, ens="ad_ens",
                     mens="ad_multi_ens")
_AD_STEP = _Family("ad_step", "ad_multi_step", STEP_IN, AD_MULTI_WIDTH, _lib.AD_MAX_DIRS, adjoint=True, ens="ad_step_ens",
                   mens="ad_multi_step_ens")
_AD_MASKED_EVAP = _Family("ad_evap", "ad_evap_multi", NL_IN, AD_MULTI_WIDTH, _lib.AD_MAX_DIRS, adjoint=True, ens="ad_evap_ens")
_AD_STEP_EVAP = _Family("ad_evap_step", "ad_evap_multi_step", STEP_IN, AD_MULTI_WIDTH, _lib.AD_MAX_DIRS, adjoint=True,
                        ens="ad_evap_step_ens")
_FAMILIES = {f.single: f for f in (_TL_MASKED, _TL_STEP, _AD_MASKED, _AD_STEP)}
_ZERO_LINE_BYTES = 512
_zero_lines: Dict[Tuple[torch.device, torch.dtype], torch.Tensor] = {}


def _zero_line(device: torch.device, dtype: torch.dtype) -> torch.Tensor:
    """the 512 zero bytes an absent input is read from: one per device and dtype, kept for the life of the process"""
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, dtype)
    line = _zero_lines.get(key)
    if line is None:
        line = _zero_lines[key] = torch.zeros(_ZERO_LINE_BYTES // torch.empty((), dtype=dtype).element_size(),
                                              dtype=dtype, device=device)
        # its memset ran on the stream current now; later calls read it from any stream: complete it once, here
        torch.cuda.current_stream(device).synchronize()
    return line


def _plain(t: torch.Tensor) -> torch.Tensor:
    return t.detach().as_subclass(torch.Tensor)


def _checked(what: str, groups: Iterable[Tuple[Mapping[str, torch.Tensor], Tuple[str, ...], bool]]):
    """geometry, dtype and device shared by every field of a call; `groups`: (fields, allowed names, all required)"""
    first, geo = None, None
    for fields, names, required in groups:
        unknown = sorted(set(fields) - set(names))
        if unknown:
            raise ValueError(f"{what}: unknown field names {unknown}")
        if required and set(fields) != set(names):
            raise ValueError(f"{what}: missing fields {sorted(set(names) - set(fields))}")
        for n, f in fields.items():
            if not isinstance(f, torch.Tensor):
                raise TypeError(f"{what}: {n} is not a torch.Tensor")
            if not f.is_cuda:
                raise ValueError(f"{what}: {n} lives on {f.device}; fields must live on the GPU (there is no host path)")
            g = field_geometry(f)
            if first is None:
                first, geo = f, g
            elif g != geo or f.dtype != first.dtype or f.device != first.device:
                raise ValueError(f"{what}: {n} has (nx, nlev, lev_stride) / dtype / device {g} / {f.dtype} / {f.device}, "
                                 f"the call's are {geo} / {first.dtype} / {first.device}")
    if first.dtype not in _SFX:
        raise TypeError(f"{what}: unsupported dtype {first.dtype}")
    return geo, first.dtype, first.device


def _eta(what: str, eta: torch.Tensor, nz: int, dtype, device) -> torch.Tensor:
    if (not isinstance(eta, torch.Tensor) or eta.dim() != 1 or eta.shape[0] < nz + 1 or eta.dtype != dtype
            or eta.device != device or not eta.is_contiguous()):
        raise ValueError(f"{what}: eta must be a contiguous 1-D {dtype} tensor on {device} with >= {nz + 1} entries")
    return eta


def _params(externals: Optional[Mapping[str, Any]], nz: int, **over):
    ext = dict(default_externals() if externals is None else externals)
    ext.update(over)
    p = make_params(ext)
    p.NLEV = nz
    return p


def _ptrs(fields: Mapping[str, torch.Tensor], names) -> ctypes.Array:
    return _lib.ptr_array([fields[n].data_ptr() if n in fields else 0 for n in names])


def _new_like(ref: torch.Tensor, nx: int, nz: int, ls: int) -> torch.Tensor:
    out = zeros(nx, nz, ref.dtype, ref.device)
    if nx > 0 and field_geometry(out)[2] != ls:      # the call's fields are windows of wider allocations: match their pitch
        out = torch.zeros((nz + 1, ls), dtype=ref.dtype, device=ref.device)[:, :nx].unsqueeze(1).permute(2, 1, 0)
    return out


def tl_masked(state: Mapping[str, torch.Tensor], perturbations: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
              externals: Optional[Mapping[str, Any]] = None, *, want: Iterable[str], write_nl: bool = False):
    """Tangent-linear CLOUDSC2 with absent fields: `perturbations` holds the perturbed inputs (`NL_IN` names; a missing
    name is a zero perturbation), `want` names the perturbed outputs (`NL_OUT` names) to produce.  Returns
    `(nl_outputs or None, {name: perturbed output})`; results are new `storage.zeros` fields."""
    return _call(_TL_MASKED, False, state, perturbations, eta, dt, externals, want, write_nl=write_nl)


def tl_step(state: Mapping[str, torch.Tensor], perturbations: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
            externals: Optional[Mapping[str, Any]] = None, *, want: Iterable[str], write_nl: bool = False):
    """Tangent-linear of the step `saturation` + `cloudsc2_nl` in ONE launch (`cloudsc2_tl_step_*`): `tl_masked` without the
    field `qsat` (`STEP_IN` names).  `qsat` is formed in the kernel from `ap` and `t`, and its perturbation from theirs by
    the derivative rule of `saturation_tl`.  LPHYLIN only (`ValueError` otherwise)."""
    return _call(_TL_STEP, False, state, perturbations, eta, dt, externals, want, write_nl=write_nl)


def tl_multi(state: Mapping[str, torch.Tensor], perturbations: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
             externals: Optional[Mapping[str, Any]] = None, *, want: Iterable[str], write_nl: bool = False,
             width: Optional[int] = None):
    """`tl_masked` for `ndir` perturbations of one state: `perturbations` maps `NL_IN` names to `(ndir, nx, 1, nz+1)`
    tensors (a missing name is zero in every direction).  Returns `(nl_outputs or None, {name: (ndir, nx, 1, nz+1)})`; the
    results are one `storage.zeros_batched` allocation per name, the NL outputs are written once.

    Directions are served in chunks of at most `width` (default `MULTI_WIDTH` of the dtype) per `cloudsc2_tl_multi_*`
    launch, which reads the state once per chunk; a chunk of one direction is a plain `tl_masked` launch.  Any `ndir >= 1`
    works.  A perturbation that is not laid out as `storage.zeros_batched` gives is copied into such a field first."""
    return _call(_TL_MASKED, True, state, perturbations, eta, dt, externals, want, write_nl=write_nl, width=width)


def tl_step_multi(state: Mapping[str, torch.Tensor], perturbations: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                  externals: Optional[Mapping[str, Any]] = None, *, want: Iterable[str], write_nl: bool = False,
                  width: Optional[int] = None):
    """`tl_step` for `ndir` perturbations of one state (`cloudsc2_tl_multi_step_*`; `STEP_IN` names): see `tl_multi`.
    `saturation` and its derivative are evaluated once per level for all directions of a chunk.  LPHYLIN only."""
    return _call(_TL_STEP, True, state, perturbations, eta, dt, externals, want, write_nl=write_nl, width=width)


def ad_masked(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
              externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str]):
    """Adjoint CLOUDSC2 with absent fields: `forcing` holds the adjoint forcing (`NL_OUT` names; a missing name is zero
    forcing), `traj` the `fplsl` / `fplsn` outputs of a `cloudsc2_nl` / `cloudsc2_tl` call on `state`, `want` names the
    inputs (`NL_IN` names) whose adjoints to produce.  Returns `{name: adjoint}` as new `storage.zeros` fields.
    LEVAPLS2 / LDRAIN1D are refused (`ValueError`), as by `cloudsc2_ad_from_trajectory`."""
    return _call(_AD_MASKED, False, state, forcing, eta, dt, externals, want, traj=traj)


def ad_step(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
            externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str]):
    """Adjoint of the step `saturation` + `cloudsc2_nl` in ONE launch (`cloudsc2_ad_step_*`): `ad_masked` without the field
    `qsat` (`STEP_IN` names).  The adjoint of `qsat` is not produced: it is taken through `saturation` by the rule of
    `saturation_ad` and arrives inside the adjoints of `t` and `ap`.  LPHYLIN only, and no LEVAPLS2 / LDRAIN1D."""
    return _call(_AD_STEP, False, state, forcing, eta, dt, externals, want, traj=traj)


def ad_multi(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
             externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
             width: Optional[int] = None):
    """`ad_masked` for `ndir` cotangents of one state: `forcing` maps `NL_OUT` names to `(ndir, nx, 1, nz+1)` tensors (a
    missing name is zero forcing in every direction); `traj` is not batched.  Returns `{name: (ndir, nx, 1, nz+1)}`, one
    `storage.zeros_batched` allocation per wanted name.

    Directions are served in chunks of at most `width` (default `AD_MULTI_WIDTH` of the dtype) per `cloudsc2_ad_multi_*`
    launch, which reads the state and recomputes the nonlinear trajectory once per chunk; a chunk of one direction is a
    plain `ad_masked` launch.  Any `ndir >= 1` works.  A forcing that is not laid out as `storage.zeros_batched` gives is
    copied into such a field first.  LEVAPLS2 / LDRAIN1D are refused (`ValueError`)."""
    return _call(_AD_MASKED, True, state, forcing, eta, dt, externals, want, traj=traj, width=width)


def ad_step_multi(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                  externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                  width: Optional[int] = None):
    """`ad_step` for `ndir` cotangents of one state (`cloudsc2_ad_multi_step_*`; `STEP_IN` names): see `ad_multi`.
    `saturation` and its derivative are evaluated once per level for all directions of a chunk.  LPHYLIN only, and no
    LEVAPLS2 / LDRAIN1D."""
    return _call(_AD_STEP, True, state, forcing, eta, dt, externals, want, traj=traj, width=width)


def ad_masked_evap(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                   externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                   cover: Optional[torch.Tensor] = None, cover_ready: bool = False):
    """`ad_masked` WITH the evaporation block (`cloudsc2_ad_evap_*`; LEVAPLS2 or LDRAIN1D must be set, `ValueError`
    otherwise): the same arguments and result.  `cover` is the field the launch parks the precipitation cover entering each
    level in (`storage` layout of the state; a new one when None).  `cover_ready=True`: `cover` already holds what an
    earlier such call left for the same state, `traj`, `eta`, `dt` and externals - it is only read, and the forward cover
    sweep is skipped.  `ad_masked_evap_ens` is the same call for the members of an ensemble."""
    return _call(_AD_MASKED_EVAP, False, state, forcing, eta, dt, externals, want, traj=traj, cover=cover,
                 cover_ready=cover_ready)


def ad_step_evap(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                 externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                 cover: Optional[torch.Tensor] = None, cover_ready: bool = False):
    """`ad_step` with the evaporation block in ONE launch (`cloudsc2_ad_evap_step_*`; `STEP_IN` names): see `ad_masked_evap`.
    LPHYLIN only."""
    return _call(_AD_STEP_EVAP, False, state, forcing, eta, dt, externals, want, traj=traj, cover=cover,
                 cover_ready=cover_ready)


def ad_multi_evap(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                  externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                  width: Optional[int] = None, cover: Optional[torch.Tensor] = None, cover_ready: bool = False):
    """`ad_multi` with the evaporation block (`cloudsc2_ad_evap_multi_*`): see `ad_multi` and `ad_masked_evap`.  The cover
    field is not batched; the first chunk of `width` cotangents fills it (unless `cover_ready`), every later chunk reads it
    (`cover_ready = 1`)."""
    return _call(_AD_MASKED_EVAP, True, state, forcing, eta, dt, externals, want, traj=traj, width=width, cover=cover,
                 cover_ready=cover_ready)


def ad_step_multi_evap(state: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                       externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor],
                       want: Iterable[str], width: Optional[int] = None, cover: Optional[torch.Tensor] = None,
                       cover_ready: bool = False):
    """`ad_step_multi` with the evaporation block (`cloudsc2_ad_evap_multi_step_*`; `STEP_IN` names): see `ad_multi_evap`.
    LPHYLIN only."""
    return _call(_AD_STEP_EVAP, True, state, forcing, eta, dt, externals, want, traj=traj, width=width, cover=cover,
                 cover_ready=cover_ready)


def tl_masked_ens(states: Mapping[str, torch.Tensor], perturbations: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                  externals: Optional[Mapping[str, Any]] = None, *, want: Iterable[str], write_nl: bool = False,
                  shared: Optional[Mapping[str, torch.Tensor]] = None):
    """`tl_masked` for an ENSEMBLE of `nmem` states in ONE launch (`cloudsc2_tl_ens_*`): `states` and `perturbations` map
    names to member-major `(nmem, nx, 1, nz+1)` tensors - the layout of `storage.zeros_batched`, of `torch.stack` and of
    every `*_multi` result; `eta`, `dt` and the externals are shared.  Every member is an independent `tl_masked` call.
    Returns `(nl_outputs or None, {name: (nmem, nx, 1, nz+1)})`, one `storage.zeros_batched` allocation per name.  A tensor
    that is not laid out like the first state field (as `zeros_batched` gives) is copied into such a field first.

    `shared` maps state names to plain `(nx, 1, nz+1)` fields that ALL members read (C ABI `cloudsc2_tl_enss_*`): a name is in
    exactly one of `states` and `shared` (`ValueError` otherwise); nothing is copied per member (a shared field in another
    layout is copied once, as one field).  `eta` may be `(nmem, nz+1)` with contiguous rows: one level vector per member."""
    return _call(_TL_MASKED, False, states, perturbations, eta, dt, externals, want, write_nl=write_nl, ens=True,
                 shared=shared)


def tl_step_ens(states: Mapping[str, torch.Tensor], perturbations: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                externals: Optional[Mapping[str, Any]] = None, *, want: Iterable[str], write_nl: bool = False,
                shared: Optional[Mapping[str, torch.Tensor]] = None):
    """`tl_step` for an ensemble of states in one launch (`cloudsc2_tl_step_ens_*`; `STEP_IN` names): see `tl_masked_ens`,
    also for `shared` and a per-member `eta` (`cloudsc2_tl_step_enss_*`)."""
    return _call(_TL_STEP, False, states, perturbations, eta, dt, externals, want, write_nl=write_nl, ens=True,
                 shared=shared)


def ad_masked_ens(states: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                  externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                  shared: Optional[Mapping[str, torch.Tensor]] = None):
    """`ad_masked` for an ensemble of `nmem` states in ONE launch (`cloudsc2_ad_ens_*`): `states`, `forcing` and `traj` map
    names to member-major `(nmem, nx, 1, nz+1)` tensors (see `tl_masked_ens`); every member is an independent `ad_masked`
    call.  Returns `{name: (nmem, nx, 1, nz+1)}`.  LEVAPLS2 / LDRAIN1D are refused (`ValueError`).
    `shared` and a per-member `eta` as in `tl_masked_ens` (`cloudsc2_ad_enss_*`).  The adjoint of a shared input is returned
    PER MEMBER like every other; the adjoint of the shared field itself is its sum over the members.  The evaporation
    (`ad_masked_evap_ens`) and members-times-directions (`ad_multi_ens`) calls take no `shared`: materialise the members."""
    return _call(_AD_MASKED, False, states, forcing, eta, dt, externals, want, traj=traj, ens=True, shared=shared)


def ad_step_ens(states: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                shared: Optional[Mapping[str, torch.Tensor]] = None):
    """`ad_step` for an ensemble of states in one launch (`cloudsc2_ad_step_ens_*`; `STEP_IN` names): see `ad_masked_ens`,
    also for `shared` and a per-member `eta` (`cloudsc2_ad_step_enss_*`)."""
    return _call(_AD_STEP, False, states, forcing, eta, dt, externals, want, traj=traj, ens=True, shared=shared)


def ad_masked_evap_ens(states: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                       externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                       cover: Optional[torch.Tensor] = None, cover_ready: bool = False):
    """`ad_masked_evap` for an ensemble of `nmem` states in ONE launch (`cloudsc2_ad_evap_ens_*`; LEVAPLS2 or LDRAIN1D must be
    set): the arguments and the result of `ad_masked_ens`, one cotangent per member.  `cover` is member-major like every
    other tensor of the call, `(nmem, nx, 1, nz+1)` as `storage.zeros_batched` gives (a new one when None); the launch
    parks every member's precipitation cover in it.  `cover_ready=True`: `cover` holds what an earlier such call left for
    the same states, `traj`, `eta`, `dt` and externals, and is only read.  A `cover` in another layout is copied into the
    call's like any other tensor, and what the launch parked is copied back into it."""
    return _call(_AD_MASKED_EVAP, False, states, forcing, eta, dt, externals, want, traj=traj, ens=True, cover=cover,
                 cover_ready=cover_ready)


def ad_step_evap_ens(states: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                     externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                     cover: Optional[torch.Tensor] = None, cover_ready: bool = False):
    """`ad_step_evap` for an ensemble of states in one launch (`cloudsc2_ad_evap_step_ens_*`; `STEP_IN` names): see
    `ad_masked_evap_ens`.  LPHYLIN only."""
    return _call(_AD_STEP_EVAP, False, states, forcing, eta, dt, externals, want, traj=traj, ens=True, cover=cover,
                 cover_ready=cover_ready)


def ad_multi_ens(states: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                 externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor], want: Iterable[str],
                 width: Optional[int] = None):
    """`ad_multi` for an ENSEMBLE of `nmem` states: members TIMES directions, an ensemble of Jacobian row blocks (C ABI
    `cloudsc2_ad_multi_ens_*`).  `states` and `traj` map names to member-major `(nmem, nx, 1, nz+1)` tensors (see
    `ad_masked_ens`), `forcing` maps `NL_OUT` names to `(nmem, ndir, nx, 1, nz+1)` tensors (a missing name is zero forcing in
    every member and direction).  Returns `{name: (nmem, ndir, nx, 1, nz+1)}`: one allocation per wanted name, laid out as
    `nmem` consecutive `storage.zeros_batched(ndir, ...)` blocks.

    Directions are served in chunks of at most `width` (default `AD_MULTI_WIDTH` of the dtype); each chunk is ONE launch for
    all members.  A chunk of one direction is the same entry with `ndir = 1`, not `ad_masked_ens`: that entry has one member
    stride for every field of the call, and here states, forcings and results are three allocations with three strides.
    A forcing that is not member-major with the first forcing's strides (packed, as `torch.stack` of `zeros_batched` fields
    or a result of this call, if the first is in some other layout) is copied once.  LEVAPLS2 / LDRAIN1D are refused
    (`ValueError`)."""
    return _call(_AD_MASKED, True, states, forcing, eta, dt, externals, want, traj=traj, width=width, ens=True)


def ad_step_multi_ens(states: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                      externals: Optional[Mapping[str, Any]] = None, *, traj: Mapping[str, torch.Tensor],
                      want: Iterable[str], width: Optional[int] = None):
    """`ad_step_multi` for an ensemble of states, one launch per chunk of cotangents (`cloudsc2_ad_multi_step_ens_*`;
    `STEP_IN` names): see `ad_multi_ens`.  LPHYLIN only, and no LEVAPLS2 / LDRAIN1D."""
    return _call(_AD_STEP, True, states, forcing, eta, dt, externals, want, traj=traj, width=width, ens=True)


def _member_directions(what: str, noun: str, dirs, first: torch.Tensor, geo, nmem: int):
    """the `(nmem, ndir, nx, 1, nlev)` forcings of a members-times-directions call -> (them in ONE member-major layout, ndir,
    direction stride, member stride): the first tensor's own strides if it is such a batch of column-fastest fields of the
    call's geometry whose directions lie inside its member stride, else packed; whatever differs is copied once"""
    nx, nlev, ls = geo
    field = nlev * ls
    shapes = {tuple(getattr(f, "shape", ())) for f in dirs.values()}
    shape = next(iter(shapes)) if len(shapes) == 1 else ()
    if len(shape) != 5 or shape[0] != nmem or shape[1] < 1 or shape[2:] != (nx, 1, nlev):
        raise ValueError(f"{what}: every {noun} must be a tensor of one shape ({nmem}, ndir, {nx}, 1, {nlev}), got "
                         f"{ {n: tuple(getattr(f, 'shape', ())) for n, f in dirs.items()} }")
    ndir = shape[1]

    def strides(g):     # (direction stride, member stride) of a batch in a layout the kernel takes, else None
        if g.dtype != first.dtype or g.device != first.device:
            return None
        try:
            if field_geometry(g[0, 0]) != geo:
                return None
        except ValueError:
            return None
        ds = g.stride(1) if ndir > 1 else field
        ms = g.stride(0) if nmem > 1 else (ndir - 1) * ds + field
        return (ds, ms) if ds >= field and ms >= (ndir - 1) * ds + field else None

    plain = {n: _plain(f) for n, f in dirs.items()}
    ds, ms = strides(next(iter(plain.values()))) or (field, ndir * field)
    out = {}
    for n, g in plain.items():
        if strides(g) != (ds, ms):
            f = torch.zeros(nmem * ms, dtype=first.dtype, device=first.device).as_strided(
                (nmem, ndir, nx, 1, nlev), (ms, ds, 1, field, ls))
            f.copy_(g)
            g = f
        out[n] = g
    return out, ndir, ds, ms


def _batched_layout(g: torch.Tensor, ref: torch.Tensor, geo, stride: Optional[int] = None) -> torch.Tensor:
    """`g` as `ndir` fields of the call's geometry, one field behind the other (`stride` elements apart; by default packed,
    as `zeros_batched` gives): itself, or a copy into such an allocation (what `_in_layout` is for one direction)"""
    g = _plain(g)
    nx, nlev, ls = geo
    stride = nlev * ls if stride is None else stride
    if g.dtype == ref.dtype and g.device == ref.device and g.dim() == 4 and tuple(g.shape[1:]) == (nx, 1, nlev):
        try:
            if field_geometry(g[0]) == geo and direction_stride(g) == stride:
                return g
        except ValueError:
            pass
    f = _zeros_members(g.shape[0], geo, ref.dtype, ref.device, stride)
    f.copy_(g)
    return f


def _zeros_members(n: int, geo, dtype, device, stride: int) -> torch.Tensor:
    """`zeros_batched` with `stride` elements from one entry to the next (packed: one `zeros_batched` allocation)"""
    nx, nlev, ls = geo
    if stride == nlev * ls:
        return zeros_batched(n, nx, nlev - 1, dtype, device, ls)
    return torch.zeros((n, stride), dtype=dtype, device=device)[:, :nlev * ls].view(n, nlev, ls)[:, :, :nx] \
        .unsqueeze(2).permute(0, 3, 2, 1)


def _ens_geometry(what: str, first: torch.Tensor):
    """(nmem, (nx, nlev, lev_stride), member stride) an ensemble call takes from its first state tensor: that tensor's own
    if it is a batch of column-fastest fields, else the packed `zeros_batched` layout it will be copied into"""
    if not isinstance(first, torch.Tensor) or first.dim() != 4 or first.shape[2] != 1 or first.shape[0] < 1:
        raise ValueError(f"{what}: every field must be a member-major (nmem, nx, 1, nz+1) tensor, got "
                         f"{tuple(getattr(first, 'shape', ()))}")
    if not first.is_cuda:
        raise ValueError(f"{what}: fields live on {first.device}; they must live on the GPU (there is no host path)")
    try:
        geo = field_geometry(first[0])
        return first.shape[0], geo, direction_stride(first)
    except ValueError:
        nx, nlev = first.shape[1], first.shape[3]
        geo = (nx, nlev, level_pitch(nx, first.dtype))
        return first.shape[0], geo, geo[1] * geo[2]


def _batch_size(what, noun, dirs, names, geo) -> int:
    """`dirs`, the `ndir` perturbations / forcings of a multi call: known names, at least one, all GPU tensors of the one
    shape (ndir, nx, 1, nlev) -> ndir"""
    nx, nlev, _ = geo
    unknown = sorted(set(dirs) - set(names))
    if unknown:
        raise ValueError(f"{what}: unknown field names {unknown}")
    if not dirs:
        raise ValueError(f"{what}: no {noun} given")
    shapes = {tuple(f.shape) for f in dirs.values() if isinstance(f, torch.Tensor)}
    shape = next(iter(shapes)) if len(shapes) == 1 else ()
    if len(shape) != 4 or shape[1:] != (nx, 1, nlev) or shape[0] < 1:
        raise ValueError(f"{what}: every {noun} must be a tensor of one shape (ndir, {nx}, 1, {nlev}), got "
                         f"{ {n: tuple(getattr(f, 'shape', ())) for n, f in dirs.items()} }")
    for n, f in dirs.items():
        if not f.is_cuda:
            raise ValueError(f"{what}: {n} lives on {f.device}; fields must live on the GPU (there is no host path)")
    return shape[0]


def _tl_args(p, geo, state, pert, zero_line, eta, out, out_i, dt, stream, tail=()):
    """the arguments of `cloudsc2_tl_masked_*` / `_tl_step_*`; with `tail` = (ndir, in_dir_stride, out_dir_stride) those of
    their multi-direction forms (`_lib.MULTI_LAYOUTS`)"""
    nx, nlev, ls = geo
    return (ctypes.byref(p), nx, nlev - 1, ls, _ptrs(state, NL_IN), _ptrs(pert, NL_IN), zero_line.data_ptr(), eta.data_ptr(),
            None if out is None else _ptrs(out, NL_OUT), _ptrs(out_i, NL_OUT), float(dt), stream) + tail


def _ad_args(p, geo, state, forcing, zero_line, eta, traj, out_adj, dt, stream, tail=(), cover=(), members=()):
    """the arguments of `cloudsc2_ad_masked_*` / `_ad_step_*`; `tail` as for `_tl_args`; `cover` = (pointer, cover_ready):
    those of the `cloudsc2_ad_evap_*` entries (`_lib.EVAP_LAYOUTS`) - in front of `stream`, or behind a multi entry's `tail`;
    `members` = (nmem, member_stride): those of the ensemble form of either (`_lib.ENS_LAYOUTS`, `_lib.EVAP_ENS_LAYOUTS`), or
    with `tail` (nmem, member_stride, in_member_stride, out_member_stride) of `_lib.MULTI_ENS_LAYOUTS`"""
    nx, nlev, ls = geo
    head = (ctypes.byref(p), nx, nlev - 1, ls, _ptrs(state, NL_IN), _ptrs(forcing, NL_OUT), zero_line.data_ptr(),
            eta.data_ptr(), traj["fplsl"].data_ptr(), traj["fplsn"].data_ptr(), _ptrs(out_adj, NL_IN), float(dt))
    return (head + (stream,) + tail + cover if tail else head + cover + (stream,)) + members


def _eta_members(what: str, eta, nz: int, nmem: int, dtype, device) -> Tuple[torch.Tensor, int]:
    """`eta` of an ensemble call -> (it, its member stride in elements): 1-D, one level vector for all members (stride 0), or
    `(nmem, >= nz+1)` with contiguous rows, one per member (packed, or rows of a wider buffer)"""
    if isinstance(eta, torch.Tensor) and eta.dim() == 2:
        if (eta.shape[0] != nmem or eta.shape[1] < nz + 1 or eta.dtype != dtype or eta.device != device or eta.stride(1) != 1
                or (nmem > 1 and eta.stride(0) < nz + 1)):
            raise ValueError(f"{what}: a per-member eta must be a ({nmem}, >= {nz + 1}) {dtype} tensor on {device} with "
                             f"contiguous rows, got shape {tuple(eta.shape)}, strides {eta.stride()}, {eta.dtype} on {eta.device}")
        return eta, (eta.stride(0) if nmem > 1 else eta.shape[1])
    return _eta(what, eta, nz, dtype, device), 0


def _shared_entry(what: str, fam_names, states, shared, eta) -> bool:
    """does an ensemble call take the shared-state entry (`_lib.ENSS_LAYOUTS`)?  With `shared` given, or a 2-D `eta`.  A name
    must be in exactly one of `states` and `shared`."""
    if shared is None:
        return isinstance(eta, torch.Tensor) and eta.dim() == 2
    both, missing = sorted(set(states) & set(shared)), sorted(set(fam_names) - set(states) - set(shared))
    unknown = sorted(set(shared) - set(fam_names))
    if both or missing or unknown:
        raise ValueError(f"{what}: every state field must be in exactly one of `states` and `shared`: in both {both}, in "
                         f"neither {missing}, unknown shared names {unknown}")
    return True


def _block_order_bits() -> int:
    if BLOCK_ORDER not in (None, "member", "column"):
        raise ValueError(f"autodiff.BLOCK_ORDER must be None, 'member' or 'column', got {BLOCK_ORDER!r}")
    return {None: 0, "member": _lib.ENSS_MEMBER_MAJOR, "column": _lib.ENSS_COLUMN_MAJOR}[BLOCK_ORDER]


def _shared_fields(what: str, shared, ref: torch.Tensor, geo) -> Dict[str, torch.Tensor]:
    """the shared fields of an ensemble call as plain `(nx, 1, nlev)` fields of the call's geometry: themselves, or ONE copy
    each (never one per member)"""
    nx, nlev, _ = geo
    for n, f in shared.items():
        if not isinstance(f, torch.Tensor) or tuple(f.shape) != (nx, 1, nlev):
            raise ValueError(f"{what}: shared field {n} must be a plain ({nx}, 1, {nlev}) field like one member of the state, "
                             f"got {tuple(getattr(f, 'shape', ()))}")
    if ref is None:       # the shapes only
        return {}
    for n, f in shared.items():
        if not f.is_cuda:
            raise ValueError(f"{what}: {n} lives on {f.device}; fields must live on the GPU (there is no host path)")
    return {n: _in_layout(f, ref, geo) for n, f in shared.items()}


def _call(fam: _Family, batched: bool, state, dirs, eta, dt, externals, want, *, traj=None, write_nl=False, width=None,
          ens=False, cover=None, cover_ready=False, shared=None):
    """The launch path of the twenty thin calls.  Everything is checked ONCE, up front; then the directions are served in
    chunks of at most `width`: a chunk of one direction by the single-direction entry, a wider one by the multi-direction
    entry.  `batched`: `dirs` maps names to (ndir, nx, 1, nlev) batches and so do the results, which are one `zeros_batched`
    allocation per wanted name that every chunk writes through the views `f[d0]`; otherwise `dirs` and the results are
    single fields and there is one launch.  The NL outputs of `write_nl` are new fields, written by the first launch.
    `ens`: EVERY tensor of the call - state, `dirs`, `traj`, the results - is a member-major (nmem, nx, 1, nlev) batch of one
    layout (that of the first state tensor, `_ens_geometry`); the checks run on member 0 and ONE launch of the family's
    ensemble entry, given member 0's pointers and (nmem, member stride), serves all members.
    `ens` and `batched` (the adjoint families without the evaporation block): members times directions - `dirs` and the
    results are (nmem, ndir, nx, 1, nlev), and every chunk of `width` directions is ONE launch of the family's `mens` entry.
    `cover`, `cover_ready`: the evaporation families' cover field (a new one when None); every chunk behind the first reads
    what the first left in it.  With `ens` it is a member-major batch like every other tensor of the call."""
    mens = ens and batched     # members times directions: `dirs` and the results are (nmem, ndir, nx, 1, nlev)
    if ens and not mens and fam.ens in _lib.ENS_LAYOUTS:
        state, shared = _expanded_as_shared(state, shared)
    what = (fam.mens if mens else fam.ens) if ens else fam.multi if batched else fam.single
    enss = ens and not mens and what in _lib.ENS_LAYOUTS and _shared_entry(what, fam.names, state, shared, eta)
    if (shared is not None or (ens and isinstance(eta, torch.Tensor) and eta.dim() == 2)) and not enss:
        raise ValueError(f"{what}: shared state fields and a per-member eta are served by the six plain ensemble families "
                         f"only ({sorted(_lib.ENSS_LAYOUTS)}): materialise the members for this call")
    if enss:
        what = what.replace("_ens", "_enss")
    if ens and not what:
        raise ValueError(f"{fam.multi}: members times directions in one call has no kernel in this family")
    noun, dir_names, res_names = ("forcing", NL_OUT, fam.names) if fam.adjoint else ("perturbation", fam.names, NL_OUT)
    want = tuple(want)
    if not want or set(want) - set(res_names):
        raise ValueError(f"{what}: `want` must name at least one of {res_names}, got {want}")
    nmem = mstride = 0
    cover_given = cover_all = None
    if ens:
        # the first tensor that has members: of the state, or (every state field shared) of the forcing / perturbations
        first = state.get(fam.names[0])
        if enss:
            first = next((state[n] for n in fam.names if n in state), next(iter(dirs.values()), None))
        if shared and isinstance(first, torch.Tensor) and first.dim() == 4:     # shapes first: they need no device
            _shared_fields(what, shared, None, (first.shape[1], first.shape[3], 0))
        nmem, egeo, mstride = _ens_geometry(what, first)

        def laid_out(fields):    # -> every tensor in the call's layout
            for n, f in fields.items():
                if not isinstance(f, torch.Tensor) or tuple(f.shape) != (nmem, egeo[0], 1, egeo[1]):
                    raise ValueError(f"{what}: {n} must be a tensor of shape {(nmem, egeo[0], 1, egeo[1])} like the state's "
                                     f"{fam.names[0]}, got {tuple(getattr(f, 'shape', ()))}")
            return {n: _batched_layout(f, first, egeo, mstride) for n, f in fields.items()}

        def members(fields):    # -> member 0 of every tensor, in the call's layout
            return {n: f[0] for n, f in laid_out(fields).items()}
        state = members(state)
        if shared:
            state.update(_shared_fields(what, shared, _plain(first), egeo))
        if mens:
            unknown = sorted(set(dirs) - set(dir_names))
            if unknown or not dirs:
                raise ValueError(f"{what}: unknown field names {unknown}" if unknown else f"{what}: no {noun} given")
            dirs_all, _, in_ds, in_ms = _member_directions(what, noun, dirs, first, egeo, nmem)
            dirs = {n: f[0] for n, f in dirs_all.items()}     # member 0's (ndir, nx, 1, nlev): what the checks below see
        else:
            dirs = members(dirs)
        traj = members(traj) if fam.adjoint else None
        if cover is not None:   # the checks below see member 0, the launch gets the batch
            cover_given, cover_all = cover, laid_out({"cover": cover})["cover"]
            cover = cover_all[0]
    state = {n: _plain(f) for n, f in state.items()}
    groups = [(state, fam.names, True)]
    if not batched:
        dirs = {n: _plain(f) for n, f in dirs.items()}
        groups.append((dirs, dir_names, False))
    if fam.adjoint:
        traj = {n: _plain(f) for n, f in traj.items()}
        groups.append((traj, ("fplsl", "fplsn"), True))
    evap = fam.single in _lib.EVAP_LAYOUTS
    if evap and cover is not None:
        groups.append(({"cover": _plain(cover)}, ("cover",), True))
    elif cover_ready:
        raise ValueError(f"{what}: cover_ready without a `cover` field that an earlier call filled")
    geo, dtype, device = _checked(what, groups)
    nx, nlev, ls = geo
    nz = nlev - 1
    ndir = _batch_size(what, noun, dirs, dir_names, geo) if batched else 1
    eta, eta_ms = _eta_members(what, eta, nz, nmem, dtype, device) if enss else (_eta(what, eta, nz, dtype, device), 0)
    ref = state[NL_IN[0]]
    if batched:
        width = fam.width[dtype] if width is None else int(width)
        if not 1 <= width <= fam.max_dirs:
            raise ValueError(f"{what}: width={width} outside [1, {fam.max_dirs}]")
        if not mens:
            dirs = {n: _batched_layout(f, ref, geo) for n, f in dirs.items()}
            res = {n: zeros_batched(ndir, nx, nz, dtype, device, ls) for n in want}
    elif not ens:
        width = 1
        res = {n: _new_like(ref, nx, nz, ls) for n in want}
    out = {n: _new_like(ref, nx, nz, ls) for n in NL_OUT} if write_nl and not ens else None
    p = _params(externals, nz)
    lib, zero, dstride = _lib.load(), _zero_line(device, dtype), nlev * ls
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    if evap and not ens:
        cover = _new_like(ref, nx, nz, ls) if cover is None else _plain(cover)
    if mens:     # one launch per chunk of directions, all members; the results packed: nmem blocks of `zeros_batched(ndir)`
        res = {n: zeros_batched(nmem * ndir, nx, nz, dtype, device, ls).unflatten(0, (nmem, ndir)) for n in want}
        with torch.cuda.device(device):
            for d0 in range(0, ndir, width):
                n = min(width, ndir - d0)
                args = _ad_args(p, geo, state, {k: f[0, d0] for k, f in dirs_all.items()}, zero, eta, traj,
                                {k: f[0, d0] for k, f in res.items()}, dt, stream, (n, in_ds, dstride),
                                members=(nmem, mstride, in_ms, ndir * dstride))
                _lib.check(getattr(lib, f"cloudsc2_{fam.mens}_{_SFX[dtype]}")(*args), fam.mens)
        return res
    if ens:
        new = lambda: _zeros_members(nmem, geo, dtype, device, mstride)  # noqa: E731
        res, out = {n: new() for n in want}, ({n: new() for n in NL_OUT} if write_nl else None)
        r0, o0 = {n: f[0] for n, f in res.items()}, (None if out is None else {n: f[0] for n, f in out.items()})
        park = ()
        if fam.adjoint and evap:
            cover_all = new() if cover_all is None else cover_all
            park = (cover_all[0].data_ptr(), int(bool(cover_ready)))
        group = (nmem, mstride)     # + (shared_mask, eta_member_stride) for the shared-state entries
        if enss:
            group += (sum(1 << NL_IN.index(n) for n in shared or ()) | _block_order_bits(), eta_ms)
        if fam.adjoint:
            args = _ad_args(p, geo, state, dirs, zero, eta, traj, r0, dt, stream, cover=park, members=group)
        else:
            args = _tl_args(p, geo, state, dirs, zero, eta, o0, r0, dt, stream, group)
        with torch.cuda.device(device):
            _lib.check(getattr(lib, f"cloudsc2_{what}_{_SFX[dtype]}")(*args), what)
        if cover_given is not None and not cover_ready and cover_all.data_ptr() != cover_given.data_ptr():
            _plain(cover_given).copy_(cover_all)     # the caller's field was in another layout: hand back what was parked
        return res if fam.adjoint else (out, res)
    with torch.cuda.device(device):
        for d0 in range(0, ndir, width):
            n = min(width, ndir - d0)
            entry = fam.single if n == 1 else fam.multi
            tail = () if n == 1 else (n, dstride, dstride)
            d = {k: f[d0] for k, f in dirs.items()} if batched else dirs
            r = {k: f[d0] for k, f in res.items()} if batched else res
            if fam.adjoint:
                park = (cover.data_ptr(), int(bool(cover_ready) or d0 > 0)) if evap else ()
                args = _ad_args(p, geo, state, d, zero, eta, traj, r, dt, stream, tail, park)
            else:
                args = _tl_args(p, geo, state, d, zero, eta, out if d0 == 0 else None, r, dt, stream, tail)
            _lib.check(getattr(lib, f"cloudsc2_{entry}_{_SFX[dtype]}")(*args), entry)
    return res if fam.adjoint else (out, res)


def _in_layout(g: torch.Tensor, ref: torch.Tensor, geo) -> torch.Tensor:
    """`g` as a field of the call's geometry: itself, or a copy into a `storage.zeros` field (autograd hands over whatever
    layout the consumer produced, e.g. the stride-0 expansion of `.sum().backward()`)"""
    g = _plain(g)
    nx, nlev, ls = geo
    if g.dtype == ref.dtype and g.device == ref.device and tuple(g.shape) == (nx, 1, nlev):
        try:
            if field_geometry(g) == geo:
                return g
        except ValueError:
            pass
    f = _new_like(ref, nx, nlev - 1, ls)
    f.copy_(g)
    return f


# ---- the launches behind the derivative rules, as Functions of their own ---------------------------------------------------
# `backward` and `jvp` of the public Functions touch no storage: they hand what they were given to one of these, which holds
# the layout normalisation and the launch - and a `vmap` rule, so that under `torch.func.vmap` (`jacfwd`, `jacrev`, `vmap` of
# `jvp`) the rule sees all tangents / cotangents stacked, as ordinary tensors.  Outside `vmap` they are plain calls.
_BATCHED_STATE = ("`vmap` over the state (a primal input of cloudsc2 / cloudsc2_step / saturation) runs the ensemble "
                  "launches, and `vmap` over tangents or cotangents the multi-direction ones, but not both at once: members "
                  "times directions in one call (nested `vmap`, e.g. `vmap(jacrev(f))` or `vmap(vmap(f))`) is not supported "
                  "- loop over the members, or over the directions")
_BATCHED_ETA = ("`eta` is shared by all members of an ensemble: `vmap` over `eta` is not supported (in_dims must be None for "
                "it) - loop over the level vectors")
_PARTLY_BATCHED = ("beside a state of which SOME fields are batched and others are not, only tangents and cotangents may be "
                   "batched: `vmap` over part of the state (of the primal inputs of cloudsc2 / cloudsc2_step / saturation) is "
                   "not supported - an ensemble is a batch of WHOLE states: batch every field of the state (`torch.stack`, or "
                   "`expand` the fields the members share), which runs the ensemble launch")


def _whole_state(dims) -> bool:
    """the `in_dims` of the state's tensors under `vmap`: all batched (an ensemble: True) or none (False); a state batched
    in part is refused, as every batched state was before there were ensemble launches"""
    batched = [d is not None for d in dims]
    if any(batched) and not all(batched):
        raise NotImplementedError(_PARTLY_BATCHED)
    return any(batched)


def _nested(tensors) -> bool:
    return any(isinstance(t, torch.Tensor) and torch._C._functorch.is_batchedtensor(t) for t in tensors)


def _refuse_nested(tensors) -> None:
    """a tensor still wrapped for an OUTER `vmap` inside a `vmap` rule: members times directions"""
    if _nested(tensors):
        raise NotImplementedError(_BATCHED_STATE)


def _as_field(t: torch.Tensor) -> torch.Tensor:
    """a (nx, 1, nlev) tensor of any layout as a column-fastest field (differentiable; what the looping fallbacks hand a
    member to the single paths as)"""
    return t.permute(2, 1, 0).contiguous().permute(2, 1, 0)


def _members(info, in_dims, tensors):
    """every tensor of a `vmap` rule member-major, (batch, nx, 1, nlev): batched ones moved, unbatched ones expanded"""
    return [t.unsqueeze(0).expand(info.batch_size, *t.shape) if d is None else t.movedim(d, 0)
            for t, d in zip(tensors, in_dims)]


class _Launch(NamedTuple):
    """what a launch needs beside its tensors; `have`: the names of the tangents / cotangents that follow the fixed tensors
    (absent ones are `None` in autograd and are not passed); `want`: the adjoints to produce (AD)"""
    eta: Optional[torch.Tensor]
    dt: float
    ext: Mapping[str, Any]
    geo: Tuple[int, int, int]
    have: Tuple[str, ...]
    want: Tuple[str, ...] = ()


def _batched_state(in_dims, nfixed) -> bool:
    """in_dims[0] belongs to the `_Launch` (a tuple like it: `eta` is its one tensor), the next `nfixed` to the state and
    the trajectory: is any of those batched (an ensemble)?  A batched `eta` is refused, and so is a state batched in part -
    unless `SHARED_STATE` is set: then either makes an ensemble, whose unbatched state fields the members share."""
    if not SHARED_STATE:
        if in_dims[0].eta is not None:
            raise NotImplementedError(_BATCHED_ETA)
        return _whole_state(in_dims[1:1 + nfixed])
    return in_dims[0].eta is not None or any(d is not None for d in in_dims[1:1 + nfixed])


def _ens_members(info, in_dims, call, tensors, nstate=0):
    """what a `vmap` rule hands the ensemble path: (`call` with a batched `eta` as contiguous (batch, nlev) rows, every tensor
    member-major as `_members` gives).  `SHARED_STATE`: an unbatched tensor among the first `nstate`, the state's fields, stays a
    plain (nx, 1, nlev) field - the members share it - as long as another tensor of the call carries the members."""
    if in_dims[0].eta is not None:
        call = call._replace(eta=call.eta.movedim(in_dims[0].eta, 0).contiguous())
    dims = in_dims[1:]
    keep = nstate if SHARED_STATE and any(d is not None for d in dims) else 0
    return call, [t if d is None and i < keep else t.unsqueeze(0).expand(info.batch_size, *t.shape) if d is None
                  else t.movedim(d, 0) for i, (t, d) in enumerate(zip(tensors, dims))]


def _stacked(info, in_dims, tensors, nfixed):
    """the tangents / cotangents behind the `nfixed` state tensors, each as (batch, nx, 1, nlev)"""
    return [t.unsqueeze(0).expand(info.batch_size, *t.shape) if d is None else t.movedim(d, 0)
            for t, d in zip(tensors[nfixed:], in_dims[1 + nfixed:])]


class _InnerFunction(torch.autograd.Function):
    """no derivative of its own (second derivatives are not available): it exists for its `vmap` rule"""
    @staticmethod
    def setup_context(ctx, inputs, output):
        pass


def _unpacked(names, step, adjoint, call, tensors, info=None, in_dims=None):
    """`(call, *tensors)` of an inner Function -> state, `qsat` or None, `traj` or None, present tangents / cotangents by name.
    The fixed tensors come first: the `names` of the state, for a `step` its `qsat`, for an `adjoint` the two trajectory
    fluxes.  `forward`: every tangent / cotangent becomes a field of the call's geometry; `vmap` (`info`, `in_dims` given):
    they are stacked as (batch, nx, 1, nlev), and a batched state is refused."""
    nst = len(names)
    nfixed = nst + step + 2 * adjoint
    if call.geo is None:      # an ensemble: `_call` brings every member-major tensor into one layout
        rest = list(tensors[nfixed:])
    elif info is None:
        ref = _plain(tensors[0])
        rest = [_in_layout(t, ref, call.geo) for t in tensors[nfixed:]]
    else:
        rest = _stacked(info, in_dims, tensors, nfixed)
    qsat = tensors[nst] if step else None
    traj = {"fplsl": tensors[nfixed - 2], "fplsn": tensors[nfixed - 1]} if adjoint else None
    return dict(zip(names, tensors)), qsat, traj, dict(zip(call.have, rest))


def _saturation_tl_stacked(ap, t, pert, ext, geo):
    """`saturation_tl` per direction (pointwise and cheap: it loops) -> the qsat perturbations as one batch"""
    nx, nlev, ls = geo
    ref = _plain(ap)
    ndir = next(iter(pert.values())).shape[0]
    lay = lambda n, d: _in_layout(pert[n][d], ref, geo) if n in pert else None  # noqa: E731
    qsat_i = zeros_batched(ndir, nx, nlev - 1, ref.dtype, ref.device, ls)
    for d in range(ndir):
        qsat_i[d].copy_(saturation_tl(ap, t, lay("ap", d), lay("t", d), ext)[1])
    return qsat_i


def _split_shared(state, dirs):
    """the state of an ensemble Function -> (its member-major fields, its shared `(nx, 1, nlev)` fields or None, nmem)"""
    shared = {n: f for n, f in state.items() if f.dim() == 3}
    members = {n: f for n, f in state.items() if f.dim() != 3}
    nmem = max((t.shape[0] for t in list(members.values()) + list(dirs.values()) if t.dim() == 4), default=1)
    return members, (shared or None), nmem


def _looped_members(one, call, tensors, nout):
    """an ensemble where there is no ensemble kernel (the evaporation switches in the adjoint, the non-LPHYLIN step): the
    single path `one(call, *fields)` member by member, results stacked member-major"""
    rows = []
    for m in range(max(t.shape[0] for t in tensors if t.dim() == 4)):     # a (nx, 1, nlev) tensor is shared by the members
        fields = [_as_field(_plain(t)[m] if t.dim() == 4 else _plain(t)) for t in tensors]
        eta = call.eta[m] if call.eta is not None and call.eta.dim() == 2 else call.eta     # `saturation` has none
        rows.append(one(call._replace(geo=field_geometry(fields[0]), eta=eta), *fields))
    return tuple(torch.stack([r[i] for r in rows]) for i in range(nout))


def _tl_rule(fam, call, tensors, info=None, in_dims=None):
    """`forward` and, with `info` and `in_dims`, `vmap` of `_TLMasked` / `_TLStep`: batched tangents take the family's
    multi-direction launches.  The step without LPHYLIN has no kernel of its own: the qsat perturbation comes from
    `saturation_tl`, then the masked family runs on the step's `qsat`."""
    batched, step = info is not None, fam is _TL_STEP
    nfixed = len(fam.names) + step
    if batched:
        if ENSEMBLE_JACOBIANS and _nested(tensors[:nfixed]) and not _batched_state(in_dims, nfixed):
            return _members_times_directions(fam, call, tensors, info, in_dims, nfixed)
        _refuse_nested(tensors)
        if _batched_state(in_dims, nfixed):     # an ensemble of states: every tensor member-major, one ensemble launch
            call, members = _ens_members(info, in_dims, call, tensors, len(fam.names))
            outs = _tl_rule(fam, call._replace(geo=None), members)
            return outs, (0,) * len(outs)
    if call.geo is None:
        if step and not call.ext.get("LPHYLIN"):     # no ensemble kernel: the single path, member by member
            return _looped_members(lambda c, *t: _tl_rule(fam, c, t), call, tensors, len(NL_OUT))
        state, _, _, pert = _unpacked(fam.names, step, False, call, tensors)
        state, shared, nmem = _split_shared(state, pert)
        pert = {n: t if t.dim() == 4 else t.unsqueeze(0).expand(nmem, *t.shape) for n, t in pert.items()}
        out_i = _call(fam, False, state, pert, call.eta, call.dt, call.ext, NL_OUT, ens=True, shared=shared)[1]
        return tuple(out_i[n] for n in NL_OUT)
    state, qsat, _, pert = _unpacked(fam.names, step, False, call, tensors, info, in_dims)
    if step and not call.ext.get("LPHYLIN"):
        if batched and ("ap" in pert or "t" in pert):
            sat = {n: pert[n] for n in ("ap", "t") if n in pert}
            pert["qsat"] = _saturation_tl_stacked(state["ap"], state["t"], sat, call.ext, call.geo)
        elif "ap" in pert or "t" in pert:
            pert["qsat"] = saturation_tl(state["ap"], state["t"], pert.get("ap"), pert.get("t"), call.ext)[1]
        fam, state = _TL_MASKED, dict(state, qsat=qsat)
    out_i = _call(fam, batched, state, pert, call.eta, call.dt, call.ext, NL_OUT)[1]
    outs = tuple(out_i[n] for n in NL_OUT)
    return (outs, (0,) * len(outs)) if batched else outs


# ---- members times directions (opt-in: `ENSEMBLE_JACOBIANS`) ------------------------------------------------------------------
# A direction-level `vmap` rule whose STATE is still wrapped for an outer `vmap` - the inner level of `vmap(jacrev(f))`, of
# `vmap(vmap(vjp_fn))`, of `vmap(jacfwd(f))` - stacks its tangents / cotangents as ever and hands them, with the still-wrapped
# state, to `_MembersDirs`: a Function of (call, the fixed tensors, stacked (ndir, nx, 1, nlev) directions) whose own `vmap`
# rule is reached at the OUTER level, with a whole state batched.  Directions outer and members inner (`jacrev` applied outside
# `cloudsc2_ensemble`) never gets here: there the state is plain and the cotangents carry two batch levels.
def _members_times_directions(fam, call, tensors, info, in_dims, nfixed):
    outs = _MembersDirs.apply(fam.single, call, nfixed, *tensors[:nfixed], *_stacked(info, in_dims, tensors, nfixed))
    return tuple(outs), (0,) * len(outs)


class _Directions(NamedTuple):
    """what `_tl_rule` / `_ad_rule` read of a `vmap` rule's `info`: the number of stacked tangents / cotangents"""
    batch_size: int


def _one_state(fam, call, nfixed, tensors):
    """the multi-direction path of the family for ONE state: `tensors` = the fixed tensors, then the directions stacked as
    (ndir, nx, 1, nlev) - the family's rule as its `vmap` over the directions runs it"""
    rule = _ad_rule if fam.adjoint else _tl_rule
    dims = (call._replace(eta=None),) + (None,) * nfixed + (0,) * (len(tensors) - nfixed)
    return tuple(rule(fam, call, tensors, _Directions(tensors[nfixed].shape[0]), dims)[0])


class _MembersDirs(_InnerFunction):
    """(the family's name, call, nfixed, the fixed tensors, present tangents / cotangents stacked as (ndir, nx, 1, nlev)) ->
    the results as (ndir, nx, 1, nlev)"""
    @staticmethod
    def forward(family, call, nfixed, *tensors):
        return _one_state(_FAMILIES[family], call, nfixed, tensors)

    @staticmethod
    def vmap(info, in_dims, family, call, nfixed, *tensors):
        dims = in_dims[3:]
        if in_dims[1].eta is not None:               # (the forward has refused a batched `eta` before any rule gets here)
            raise NotImplementedError(_BATCHED_ETA)
        if not _whole_state(dims[:nfixed]):          # the state is batched further out: this level is a second one of directions
            raise NotImplementedError(_BATCHED_STATE)
        _refuse_nested(tensors)                      # a third batch level
        tensors = _members(info, dims, tensors)      # state (nmem, nx, 1, nlev), directions (nmem, ndir, nx, 1, nlev)
        nmem, ndir = info.batch_size, tensors[nfixed].shape[1]
        fam = _FAMILIES[family]
        adjoint, step = fam.adjoint, fam.names is STEP_IN
        ext = dict(call.ext, AD_TRAJ_FIX=1) if adjoint else call.ext
        one_launch = (not step or bool(ext.get("LPHYLIN"))) and not (adjoint and _evap(ext))
        if not one_launch:      # no kernel: the multi-direction path, member by member
            rows = []
            for m in range(nmem):
                fields = [_as_field(_plain(t)[m]) for t in tensors[:nfixed]] + [_plain(t)[m] for t in tensors[nfixed:]]
                rows.append(_one_state(fam, call._replace(geo=field_geometry(fields[0])), nfixed, fields))
            outs = tuple(torch.stack([r[i] for r in rows]) for i in range(len(rows[0])))
            return outs, (0,) * len(outs)
        state, _, traj, dirs = _unpacked(fam.names, step, adjoint, call._replace(geo=None), tensors)
        if adjoint:             # one launch per `width` cotangents, all members
            adj = _call(fam, True, state, dirs, call.eta, call.dt, ext, call.want, traj=traj, ens=True)
            outs = tuple(adj[n] for n in call.want)
        else:                   # one ensemble launch per direction
            rows = [_call(fam, False, state, {n: f[:, d] for n, f in dirs.items()}, call.eta, call.dt, ext, NL_OUT, ens=True)[1]
                    for d in range(ndir)]
            outs = tuple(torch.stack([r[n] for r in rows], dim=1) for n in NL_OUT)
        return outs, (0,) * len(outs)


class _TLMasked(_InnerFunction):
    """(call, 16 state fields, present tangents) -> the ten perturbed outputs"""
    @staticmethod
    def forward(call, *tensors):
        return _tl_rule(_TL_MASKED, call, tensors)

    @staticmethod
    def vmap(info, in_dims, call, *tensors):
        return _tl_rule(_TL_MASKED, call, tensors, info, in_dims)


class _TLStep(_InnerFunction):
    """(call, 15 state fields, qsat, present tangents) -> the ten perturbed outputs of the step"""
    @staticmethod
    def forward(call, *tensors):
        return _tl_rule(_TL_STEP, call, tensors)

    @staticmethod
    def vmap(info, in_dims, call, *tensors):
        return _tl_rule(_TL_STEP, call, tensors, info, in_dims)


class _SaturationTL(_InnerFunction):
    """(call, ap, t, present tangents of ap / t) -> qsat_i"""
    @staticmethod
    def forward(call, ap, t, *tangents):
        ref = _plain(ap)
        pert = {n: _in_layout(g, ref, call.geo) for n, g in zip(call.have, tangents)}
        return saturation_tl(ap, t, pert.get("ap"), pert.get("t"), call.ext)[1]

    @staticmethod
    def vmap(info, in_dims, call, ap, t, *tangents):
        _refuse_nested((ap, t) + tangents)
        if _batched_state(in_dims, 2):      # an ensemble of states: pointwise, member by member
            one = lambda c, *f: (_SaturationTL.forward(c, *f),)  # noqa: E731
            return _looped_members(one, call, _members(info, in_dims[1:], (ap, t) + tangents), 1)[0], 0
        pert = dict(zip(call.have, _stacked(info, in_dims, (ap, t) + tangents, 2)))
        return _saturation_tl_stacked(ap, t, pert, call.ext, call.geo), 0


def _looped_adjoint(one, info, in_dims, call, tensors, nfixed, nout):
    """the `vmap` rule of the adjoint launches that have no multi-direction kernel (the evaporation switches, the
    non-LPHYLIN step, `saturation`): one single launch per cotangent, results stacked; `one(call, *tensors)` is the
    Function's own `forward`"""
    _refuse_nested(tensors)
    if _batched_state(in_dims, nfixed):     # an ensemble of states: the single launch member by member
        call, members = _ens_members(info, in_dims, call, tensors)
        return _looped_members(one, call, members, nout), (0,) * nout
    cot = _stacked(info, in_dims, tensors, nfixed)
    rows = [one(call, *tensors[:nfixed], *(g[b] for g in cot)) for b in range(info.batch_size)]
    return tuple(torch.stack([r[i] for r in rows]) for i in range(nout)), (0,) * nout


def _ad_rule(fam, call, tensors, info=None, in_dims=None):
    """`forward` and, with `info` and `in_dims`, `vmap` of `_ADMasked` / `_ADStep`.  Where the adjoint is ONE launch of the
    family - the step with LPHYLIN only; with the evaporation switches only under `EVAP_ADJOINT = "trajectory"`, which
    swaps in the evaporation families (`ad_masked_evap` ...), and then for a single state only - batched cotangents take
    its multi-direction launches.  Elsewhere they loop over this rule for one cotangent: the dense `cloudsc2_ad`
    (evaporation, `EVAP_ADJOINT = "dense"`), `ad_masked_evap` or `ad_masked`, for the step producing the adjoint of its
    `qsat`, which `saturation_ad` adds into those of `ap` and `t`.  Ensembles with the evaporation switches loop over their
    members in either mode, unless `EVAP_ENSEMBLE` is set: then, under `"trajectory"`, they are one launch of the evaporation
    family's ensemble entry (`ad_masked_evap_ens` / `ad_step_evap_ens`; the non-LPHYLIN step still loops)."""
    batched, step, want = info is not None, fam is _AD_STEP, call.want
    ext = dict(call.ext, AD_TRAJ_FIX=1)
    if EVAP_ADJOINT not in ("dense", "trajectory"):
        raise ValueError(f"autodiff.EVAP_ADJOINT must be 'dense' or 'trajectory', got {EVAP_ADJOINT!r}")
    evap_traj = _evap(ext) and EVAP_ADJOINT == "trajectory"     # the cover kernels; their ensemble form only on request
    evap_ens = evap_traj and bool(EVAP_ENSEMBLE)
    one_launch = (not _evap(ext) or (evap_traj and (call.geo is not None or evap_ens))) and \
        (not step or bool(ext.get("LPHYLIN")))
    launch = (_AD_STEP_EVAP if step else _AD_MASKED_EVAP) if evap_traj else fam     # the family `_call` runs
    nfixed = len(fam.names) + step + 2
    if batched:
        if ENSEMBLE_JACOBIANS and _nested(tensors[:nfixed]) and not _batched_state(in_dims, nfixed):
            return _members_times_directions(fam, call, tensors, info, in_dims, nfixed)
        _refuse_nested(tensors)
        if one_launch and evap_traj and not evap_ens and _batched_state(in_dims, nfixed):   # an ensemble: member by member
            return _looped_adjoint(lambda c, *t: _ad_rule(fam, c, t), info, in_dims, call, tensors, nfixed, len(want))
        if one_launch and _batched_state(in_dims, nfixed):   # an ensemble of states: one ensemble launch
            call, members = _ens_members(info, in_dims, call, tensors, len(fam.names))
            outs = _ad_rule(fam, call._replace(geo=None), members)
            return outs, (0,) * len(outs)
    if call.geo is None:
        if not one_launch:
            return _looped_members(lambda c, *t: _ad_rule(fam, c, t), call, tensors, len(want))
        state, _, traj, forcing = _unpacked(fam.names, step, True, call, tensors)
        state, shared, _ = _split_shared(state, forcing)
        if shared is not None and launch is not fam:     # the evaporation ensemble launch takes whole members only
            state = {**state, **{n: f.unsqueeze(0).expand(traj["fplsl"].shape[0], *f.shape) for n, f in shared.items()}}
            shared = None
        adj = _call(launch, False, state, forcing, call.eta, call.dt, ext, want, traj=traj, ens=True, shared=shared)
        return tuple(adj[n] for n in want)
    if batched and not one_launch:
        return _looped_adjoint(lambda c, *t: _ad_rule(fam, c, t), info, in_dims, call, tensors, len(fam.names) + step + 2,
                               len(want))
    state, qsat, traj, forcing = _unpacked(fam.names, step, True, call, tensors, info, in_dims)
    if one_launch:
        adj = _call(launch, batched, state, forcing, call.eta, call.dt, ext, want, traj=traj)
    else:
        through = tuple(n for n in ("ap", "t") if step and n in want)    # the adjoints the path through qsat arrives in
        if step:
            state, want = dict(state, qsat=qsat), want + (("qsat",) if through else ())
        if evap_traj:
            adj = ad_masked_evap(state, forcing, call.eta, call.dt, ext, traj=traj, want=want)
        elif _evap(ext):
            adj = _dense_ad(state, forcing, call.eta, call.dt, ext, call.geo, want)
        else:
            adj = ad_masked(state, forcing, call.eta, call.dt, ext, traj=traj, want=want)
        if through:
            saturation_ad(state["ap"], state["t"], adj["qsat"], ext, want=through, into={n: adj[n] for n in through})
    outs = tuple(adj[n] for n in call.want)
    return (outs, (0,) * len(outs)) if batched else outs


class _ADMasked(_InnerFunction):
    """(call, 16 state fields, traj fplsl, traj fplsn, present cotangents) -> the adjoints of `call.want`"""
    @staticmethod
    def forward(call, *tensors):
        return _ad_rule(_AD_MASKED, call, tensors)

    @staticmethod
    def vmap(info, in_dims, call, *tensors):
        return _ad_rule(_AD_MASKED, call, tensors, info, in_dims)


class _ADStep(_InnerFunction):
    """(call, 15 state fields, qsat, traj fplsl, traj fplsn, present cotangents) -> the adjoints of `call.want`"""
    @staticmethod
    def forward(call, *tensors):
        return _ad_rule(_AD_STEP, call, tensors)

    @staticmethod
    def vmap(info, in_dims, call, *tensors):
        return _ad_rule(_AD_STEP, call, tensors, info, in_dims)


class _SaturationAD(_InnerFunction):
    """(call, ap, t, the cotangent of qsat) -> the adjoints of `call.want` (of ap, t)"""
    @staticmethod
    def forward(call, ap, t, grad):
        adj = saturation_ad(ap, t, _in_layout(grad, _plain(ap), call.geo), call.ext, want=call.want)
        return tuple(adj[n] for n in call.want)

    @staticmethod
    def vmap(info, in_dims, call, ap, t, grad):
        return _looped_adjoint(_SaturationAD.forward, info, in_dims, call, (ap, t, grad), 2, len(call.want))


def _ext_of(externals) -> Dict[str, Any]:
    return dict(default_externals() if externals is None else externals)


def _refuse_batched_state(info, in_dims, *args):
    raise NotImplementedError(_BATCHED_STATE)


def _geometry(field):
    """`field_geometry`, or (-1, -1, -1) for a member of a state batched by `vmap` in some other layout: the derivative
    rules then see a batched state and take the ensemble path, which settles the layout itself"""
    try:
        return field_geometry(field)
    except ValueError:
        return (-1, -1, -1)


class _NLFunction(torch.autograd.Function):
    """What `_Cloudsc2` and `_Cloudsc2Step` share: everything but `forward`.  A subclass names its inputs behind (eta, dt,
    externals) in `names`, the inner Functions that launch its `jvp` / `backward` in `tl` / `ad`, and says `with_qsat` if its
    last output is `qsat`: not differentiable, and saved behind the inputs for both modes.  The rules are classmethods -
    torch reaches them through the class in every mode (autograd, forward AD, `torch.func`)."""
    names: Tuple[str, ...] = ()
    tl = ad = None
    with_qsat = False
    ensemble = None      # the Function on member-major batches that `vmap` over the state runs; None: this is one

    @classmethod
    def setup_context(cls, ctx, inputs, outputs):
        eta, dt, externals, *fields = inputs
        qsat = outputs[len(NL_OUT):] if cls.with_qsat else ()
        ctx.set_materialize_grads(False)
        # an ensemble Function has no single geometry: `_Launch.geo` is None and `_call` settles the layout
        ctx.call = _Launch(eta, float(dt), _ext_of(externals), None if cls.ensemble is None else _geometry(fields[0]), ())
        ctx.save_for_backward(*fields, *qsat, outputs[NL_OUT.index("fplsl")], outputs[NL_OUT.index("fplsn")])
        ctx.save_for_forward(*fields, *qsat)
        if qsat:
            ctx.mark_non_differentiable(*qsat)

    @classmethod
    @torch.autograd.function.once_differentiable     # it hands its arguments through: here (cls, ctx, *grads)
    def backward(cls, ctx, *grads):
        grads = grads[:len(NL_OUT)]                      # one behind them belongs to `qsat`
        need = ctx.needs_input_grad[3:]
        if all(g is None for g in grads) or not any(need):
            return (None,) * (3 + len(cls.names))
        have = tuple(n for n, g in zip(NL_OUT, grads) if g is not None)
        want = tuple(n for n, w in zip(cls.names, need) if w)
        adj = dict(zip(want, cls.ad.apply(ctx.call._replace(have=have, want=want), *(f.detach() for f in ctx.saved_tensors),
                                          *(g for g in grads if g is not None))))
        if cls.ensemble is None:      # an ensemble Function: the adjoint of a SHARED input is the sum of the members' adjoints
            for n, f in zip(cls.names, ctx.saved_tensors):
                if n in adj and f.dim() == 3:
                    adj[n] = adj[n].sum(0)
        return (None, None, None) + tuple(adj.get(n) for n in cls.names)

    @classmethod
    def jvp(cls, ctx, _eta_t, _dt_t, _ext_t, *tangents):
        have = tuple(n for n, t in zip(cls.names, tangents) if t is not None)
        if not have:
            return (None,) * (len(NL_OUT) + cls.with_qsat)
        # in jvp, ctx.saved_tensors is what save_for_forward kept: the fields, and `qsat`
        with torch.no_grad():
            out_i = cls.tl.apply(ctx.call._replace(have=have), *(f.detach() for f in ctx.saved_tensors),
                                 *(t for t in tangents if t is not None))
        return tuple(out_i) + (None,) * cls.with_qsat

    @classmethod
    def vmap(cls, info, in_dims, eta, dt, externals, *fields):
        """`vmap` over the WHOLE state (every field batched; a state batched in part is refused): the fields are moved to
        dimension 0 and the ensemble Function runs on the member-major batch - one launch, and differentiable like this one"""
        if in_dims[0] is not None and not SHARED_STATE:
            raise NotImplementedError(_BATCHED_ETA)
        if cls.ensemble is None:
            raise NotImplementedError(_BATCHED_STATE)
        _refuse_nested(fields + (eta,))
        if not SHARED_STATE:
            _whole_state(in_dims[3:])
            members = _members(info, in_dims[3:], fields)
        else:   # the fields at in_dims=None are shared by the members; a batched eta is one level vector per member
            if in_dims[0] is not None:
                eta = eta.movedim(in_dims[0], 0).contiguous()
            dims = list(in_dims[3:])
            if all(d is None for d in dims):    # only eta is batched: one field has to carry the members
                at = cls.names.index("t")
                fields = fields[:at] + (fields[at].unsqueeze(0).expand(info.batch_size, *fields[at].shape),) + fields[at + 1:]
                dims[at] = 0
            members = [f if d is None else f.movedim(d, 0) for f, d in zip(fields, dims)]
        outs = cls.ensemble.apply(eta, dt, externals, *members)
        return outs, (0,) * len(outs)


def _state_fields(what, state, names):
    """the public calls' check of `state` -> its fields in the order of `names`"""
    missing = [n for n in names if n not in state]
    if missing or len(state) != len(names):
        raise ValueError(f"{what}: state must hold exactly the fields {names}; missing {missing}")
    for n in names:
        if isinstance(state[n], torch.Tensor) and not state[n].is_cuda:
            raise ValueError(f"{what}: {n} lives on {state[n].device}; fields must live on the GPU")
    return tuple(state[n] for n in names)


class _Cloudsc2(_NLFunction):
    names, tl, ad = NL_IN, _TLMasked, _ADMasked

    @staticmethod
    def forward(eta, dt, externals, *inputs):
        from .stencils import compile_stencil

        state = {n: _plain(f) for n, f in zip(NL_IN, inputs)}
        (nx, nlev, ls), dtype, device = _checked("cloudsc2", ((state, NL_IN, True),))
        nz = nlev - 1
        ref = state[NL_IN[0]]
        out = {n: _new_like(ref, nx, nz, ls) for n in NL_OUT}
        compile_stencil("cloudsc2_nl", _ext_of(externals))(
            **{"in_" + n: f for n, f in state.items()}, **{"out_" + n: f for n, f in out.items()}, in_eta=eta, dt=dt,
            origin=(0, 0, 0), domain=(nx, 1, nlev), validate_args=False, exec_info=None)
        return tuple(out[n] for n in NL_OUT)


def _dense_ad(state, forcing, eta, dt, ext, geo, want):
    """the evaporation switches: `cloudsc2_ad` with zero fields for the absent forcing; unwanted adjoints are dropped"""
    from .stencils import compile_stencil

    nx, nlev, ls = geo
    ref = _plain(state[NL_IN[0]])
    new = lambda: _new_like(ref, nx, nlev - 1, ls)  # noqa: E731
    args = {"in_" + n: _plain(f) for n, f in state.items()}
    args.update({"in_" + n + "_i": forcing[n] if n in forcing else new() for n in NL_OUT})
    args.update({"out_" + n: new() for n in NL_OUT})
    adj = {n: new() for n in NL_IN}
    args.update({"out_" + n + "_i": f for n, f in adj.items()})
    compile_stencil("cloudsc2_ad", ext)(**args, in_eta=eta, dt=dt, origin=(0, 0, 0), domain=(nx, 1, nlev), validate_args=False,
                                         exec_info=None)
    return {n: adj[n] for n in want}


def cloudsc2(state: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
             externals: Optional[Mapping[str, Any]] = None) -> Dict[str, torch.Tensor]:
    """One differentiable CLOUDSC2 step: the 16 inputs (`NL_IN` names, storage layout `(nx, 1, nz+1)`, column-fastest) ->
    the 10 NL outputs (`NL_OUT` names), computed by `cloudsc2_nl`.

    Derivatives are the reference's tangent-linear model and its exact transpose.  They are the reference's REGULARISED
    TL / AD (LREGCL damps the derivatives of the cloud-fraction and autoconversion terms), not finite differences of the
    NL step: a Taylor test of NL against them converges to the regularised slope.  `AD_TRAJ_FIX=1` is forced for the
    adjoint call, so the VJP is the transpose of the JVP in every column (the reference's own AD differs from it where the
    saturation adjustment crosses the freezing point), and the trajectory fluxes are the NL kernel's own.

    `backward` is ONE masked adjoint launch: forcing = the gradients that arrived, results = the inputs that require one;
    `jvp` is one masked tangent-linear launch.  With LEVAPLS2 / LDRAIN1D the backward falls back to the dense
    `cloudsc2_ad` (which recomputes the trajectory: 70 words per level and column plus ten zero-filled forcing fields and
    26 scratch results) - same gradients, at that cost - unless `autodiff.EVAP_ADJOINT = "trajectory"`, which makes it one
    `ad_masked_evap` launch (one cover field allocated per backward).  Second derivatives are not available (`once_differentiable`)."""
    outs = _Cloudsc2.apply(eta, dt, externals, *_state_fields("cloudsc2", state, NL_IN))
    return dict(zip(NL_OUT, outs))


# ---- the first half of the step, and the step as a whole ------------------------------------------------------------------
def _ptr(f: Optional[torch.Tensor]):
    return None if f is None else f.data_ptr()


def saturation_tl(ap: torch.Tensor, t: torch.Tensor, ap_i: Optional[torch.Tensor] = None, t_i: Optional[torch.Tensor] = None,
                  externals: Optional[Mapping[str, Any]] = None, *, write_qsat: bool = False):
    """Tangent-linear of `saturation` (`cloudsc2_saturation_tl_*`): `qsat_i = g_t t_i + g_ap ap_i` on levels `< nz`; a
    perturbation that is `None` is zero (at least one is given).  Returns `(qsat or None, qsat_i)` as new `storage.zeros`
    fields.  All three forms of `saturation` (LPHYLIN; KFLAG 1 / other)."""
    what = "saturation_tl"
    fields = {"ap": _plain(ap), "t": _plain(t)}
    pert = {n: _plain(f) for n, f in (("ap", ap_i), ("t", t_i)) if f is not None}
    if not pert:
        raise ValueError(f"{what}: ap_i and t_i are both None: there is nothing to propagate")
    (nx, nlev, ls), dtype, device = _checked(what, ((fields, ("ap", "t"), True), (pert, ("ap", "t"), False)))
    nz = nlev - 1
    qsat = _new_like(fields["ap"], nx, nz, ls) if write_qsat else None
    qsat_i = _new_like(fields["ap"], nx, nz, ls)
    p = _params(externals, nz)
    with torch.cuda.device(device):
        rc = getattr(_lib.load(), "cloudsc2_saturation_tl_" + _SFX[dtype])(
            ctypes.byref(p), nx, nz, ls, fields["ap"].data_ptr(), fields["t"].data_ptr(), _ptr(pert.get("ap")),
            _ptr(pert.get("t")), _ptr(qsat), qsat_i.data_ptr(), int(torch.cuda.current_stream(device).cuda_stream))
    _lib.check(rc, what)
    return qsat, qsat_i


def saturation_ad(ap: torch.Tensor, t: torch.Tensor, qsat_adj: torch.Tensor, externals: Optional[Mapping[str, Any]] = None,
                  *, want: Iterable[str] = ("ap", "t"), into: Optional[Mapping[str, torch.Tensor]] = None):
    """Adjoint of `saturation` (`cloudsc2_saturation_ad_*`): `t_adj = g_t qsat_adj`, `ap_adj = g_ap qsat_adj` on levels
    `< nz`, for the names in `want`.  With `into` (a field per wanted name) the products are ADDED to those fields in place
    (`accumulate = 1`) - e.g. to the `t` / `ap` adjoints `ad_masked` has just written, which completes the adjoint of
    `saturation` + `cloudsc2_nl`.  Returns `{name: adjoint}`: new `storage.zeros` fields, or the fields of `into`."""
    what = "saturation_ad"
    want = tuple(want)
    if not want or set(want) - {"ap", "t"}:
        raise ValueError(f"{what}: `want` must name at least one of ('ap', 't'), got {want}")
    fields = {"ap": _plain(ap), "t": _plain(t), "qsat_adj": _plain(qsat_adj)}
    groups = [(fields, ("ap", "t", "qsat_adj"), True)]
    if into is not None:
        if set(into) != set(want):
            raise ValueError(f"{what}: `into` must hold exactly the wanted fields {want}, got {sorted(into)}")
        groups.append(({n: _plain(f) for n, f in into.items()}, ("ap", "t"), False))
    (nx, nlev, ls), dtype, device = _checked(what, groups)
    nz = nlev - 1
    adj = {n: (_new_like(fields["ap"], nx, nz, ls) if into is None else _plain(into[n])) for n in want}
    p = _params(externals, nz)
    with torch.cuda.device(device):
        rc = getattr(_lib.load(), "cloudsc2_saturation_ad_" + _SFX[dtype])(
            ctypes.byref(p), nx, nz, ls, fields["ap"].data_ptr(), fields["t"].data_ptr(), fields["qsat_adj"].data_ptr(),
            _ptr(adj.get("ap")), _ptr(adj.get("t")), 0 if into is None else 1,
            int(torch.cuda.current_stream(device).cuda_stream))
    _lib.check(rc, what)
    return adj


def _run_saturation(ap, t, ext, geo):
    from .stencils import compile_stencil

    nx, nlev, ls = geo
    qsat = _new_like(ap, nx, nlev - 1, ls)
    compile_stencil("saturation", ext)(in_ap=ap, in_t=t, out_qsat=qsat, origin=(0, 0, 0), domain=(nx, 1, nlev - 1),
                                       validate_args=False, exec_info=None)
    return qsat


class _Saturation(torch.autograd.Function):
    @staticmethod
    def forward(externals, ap, t):
        fields = {"ap": _plain(ap), "t": _plain(t)}
        geo, _, _ = _checked("saturation", ((fields, ("ap", "t"), True),))
        return _run_saturation(fields["ap"], fields["t"], _ext_of(externals), geo)

    @staticmethod
    def setup_context(ctx, inputs, output):
        externals, ap, t = inputs
        ctx.set_materialize_grads(False)
        ctx.call = _Launch(None, 0.0, _ext_of(externals), _geometry(ap), ())
        ctx.save_for_backward(ap, t)
        ctx.save_for_forward(ap, t)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        want = tuple(n for n, w in zip(("ap", "t"), ctx.needs_input_grad[1:]) if w)
        if grad is None or not want:
            return None, None, None
        ap, t = ctx.saved_tensors
        adj = dict(zip(want, _SaturationAD.apply(ctx.call._replace(want=want), ap.detach(), t.detach(), grad)))
        return None, adj.get("ap"), adj.get("t")

    @staticmethod
    def jvp(ctx, _ext_t, ap_i, t_i):
        have = tuple(n for n, g in (("ap", ap_i), ("t", t_i)) if g is not None)
        if not have:
            return None
        ap, t = ctx.saved_tensors
        with torch.no_grad():
            return _SaturationTL.apply(ctx.call._replace(have=have), ap.detach(), t.detach(),
                                       *(g for g in (ap_i, t_i) if g is not None))

    @staticmethod
    def vmap(info, in_dims, externals, ap, t):
        """`vmap` over the state: `saturation` is pointwise - it loops over the members (differentiably) and stacks"""
        _refuse_nested((ap, t))
        _whole_state(in_dims[1:])
        ap, t = _members(info, in_dims[1:], (ap, t))
        return torch.stack([_Saturation.apply(externals, _as_field(ap[m]), _as_field(t[m]))
                            for m in range(info.batch_size)]), 0


def saturation(ap: torch.Tensor, t: torch.Tensor, externals: Optional[Mapping[str, Any]] = None) -> torch.Tensor:
    """Differentiable `saturation`: `qsat` of `ap` and `t` on levels `< nz` (level `nz` stays 0), computed by the
    `saturation` stencil, all three forms (LPHYLIN; KFLAG 1 / other).  `backward` is ONE `saturation_ad` launch, `jvp` one
    `saturation_tl` launch.  The derivative is the exact one of the formula, with every `min` / `max` taken on the branch
    the value took (a clamped branch - `alfa` outside (RTICE, RTWAT), `qs` clipped at QMAX - has derivative 0)."""
    for n, f in (("ap", ap), ("t", t)):
        if isinstance(f, torch.Tensor) and not f.is_cuda:
            raise ValueError(f"saturation: {n} lives on {f.device}; fields must live on the GPU")
    return _Saturation.apply(externals, ap, t)


def _evap(ext) -> bool:
    return bool(ext.get("LEVAPLS2") or ext.get("LDRAIN1D"))


class _Cloudsc2Step(_NLFunction):
    names, tl, ad, with_qsat = STEP_IN, _TLStep, _ADStep, True

    @staticmethod
    def forward(eta, dt, externals, *inputs):
        from .stencils import compile_stencil

        state = {n: _plain(f) for n, f in zip(STEP_IN, inputs)}
        (nx, nlev, ls), dtype, device = _checked("cloudsc2_step", ((state, STEP_IN, True),))
        nz = nlev - 1
        ref = state[STEP_IN[0]]
        out = {n: _new_like(ref, nx, nz, ls) for n in NL_OUT}
        ext = _ext_of(externals)
        call = dict(in_eta=eta, dt=dt, origin=(0, 0, 0), domain=(nx, 1, nlev), validate_args=False, exec_info=None)
        ins, outs = {"in_" + n: f for n, f in state.items()}, {"out_" + n: f for n, f in out.items()}
        if ext.get("LPHYLIN"):
            qsat = _new_like(ref, nx, nz, ls)
            compile_stencil("cloudsc2_nl_saturation", ext)(**ins, out_qsat=qsat, **outs, **call)
        else:
            qsat = _run_saturation(state["ap"], state["t"], ext, (nx, nlev, ls))
            compile_stencil("cloudsc2_nl", ext)(**ins, in_qsat=qsat, **outs, **call)
        return tuple(out[n] for n in NL_OUT) + (qsat,)


def cloudsc2_step(state: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                  externals: Optional[Mapping[str, Any]] = None) -> Dict[str, torch.Tensor]:
    """One differentiable step as the drivers run it, `saturation` + `cloudsc2_nl`: the 15 inputs (`STEP_IN` names = `NL_IN`
    without `qsat`) -> the 10 NL outputs (`NL_OUT` names) plus `"qsat"`, the saturation field the step formed.

    Gradients are TOTAL derivatives: the path t, ap -> qsat -> cloudsc2, which `cloudsc2` on a precomputed `qsat` leaves
    out, is part of them.  They are the reference's regularised TL / AD of `cloudsc2` (see `cloudsc2`: LREGCL damping,
    `AD_TRAJ_FIX=1` forced for the adjoint, trajectory fluxes the NL kernel's own) chained with the EXACT derivative of
    `saturation`, in which every `min` / `max` is differentiated on the branch the value took (`alfa` clamped outside
    (RTICE, RTWAT) and `qs` clipped at QMAX contribute 0).  The reference has no TL / AD of `saturation`.

    `"qsat"` is returned for inspection and is not differentiable; who needs gradients through it composes `saturation`
    with `cloudsc2`.  Forward, LPHYLIN: one launch (`cloudsc2_nl_saturation`), otherwise `saturation` then `cloudsc2_nl`.
    `backward` with LPHYLIN and without LEVAPLS2 / LDRAIN1D is ONE `cloudsc2_ad_step` launch (with the switches and
    `EVAP_ADJOINT = "trajectory"`: one `cloudsc2_ad_evap_step` launch); otherwise `ad_masked` (or the dense `cloudsc2_ad`
    for the evaporation switches, or `ad_masked_evap` under `"trajectory"`) producing the `qsat` adjoint, then `saturation_ad` adding into the
    `t` / `ap` adjoints.  `jvp` is one `cloudsc2_tl_step` launch, or `saturation_tl` then `tl_masked`."""
    if "qsat" in state:
        raise ValueError("cloudsc2_step: `state` holds `qsat`, which the step forms itself from `ap` and `t`; for a qsat of "
                         "your own use `cloudsc2` (compose it with `saturation` for the total derivative)")
    outs = _Cloudsc2Step.apply(eta, dt, externals, *_state_fields("cloudsc2_step", state, STEP_IN))
    return dict(zip(NL_OUT + ("qsat",), outs))


# ---- ensembles: member-major batches of states, one launch per call --------------------------------------------------------
class _TLMaskedEns(_InnerFunction):
    """(call, 16 member-major state fields, present tangents) -> the ten perturbed outputs, member-major"""
    @staticmethod
    def forward(call, *tensors):
        return _tl_rule(_TL_MASKED, call._replace(geo=None), tensors)

    vmap = staticmethod(_refuse_batched_state)


class _TLStepEns(_InnerFunction):
    @staticmethod
    def forward(call, *tensors):
        return _tl_rule(_TL_STEP, call._replace(geo=None), tensors)

    vmap = staticmethod(_refuse_batched_state)


class _ADMaskedEns(_InnerFunction):
    """(call, 16 member-major state fields, traj fplsl, traj fplsn, present cotangents) -> the adjoints of `call.want`"""
    @staticmethod
    def forward(call, *tensors):
        return _ad_rule(_AD_MASKED, call._replace(geo=None), tensors)

    vmap = staticmethod(_refuse_batched_state)


class _ADStepEns(_InnerFunction):
    @staticmethod
    def forward(call, *tensors):
        return _ad_rule(_AD_STEP, call._replace(geo=None), tensors)

    vmap = staticmethod(_refuse_batched_state)


def _nl_ens(what, single, names, inputs, eta, dt, externals):
    """forward of the ensemble Functions: ONE `cloudsc2_nl_ens_*` launch (`names` = NL_IN) or one `cloudsc2_nl_fused_ens_*`
    launch (`names` = STEP_IN: `saturation` fused in, `qsat` returned behind the ten outputs).  The non-LPHYLIN step has no
    fused kernel: it loops over the members through `single`, the forward of the single Function.
    An input that is a plain `(nx, 1, nlev)` field is SHARED by the members, and `eta` may be `(nmem, nz+1)`: the launch is
    then `cloudsc2_nl_enss_*` / `cloudsc2_nl_fused_enss_*`, and nothing is copied per member."""
    ext, step = _ext_of(externals), names is STEP_IN
    shared = {n: f for n, f in zip(names, inputs) if isinstance(f, torch.Tensor) and f.dim() == 3}
    batched = {n: f for n, f in zip(names, inputs) if n not in shared}
    if not batched:
        raise ValueError(f"{what}: every state field is shared: at least one must be member-major (nmem, nx, 1, nz+1)")
    if step and not ext.get("LPHYLIN"):
        rows = [single(eta[m] if isinstance(eta, torch.Tensor) and eta.dim() == 2 else eta, dt, externals,
                       *(_as_field(_plain(f) if n in shared else _plain(f)[m]) for n, f in zip(names, inputs)))
                for m in range(next(iter(batched.values())).shape[0])]
        return tuple(torch.stack([r[i] for r in rows]) for i in range(len(rows[0])))
    first = _plain(next(iter(batched.values())))
    nmem, geo, ms = _ens_geometry(what, first)
    nx, nlev, ls = geo
    for n, f in batched.items():
        if not isinstance(f, torch.Tensor) or tuple(f.shape) != (nmem, nx, 1, nlev):
            raise ValueError(f"{what}: {n} must be a tensor of shape {(nmem, nx, 1, nlev)} like {names[0]}, got "
                             f"{tuple(getattr(f, 'shape', ()))}")
    fields = {n: _batched_layout(f, first, geo, ms) for n, f in batched.items()}
    member0 = {n: f[0] for n, f in fields.items()}
    member0.update(_shared_fields(what, shared, first, geo))
    _, dtype, device = _checked(what, ((member0, names, True),))
    enss = bool(shared) or (isinstance(eta, torch.Tensor) and eta.dim() == 2)
    eta, eta_ms = _eta_members(what, eta, nlev - 1, nmem, dtype, device)
    new = lambda: _zeros_members(nmem, geo, dtype, device, ms)  # noqa: E731
    out = {n: new() for n in NL_OUT}
    qsat = (new(),) if step else ()
    p = _params(ext, nlev - 1)
    head = (ctypes.byref(p), nx, nlev - 1, ls, _ptrs(member0, NL_IN))
    tail = (eta.data_ptr(), _ptrs({n: f[0] for n, f in out.items()}, NL_OUT), float(dt),
            int(torch.cuda.current_stream(device).cuda_stream), nmem, ms)
    if enss:
        tail += (sum(1 << NL_IN.index(n) for n in shared) | _block_order_bits(), eta_ms)
    ens = "enss_" if enss else "ens_"
    with torch.cuda.device(device):
        if step:
            rc = getattr(_lib.load(), "cloudsc2_nl_fused_" + ens + _SFX[dtype])(*head, None, 0.0, qsat[0][0].data_ptr(), *tail)
        else:
            rc = getattr(_lib.load(), "cloudsc2_nl_" + ens + _SFX[dtype])(*head, *tail)
    _lib.check(rc, what)
    return tuple(out[n] for n in NL_OUT) + qsat


class _Cloudsc2Ens(_NLFunction):
    names, tl, ad = NL_IN, _TLMaskedEns, _ADMaskedEns

    @staticmethod
    def forward(eta, dt, externals, *inputs):
        return _nl_ens("cloudsc2_ensemble", _Cloudsc2.forward, NL_IN, inputs, eta, dt, externals)


class _Cloudsc2StepEns(_NLFunction):
    names, tl, ad, with_qsat = STEP_IN, _TLStepEns, _ADStepEns, True

    @staticmethod
    def forward(eta, dt, externals, *inputs):
        return _nl_ens("cloudsc2_step_ensemble", _Cloudsc2Step.forward, STEP_IN, inputs, eta, dt, externals)


_Cloudsc2.ensemble, _Cloudsc2Step.ensemble = _Cloudsc2Ens, _Cloudsc2StepEns


def _expanded_as_shared(states, shared):
    """`SHARED_STATE`: a field of `states` that is an `expand` over the members (stride 0 over dimension 0) whose member 0 is a
    column-fastest field moves to `shared` as that member - as long as another field keeps the members.  Differentiable:
    autograd sums the members' gradients through the `expand`."""
    if not SHARED_STATE:
        return states, shared
    found = {n: f[0] for n, f in states.items() if isinstance(f, torch.Tensor) and f.dim() == 4 and f.shape[0] > 1
             and f.stride(0) == 0 and _geometry(f[0])[0] >= 0}
    if not found or len(found) == len(states):
        return states, shared
    return {n: f for n, f in states.items() if n not in found}, {**(shared or {}), **found}


def _with_shared(what, states, shared, names):
    """`states` and `shared` of the public ensemble calls as one mapping (a shared field stays a plain (nx, 1, nz+1) field)"""
    states, shared = _expanded_as_shared(states, shared)
    if shared is None:
        return states
    _shared_entry(what, names, states, shared, None)
    for n, f in shared.items():
        if not isinstance(f, torch.Tensor) or f.dim() != 3:
            raise ValueError(f"{what}: shared field {n} must be a plain (nx, 1, nz+1) field, got "
                             f"{tuple(getattr(f, 'shape', ()))}")
    return {**states, **shared}


def cloudsc2_ensemble(states: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                      externals: Optional[Mapping[str, Any]] = None, *,
                      shared: Optional[Mapping[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """`cloudsc2` for an ENSEMBLE of `nmem` states: the 16 inputs as member-major `(nmem, nx, 1, nz+1)` tensors (the layout
    of `storage.zeros_batched` and of `torch.stack`; anything else is copied into it) -> the 10 NL outputs, member-major;
    `eta`, `dt` and the externals are shared.  Every member is an independent `cloudsc2` call with `cloudsc2`'s contract
    (`AD_TRAJ_FIX=1` forced for the adjoint, `once_differentiable`).  Forward is ONE `cloudsc2_nl_ens` launch, `backward` one
    `cloudsc2_ad_ens` launch, `jvp` one `cloudsc2_tl_ens` launch; with LEVAPLS2 / LDRAIN1D the backward loops over the
    members through the dense `cloudsc2_ad`.  `torch.func.vmap` of `cloudsc2` over the state runs this Function.

    `shared` maps state names to plain `(nx, 1, nz+1)` fields that all members read; a name is in exactly one of `states` and
    `shared`.  `eta` may be `(nmem, nz+1)`, one level vector per member.  Either runs the shared-state launches
    (`cloudsc2_nl_enss`, `cloudsc2_ad_enss`, `cloudsc2_tl_enss`): no field is copied per member, and the gradient with respect
    to a shared input is the sum over the members of the per-member adjoints - one launch and one `sum(0)`.  With LEVAPLS2 /
    LDRAIN1D the backward keeps its paths of whole members (shared fields are expanded, or the members looped)."""
    states = _with_shared("cloudsc2_ensemble", states, shared, NL_IN)
    outs = _Cloudsc2Ens.apply(eta, dt, externals, *_state_fields("cloudsc2_ensemble", states, NL_IN))
    return dict(zip(NL_OUT, outs))


def cloudsc2_step_ensemble(states: Mapping[str, torch.Tensor], eta: torch.Tensor, dt: float,
                           externals: Optional[Mapping[str, Any]] = None, *,
                           shared: Optional[Mapping[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """`cloudsc2_step` for an ensemble of states (`STEP_IN` names, member-major; see `cloudsc2_ensemble`) -> the 10 NL
    outputs plus `"qsat"`, which is not differentiable.  With LPHYLIN and without LEVAPLS2 / LDRAIN1D every call is one
    launch: `cloudsc2_nl_fused_ens`, `cloudsc2_ad_step_ens`, `cloudsc2_tl_step_ens`.  Otherwise the part that has no
    ensemble kernel loops over the members through the paths of `cloudsc2_step`.  `shared` and a per-member `eta` as in
    `cloudsc2_ensemble` (`cloudsc2_nl_fused_enss`, `cloudsc2_ad_step_enss`, `cloudsc2_tl_step_enss`)."""
    if "qsat" in states or (shared is not None and "qsat" in shared):
        raise ValueError("cloudsc2_step_ensemble: `states` holds `qsat`, which the step forms itself from `ap` and `t`")
    states = _with_shared("cloudsc2_step_ensemble", states, shared, STEP_IN)
    outs = _Cloudsc2StepEns.apply(eta, dt, externals, *_state_fields("cloudsc2_step_ensemble", states, STEP_IN))
    return dict(zip(NL_OUT + ("qsat",), outs))
