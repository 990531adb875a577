"""Physics components of the MI355X build - the host-side mirror of the reference's component classes,
for use where the reference checkout is not available (the GPU box) and as the in-repo API:

  EtaLevels        /root/reference/src/cloudsc2_gt4py/physics/common/diagnostics.py:28-45
  Saturation       .../physics/common/saturation.py:33-76
  StateIncrement   .../physics/common/increment.py:32-132
  PerturbedState   .../physics/common/increment.py:135-261
  Cloudsc2NL       .../physics/nonlinear/microphysics.py:43-172
  Cloudsc2TL       .../physics/tangent_linear/microphysics.py:46-242
  Cloudsc2AD       .../physics/adjoint/microphysics.py:46-238

Same class names, constructor arguments, state / tendency / diagnostic field names, units and call
protocol (`component(state, timestep, out_tendencies=..., out_diagnostics=...)`).  Every component is ONE field map
(`_FIELD_MAP`): the property dicts and the keyword arguments of the stencil call are generated from it, and a build
extension states only its difference from the component it extends.  Parameter groups may be the reference's pydantic
models or plain mappings (anything with `.dict()` or `.items()`).
"""
from __future__ import annotations

from datetime import timedelta
from functools import cached_property
from typing import Any, Dict, NamedTuple, Optional, Sequence, Tuple

from .framework.components import DiagnosticComponent, ImplicitTendencyComponent
from .framework.grid import I, J, K
from .stencils import INC, NL_IN, NL_OUT

_UNITS = {
    "ap": "Pa", "aph": "Pa", "lu": "g g^-1", "lude": "kg m^-3 s^-1", "mfd": "kg m^-2 s^-1", "mfu": "kg m^-2 s^-1",
    "q": "g g^-1", "qi": "g g^-1", "ql": "g g^-1", "qsat": "g g^-1", "supsat": "g g^-1", "t": "K",
    "tnd_cml_q": "g g^-1 s^-1", "tnd_cml_qi": "g g^-1 s^-1", "tnd_cml_ql": "g g^-1 s^-1", "tnd_cml_t": "K s^-1",
    "clc": "", "covptot": "", "fhpsl": "J m^-2 s^-1", "fhpsn": "J m^-2 s^-1", "fplsl": "kg m^-2 s^-1",
    "fplsn": "kg m^-2 s^-1", "tnd_q": "g g^-1 s^-1", "tnd_qi": "g g^-1 s^-1", "tnd_ql": "g g^-1 s^-1",
    "tnd_t": "K s^-1",
}
_HALF = {"aph", "fhpsl", "fhpsn", "fplsl", "fplsn"}
_DIAG_OUT = ("clc", "covptot", "fhpsl", "fhpsn", "fplsl", "fplsn")      # NL outputs kept as diagnostics
_TEND_OUT = ("tnd_q", "tnd_qi", "tnd_ql", "tnd_t")                       # NL outputs kept as tendencies


def _prop(stencil_name: Optional[str]) -> Dict[str, Any]:
    if stencil_name is None:                      # the eta level vector
        return {"grid_dims": (K,), "units": ""}
    kdim = K - 1 / 2 if stencil_name in _HALF else K
    return {"grid_dims": (I, J, kdim), "units": _UNITS[stencil_name]}


def _as_dict(group: Any) -> Dict[str, Any]:
    if group is None:
        return {}
    if hasattr(group, "dict"):
        return dict(group.dict())
    return dict(group)


def _externals(*groups: Any, **literals: Any) -> Dict[str, Any]:
    ext: Dict[str, Any] = {}
    for g in groups:
        ext.update(_as_dict(g))
    ext.update(literals)
    return ext


def _microphysics_externals(lphylin: bool, ldrain1d: bool, *groups: Any, **more: Any) -> Dict[str, Any]:
    """externals of the cloudsc2_* stencils (nonlinear/microphysics.py:64-78 and its TL / AD counterparts)"""
    return _externals(*groups, ICALL=0, LPHYLIN=lphylin, LDRAIN1D=ldrain1d, ZEPS1=1e-12, ZEPS2=1e-10, ZQMAX=0.5, ZSCAL=0.9,
                      **more)


def _tend_name(stencil_name: str) -> str:
    """NL tendency outputs are published as f_q / f_qi / f_ql / f_t (nonlinear/microphysics.py:103-108)."""
    return "f_" + stencil_name[len("tnd_"):]


class _Row(NamedTuple):
    name: str                 # key in the state / output dict
    where: str                # the dict it lives in: "state", "tend" or "diag"
    keyword: Optional[str]    # stencil keyword (None: published, but not an argument of the stencil)
    field: Optional[str]      # stencil field name that gives units and half-level-ness (None: the eta vector)


def _state(base: Sequence[str], sfx: str = "") -> Tuple[_Row, ...]:
    return tuple(_Row(f"f_{n}{sfx}", "state", f"in_{n}{sfx}", n) for n in base)


def _diags(base: Sequence[str], sfx: str = "") -> Tuple[_Row, ...]:
    return tuple(_Row(f"f_{n}{sfx}", "diag", f"out_{n}{sfx}", n) for n in base)


def _nl_outputs(*sfxs: str) -> Tuple[_Row, ...]:
    """the ten NL outputs: six diagnostics, four tendencies - per field, once per suffix ("" and "_i" for TL)"""
    return (tuple(r for n in _DIAG_OUT for sfx in sfxs for r in _diags((n,), sfx))
            + tuple(_Row(_tend_name(n) + sfx, "tend", f"out_{n}{sfx}", n) for n in _TEND_OUT for sfx in sfxs))


_ETA = (_Row("f_eta", "state", "in_eta", None),)


class _FieldMapped:
    """property dicts and stencil keywords of a component, from its `_FIELD_MAP`"""

    _FIELD_MAP: Tuple[_Row, ...] = ()

    def _props(self, where: str) -> Dict[str, Dict[str, Any]]:
        return {r.name: _prop(r.field) for r in self._FIELD_MAP if r.where == where}

    @cached_property
    def input_grid_properties(self):
        return self._props("state")

    @cached_property
    def diagnostic_grid_properties(self):
        return self._props("diag")

    def _call_stencil(self, stencil, nlev_offset: int, dicts: Dict[str, Any], **scalars: Any) -> None:
        g, cfg = self.computational_grid, self.gt4py_config
        kw = {r.keyword: dicts[r.where][r.name] for r in self._FIELD_MAP if r.keyword}
        stencil(**kw, **scalars, domain=(g.nx, 1, g.nz + nlev_offset), origin=(0, 0, 0),
                validate_args=cfg.validate_args, exec_info=cfg.exec_info)


# ---------------------------------------------------------------------------------- small components
class EtaLevels(_FieldMapped, DiagnosticComponent):
    """eta[k] = ap[column 0, k] / aph[column 0, nz] - one device slice operation instead of the
    reference's nz-step Python loop (diagnostics.py:42-45)."""

    _FIELD_MAP = (_Row("f_ap", "state", None, "ap"), _Row("f_aph", "state", None, "aph"), _Row("f_eta", "diag", None, None))

    def array_call(self, state, out) -> None:
        nz = self.computational_grid.nz
        out["f_eta"][:nz] = state["f_ap"][0, 0, :nz] / state["f_aph"][0, 0, nz]


class Saturation(_FieldMapped, DiagnosticComponent):
    _FIELD_MAP = _state(("ap", "t")) + _diags(("qsat",))

    def __init__(self, computational_grid, kflag: int, lphylin: bool, yoethf_params, yomcst_params, *,
                 enable_checks: bool = True, gt4py_config) -> None:
        super().__init__(computational_grid, enable_checks=enable_checks, gt4py_config=gt4py_config)
        ext = _externals(yoethf_params, yomcst_params, KFLAG=kflag, LPHYLIN=lphylin, QMAX=0.5)
        self.saturation = self.compile_stencil("saturation", ext)

    def array_call(self, state, out) -> None:
        self._call_stencil(self.saturation, 0, {"state": state, "diag": out})


class StateIncrement(_FieldMapped, DiagnosticComponent):
    _FIELD_MAP = _state(INC) + _diags(INC, "_i")

    def __init__(self, computational_grid, factor: float, ignore_supsat: bool = False, *,
                 enable_checks: bool = True, gt4py_config) -> None:
        super().__init__(computational_grid, enable_checks=enable_checks, gt4py_config=gt4py_config)
        self.f = gt4py_config.dtypes.float(factor)
        self.increment = self.compile_stencil("state_increment", {"IGNORE_SUPSAT": ignore_supsat})

    def array_call(self, state, out) -> None:
        self._call_stencil(self.increment, 1, {"state": state, "diag": out}, f=self.f)


class PerturbedState(_FieldMapped, DiagnosticComponent):
    _FIELD_MAP = _state(INC) + _state(INC, "_i") + _diags(INC)

    def __init__(self, computational_grid, factor: float, *, enable_checks: bool = True, gt4py_config) -> None:
        super().__init__(computational_grid, enable_checks=enable_checks, gt4py_config=gt4py_config)
        self.f = gt4py_config.dtypes.float(factor)
        self.perturbed_state = self.compile_stencil("perturbed_state", {})

    def array_call(self, state, out) -> None:
        self._call_stencil(self.perturbed_state, 1, {"state": state, "diag": out}, f=self.f)


# ---------------------------------------------------------------------------------- microphysics
class _Microphysics(_FieldMapped, ImplicitTendencyComponent):
    """the call every cloudsc2_* component makes: its field map, `dt`, and `f` where the component carries a factor"""

    f: Optional[Any] = None
    _stencil_name = ""
    _more_externals: Dict[str, Any] = {}       # what a build extension adds to the externals of the component it extends

    @cached_property
    def tendency_grid_properties(self):
        return self._props("tend")

    def _compile(self, lphylin: bool, ldrain1d: bool, *groups: Any, **more: Any) -> None:
        ext = _microphysics_externals(lphylin, ldrain1d, *groups, **more, **self._more_externals)
        self.cloudsc2 = self.compile_stencil(self._stencil_name, ext)

    def array_call(self, state, timestep: timedelta, out_tendencies, out_diagnostics, overwrite_tendencies) -> None:
        scalars = {"dt": self.gt4py_config.dtypes.float(timestep.total_seconds())}
        if self.f is not None:
            scalars["f"] = self.f
        self._call_stencil(self.cloudsc2, 1, {"state": state, "tend": out_tendencies, "diag": out_diagnostics}, **scalars)


class Cloudsc2NL(_Microphysics):
    _FIELD_MAP = _state(NL_IN) + _ETA + _nl_outputs("")
    _stencil_name = "cloudsc2_nl"

    def __init__(self, computational_grid, lphylin: bool, ldrain1d: bool, yoethf_params, yomcst_params,
                 yrecldp_params, yrephli_params, yrphnc_params, *, enable_checks: bool = True, gt4py_config) -> None:
        super().__init__(computational_grid, enable_checks=enable_checks, gt4py_config=gt4py_config)
        self._compile(lphylin, ldrain1d, yoethf_params, yomcst_params, yrecldp_params, yrephli_params, yrphnc_params)


class Cloudsc2NLSaturation(Cloudsc2NL):
    """BUILD EXTENSION: `Saturation` + `Cloudsc2NL` as ONE kernel launch (stencil `cloudsc2_nl_saturation`).
    Same inputs as `Cloudsc2NL` minus `f_qsat`, which becomes an additional diagnostic output; the result is
    bit-identical to calling the two components in sequence (tests/test_hip_nl.py)."""

    _FIELD_MAP = tuple(r for r in Cloudsc2NL._FIELD_MAP if r.name != "f_qsat") + _diags(("qsat",))
    _stencil_name = "cloudsc2_nl_saturation"
    _more_externals = {"KFLAG": 1, "QMAX": 0.5}


class Cloudsc2NLPerturbed(Cloudsc2NL):
    """BUILD EXTENSION: `PerturbedState(factor)` + `Cloudsc2NL` as ONE kernel launch (stencil
    `cloudsc2_nl_perturbed`): the state fields are read as x + factor * x_i on the fly."""

    _FIELD_MAP = Cloudsc2NL._FIELD_MAP + _state(NL_IN, "_i")
    _stencil_name = "cloudsc2_nl_perturbed"

    def __init__(self, computational_grid, factor: float, lphylin: bool, ldrain1d: bool, yoethf_params, yomcst_params,
                 yrecldp_params, yrephli_params, yrphnc_params, *, enable_checks: bool = True, gt4py_config) -> None:
        self.f = gt4py_config.dtypes.float(factor)
        super().__init__(computational_grid, lphylin, ldrain1d, yoethf_params, yomcst_params, yrecldp_params,
                         yrephli_params, yrphnc_params, enable_checks=enable_checks, gt4py_config=gt4py_config)


class Cloudsc2TL(_Microphysics):
    _FIELD_MAP = _state(NL_IN) + _state(NL_IN, "_i") + _ETA + _nl_outputs("", "_i")
    _stencil_name = "cloudsc2_tl"

    def __init__(self, computational_grid, lphylin: bool, ldrain1d: bool, yoethf_params, yomcst_params,
                 yrecldp_params, yrephli_params, yrncl_params, yrphnc_params, *, enable_checks: bool = True,
                 gt4py_config) -> None:
        super().__init__(computational_grid, enable_checks=enable_checks, gt4py_config=gt4py_config)
        self._compile(lphylin, ldrain1d, yoethf_params, yomcst_params, yrecldp_params, yrephli_params, yrncl_params,
                      yrphnc_params, NLEV=computational_grid.nz)


class Cloudsc2TLIncremented(Cloudsc2TL):
    """BUILD EXTENSION: `StateIncrement(factor, ignore_supsat)` + `Cloudsc2TL` as ONE launch (stencil
    `cloudsc2_tl_incremented`): the state needs no `f_*_i` fields, the perturbations are factor * state, formed in the
    kernel.  Outputs are those of the two components called one after the other (up to the compiler's fma contraction of
    the shared level function: ulps)."""

    _FIELD_MAP = tuple(r for r in Cloudsc2TL._FIELD_MAP if r not in _state(NL_IN, "_i"))
    _stencil_name = "cloudsc2_tl_incremented"

    def __init__(self, computational_grid, factor: float, ignore_supsat: bool, lphylin: bool, ldrain1d: bool,
                 yoethf_params, yomcst_params, yrecldp_params, yrephli_params, yrncl_params, yrphnc_params, *,
                 enable_checks: bool = True, gt4py_config) -> None:
        self.f = gt4py_config.dtypes.float(factor)
        self._more_externals = {"IGNORE_SUPSAT": ignore_supsat}
        super().__init__(computational_grid, lphylin, ldrain1d, yoethf_params, yomcst_params, yrecldp_params,
                         yrephli_params, yrncl_params, yrphnc_params, enable_checks=enable_checks, gt4py_config=gt4py_config)


class Cloudsc2AD(_Microphysics):
    """State in: the 16 trajectory fields + the adjoint forcings `f_{clc,...}_i`, `f_tnd_{t,q,ql,qi}_i`
    (adjoint/microphysics.py:91-121).  Out: NL tendencies/diagnostics + `f_cml_{t,q,ql,qi}_i` (tendency
    dict) and the 12 adjoint state fields (diagnostic dict), :123-157."""

    _ADJ_STATE = ("ap", "aph", "lu", "lude", "mfd", "mfu", "q", "qi", "ql", "qsat", "supsat", "t")
    _FIELD_MAP = (_state(NL_IN) + _state(NL_OUT, "_i") + _ETA + _nl_outputs("") + _diags(_ADJ_STATE, "_i")
                  + tuple(_Row(f"f_cml_{n}_i", "tend", f"out_tnd_cml_{n}_i", "tnd_" + n) for n in ("q", "qi", "ql", "t")))
    _stencil_name = "cloudsc2_ad"

    def __init__(self, computational_grid, lphylin: bool, ldrain1d: bool, yoethf_params, yomcst_params,
                 yrecldp_params, yrephli_params, yrncl_params, yrphnc_params, *, enable_checks: bool = True,
                 gt4py_config, ad_traj_fix: bool = False) -> None:
        super().__init__(computational_grid, enable_checks=enable_checks, gt4py_config=gt4py_config)
        self._compile(lphylin, ldrain1d, yoethf_params, yomcst_params, yrecldp_params, yrephli_params, yrncl_params,
                      yrphnc_params, NLEV=computational_grid.nz, AD_TRAJ_FIX=int(ad_traj_fix))


class Cloudsc2ADFromTrajectory(Cloudsc2AD):
    """BUILD EXTENSION: `Cloudsc2AD` called right after `Cloudsc2TL` on the same state - the symmetry test's sequence
    (adjoint/validation.py:135-151) - without the forward sweep that recomputes the NL trajectory (stencil
    `cloudsc2_ad_from_trajectory`).  The state must carry the TL call's NL flux outputs `f_fplsl` / `f_fplsn` (the harness
    puts the TL diagnostics into the state anyway, :149-150).  Only the adjoint fields are written; the NL tendencies /
    diagnostics of the output dicts are NOT (they are the TL call's).  Driver switches only.  The adjoints are Cloudsc2AD's to
    rounding only with `ad_traj_fix=True` or where no column's saturation adjustment crosses RTT: without the fix (quirk
    Q4) the TL fluxes differ from the ones Cloudsc2AD recomputes in such columns."""

    _FIELD_MAP = (tuple(r._replace(keyword=None) if r in _nl_outputs("") else r for r in Cloudsc2AD._FIELD_MAP)
                  + tuple(_Row(f"f_{n}", "state", f"traj_{n}", n) for n in ("fplsl", "fplsn")))
    _stencil_name = "cloudsc2_ad_from_trajectory"


# ---------------------------------------------------------------------------------- the NL field map, for the harness
def nl_input_keywords(state, increments: bool = False) -> Dict[str, Any]:
    """the `in_*` (with `increments`: and `in_*_i`) and `in_eta` keywords of an NL stencil, from a state of DataArrays"""
    rows = (Cloudsc2NLPerturbed if increments else Cloudsc2NL)._FIELD_MAP
    return {r.keyword: state[r.name].data for r in rows if r.where == "state"}


def nl_output_keywords(prefix: str, tends, diags) -> Dict[str, Any]:
    """the ten outputs of a `Cloudsc2NL` call under the keywords `<prefix><NL_OUT name>` (e.g. `ref_tnd_t` = tends["f_t"])"""
    dicts = {"tend": tends, "diag": diags}
    return {prefix + r.field: dicts[r.where][r.name].data for r in Cloudsc2NL._FIELD_MAP if r.where != "state"}


def nl_output_position(name: str, tendency: bool) -> int:
    """position in NL_OUT of the output `Cloudsc2NL` publishes as `name` in its tendency / diagnostic dict"""
    where = "tend" if tendency else "diag"
    return NL_OUT.index(next(r.field for r in Cloudsc2NL._FIELD_MAP if r.where == where and r.name == name))
