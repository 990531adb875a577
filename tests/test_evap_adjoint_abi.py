"""The `cloudsc2_ad_evap_*` entries of the C ABI called with dummy pointers: every refusal is settled on the host, before
anything is launched, with the argument's name in `cloudsc2_last_error()`.  The entries that were there keep refusing the
evaporation switches."""
import ctypes

import pytest

from abi_calls import FIELD, LS, NZ, Call, call  # noqa: F401  (`call` is a fixture)

P = Call.P
SINGLE = ("cloudsc2_ad_evap", "cloudsc2_ad_evap_step")
MULTI = ("cloudsc2_ad_evap_multi", "cloudsc2_ad_evap_multi_step")


def evap(c, entry, p, sfx="f64", nx=64, ls=LS, in_=None, in_adj=None, zero=P, eta=P, tl=P, tn=P, out_adj=None, cover=P,
         ready=0, dirs=(2, FIELD, FIELD)):
    step = entry.endswith("step")
    in_ = (c.no_qsat() if step else c.arr([P] * 16)) if in_ is None else in_
    out_adj = (c.no_qsat() if step else c.arr([P] * 16)) if out_adj is None else out_adj
    in_adj = c.arr([P] * 10) if in_adj is None else in_adj
    head = (ctypes.byref(p), nx, NZ, ls, in_, in_adj, zero, eta, tl, tn, out_adj, 60.0)
    tail = (cover, ready, None) if entry in SINGLE else (None,) + tuple(dirs) + (cover, ready)
    return getattr(c.lib, f"{entry}_{sfx}")(*head, *tail)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("entry", SINGLE + MULTI)
def test_refusals(call, entry, sfx):
    on = call.params(LEVAPLS2=True)
    assert evap(call, entry, on, sfx, nx=0) == 0                                   # an empty call
    assert evap(call, entry, on, sfx, nx=0, cover=None) == 0
    assert evap(call, entry, on, sfx, cover=None) == -1 and "cover" in call.err()
    assert evap(call, entry, call.params(), sfx) == -2                             # neither switch
    base = entry.replace("_evap", "") if entry != "cloudsc2_ad_evap" else "cloudsc2_ad_masked"
    assert "LEVAPLS2" in call.err() and base in call.err(), call.err()
    assert evap(call, entry, call.params(LDRAIN1D=True), sfx, cover=None) == -1    # LDRAIN1D alone is such a call
    assert evap(call, entry, on, sfx, nx=-1) == -1 and "nx" in call.err()
    assert evap(call, entry, on, sfx, ls=32) == -1 and "lev_stride" in call.err()
    assert evap(call, entry, on, sfx, eta=None) == -1 and "eta" in call.err()
    assert evap(call, entry, on, sfx, tl=None) == -1 and "traj_fplsl" in call.err()
    assert evap(call, entry, on, sfx, in_adj=call.arr([0] * 10), zero=None) == -1 and "zero_line" in call.err()
    assert evap(call, entry, on, sfx, out_adj=call.arr([0] * 16)) == -1 and "out_adj" in call.err()
    assert evap(call, entry, on, sfx, in_=call.arr([0] * 16)) == -1 and "in" in call.err()
    if entry.endswith("step"):
        assert evap(call, entry, on, sfx, out_adj=call.arr([P] * 16)) == -1 and "NL_IN_QSAT" in call.err()
        assert evap(call, entry, call.params(LEVAPLS2=True, LPHYLIN=False), sfx) == -2 and "LPHYLIN" in call.err()
    if entry in MULTI:
        for ndir in (0, 9):
            assert evap(call, entry, on, sfx, dirs=(ndir, FIELD, FIELD)) == -1 and "ndir" in call.err()
        assert evap(call, entry, on, sfx, dirs=(2, FIELD - 1, FIELD)) == -1 and "overlap" in call.err()
        assert evap(call, entry, on, sfx, dirs=(2, FIELD, FIELD - 1)) == -1 and "overlap" in call.err()


def test_the_old_entries_still_refuse_the_switches(call):
    p = call.params(LEVAPLS2=True)
    for entry in ("cloudsc2_ad_masked", "cloudsc2_ad_step"):
        assert call.ad(p, entry=entry) == -2 and "use cloudsc2_ad" in call.err() and "LEVAPLS2 / LDRAIN1D" in call.err()
    for entry in ("cloudsc2_ad_multi", "cloudsc2_ad_multi_step"):
        assert call(entry, "f64", p) == -2 and "LEVAPLS2 / LDRAIN1D" in call.err()


def test_layouts_and_symbols(hip_lib):
    from gt4py_dwarf_p_cloudsc2_tl_ad_amd import _lib

    assert _lib.EVAP_LAYOUTS == {"ad_evap": "ad_masked", "ad_evap_step": "ad_step", "ad_evap_multi": "ad_multi",
                                 "ad_evap_multi_step": "ad_multi_step"}
    for name in _lib.EVAP_LAYOUTS:
        for sfx in ("f64", "f32"):
            assert f"cloudsc2_{name}_{sfx}" in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, f"cloudsc2_{name}_{sfx}")
    assert hip_lib.cloudsc2_abi_version() == 4
