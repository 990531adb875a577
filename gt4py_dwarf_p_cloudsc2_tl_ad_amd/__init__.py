"""CLOUDSC2 (NL / TL / AD) on the MI355X.  `cloudsc2`, `tl_masked` and `ad_masked` (the differentiable `cloudsc2_nl` and the
masked linearisations underneath), `cloudsc2_step`, `saturation` and their thin calls (the whole step `saturation` +
`cloudsc2_nl` with its total derivative; `tl_multi` / `tl_step_multi` for many perturbations and `ad_multi` / `ad_step_multi` for many cotangents of one state; see `autodiff`) are resolved on first use, so importing the package stays free of
torch."""

_AUTODIFF = ("cloudsc2", "tl_masked", "ad_masked", "cloudsc2_step", "saturation", "saturation_tl", "saturation_ad", "tl_step",
             "ad_step", "tl_multi", "tl_step_multi", "ad_multi", "ad_step_multi")
__all__ = list(_AUTODIFF)


def __getattr__(name):
    if name in _AUTODIFF:
        from . import autodiff

        return getattr(autodiff, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
