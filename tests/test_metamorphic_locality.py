"""Column, member and direction locality, and permutation equivariance, of every NL, TL and AD entry - bit for bit.

The scheme is column-local, the kernels are not by construction: they stage levels in an LDS ring a workgroup shares, use
LDS-DMA, add member, direction and shared-field bases as 64-bit scalars, and treat a ragged last wave separately.  A result
that depends on a neighbouring column, member or direction shows against the oracle only beyond the tolerance; as a bit
difference it always shows.  No tolerance: tests/metamorphic_support.py `assert_bitwise`.

Entries (`metamorphic_support.ENTRIES`): `cloudsc2_nl` on its LDS ring and on its register path, `cloudsc2_nl_saturation` on
both, `cloudsc2_nl_perturbed`, `nl_ens`, `nl_fused_ens`, `nl_enss`, `nl_fused_enss`, `saturation`, `state_increment`,
`perturbed_state`, `column_dots` (its output is per column), and every TL and AD entry of tests/test_metamorphic_linearity.py.
The Taylor-reduction and `field_sums` kernels legitimately mix columns and are left out.  `eta` and the parameters are never
replaced.  The shared fields of the `*_enss_*` entries are per-column data of member 0: the column tests replace and permute
their columns like every other input, the member tests leave them alone."""
import numpy as np
import pytest

from metamorphic_support import (ENTRIES, NMEM, assert_bitwise, column_permutation, configurations, device_case, host_case, label,
                                 only, permuted, replaced, third_of_columns)

DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
MEMBER_ORDER = (2, 0, 1)


def _each(gpu, entry, dtype):
    for nx, window, flags in configurations(entry):
        c = host_case(nx, dtype, flags)
        run = lambda case, window=window: entry.run(device_case(gpu, entry, case, window))  # noqa: E731
        yield f"{entry.name} {label(nx, window, flags)} {np.dtype(dtype).name}", c, host_case(nx, dtype, flags, seed=1000), run


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_a_column_does_not_see_the_others(gpu, entry, dtype):
    """a fixed third of the columns - in every wave and workgroup - replaced in every per-column input by another seed's
    columns, then by NaN: the kept columns are bit-equal to the base run"""
    for what, c, other, run in _each(gpu, entry, dtype):
        cols = third_of_columns(c.nx)
        kept = np.setdiff1d(np.arange(c.nx), cols)
        base = run(c)
        assert_bitwise(f"{what} other columns", run(replaced(c, other, cols=cols)), base, cols=kept)
        assert_bitwise(f"{what} NaN columns", run(replaced(c, None, cols=cols)), base, cols=kept)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.members], ids=lambda e: e.name)
def test_a_member_does_not_see_the_others(gpu, entry, dtype):
    """all of member 1 replaced (another seed's member, then NaN): members 0 and 2 are bit-equal to the base run"""
    for what, c, other, run in _each(gpu, entry, dtype):
        base = only(run(c), lambda g, m, d, n: m != 1)
        assert_bitwise(f"{what} other member", run(replaced(c, other, member=1)), base)
        assert_bitwise(f"{what} NaN member", run(replaced(c, None, member=1)), base)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.dirs], ids=lambda e: e.name)
def test_a_direction_does_not_see_the_others(gpu, entry, dtype):
    """direction 2 replaced (another seed's, then NaN): every other direction, and what does not depend on the directions,
    is bit-equal to the base run"""
    for what, c, other, run in _each(gpu, entry, dtype):
        base = only(run(c), lambda g, m, d, n: d != 2)
        assert_bitwise(f"{what} other direction", run(replaced(c, other, direction=2)), base)
        assert_bitwise(f"{what} NaN direction", run(replaced(c, None, direction=2)), base)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_permuting_the_columns_permutes_the_result(gpu, entry, dtype):
    """a fixed permutation of the columns of every per-column input (nx unchanged: the same kernel and path, every column in
    another lane, wave and workgroup) permutes every output; for ensembles the same with the members"""
    for what, c, _, run in _each(gpu, entry, dtype):
        perm = column_permutation(c.nx)
        assert (perm != np.arange(c.nx)).all()
        base = run(c)
        assert_bitwise(f"{what} columns permuted", run(permuted(c, perm)), {k: (a[:, perm], lv) for k, (a, lv) in base.items()})
        if entry.members:
            want = {(g, m, d, n): base[(g, MEMBER_ORDER[m], d, n)] for g, m, d, n in base}
            assert_bitwise(f"{what} members permuted", run(permuted(c, members=MEMBER_ORDER)), want)
    assert NMEM == len(MEMBER_ORDER)
