"""`derivative_support.compare_directions` fails when it should: a batch of 2 directions x (3 + 1 levels) x 4 columns in 3
slots on the host passes as it is, and is refused with one altered word, a written padding level, a written slot behind
`ndir`, or a NaN inside the written range."""
import numpy as np
import pytest

from derivative_support import Box, compare_directions

NX, NZ, NDIR, SLOTS = 4, 3, 2, 3
NAME = "tnd_t"               # a full-level field: levels 0 .. NZ-1 are written, level NZ is padding


def _batch():
    """-> the batch as a launch leaves it (written range filled, everything else NaN), the single launches' rows"""
    rng = np.random.default_rng(3)
    rows = [{NAME: rng.standard_normal((NZ + 1, NX))} for _ in range(NDIR)]
    written = [np.where(np.arange(NZ + 1)[:, None] < NZ, r[NAME], np.nan) for r in rows]
    return {NAME: Box(NX, NZ, np.float64, "cpu", False).batch(written, slots=SLOTS)}, rows


def _compare(batch, rows):
    compare_directions("host batch", batch, rows, (NAME,), NZ, np.float64, NDIR)


def test_a_clean_batch_passes(capsys):
    batch, rows = _batch()
    assert tuple(batch[NAME].shape) == (SLOTS, NX, 1, NZ + 1)
    _compare(batch, rows)
    assert "bit-equal to the single launches: True" in capsys.readouterr().out


def _alter_one_word(f, rows):
    lev, col = np.unravel_index(np.argmax(np.abs(rows[1][NAME][:NZ])), (NZ, NX))
    f[1, col, 0, lev] *= 1.0 + 1e-6      # 1000 x the float64 rtol of `assert_close`


def _write_padding_level(f, rows):
    f[0, 2, 0, NZ] = 0.0


def _write_slot_behind_ndir(f, rows):
    f[NDIR, 0, 0, 0] = 0.0


def _nan_in_written_range(f, rows):
    f[1, 3, 0, 1] = float("nan")


@pytest.mark.parametrize("spoil,message", [(_alter_one_word, "outside tolerance"),
                                           (_write_padding_level, "padding level written"),
                                           (_write_slot_behind_ndir, "slot 2 >= ndir=2 written"),
                                           (_nan_in_written_range, "'tnd_t', 1")],
                         ids=["altered word", "padding level", "slot behind ndir", "nan"])
def test_a_spoilt_batch_is_refused(spoil, message):
    batch, rows = _batch()
    spoil(batch[NAME], rows)
    with pytest.raises(AssertionError, match=message):
        _compare(batch, rows)
