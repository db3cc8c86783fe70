"""Holds the reference the GPU box-maximum tests rest on (tests/boxmax_cases.py): the plain NumPy
restatement of the definition against the oracle's C++ restatement (orc_boxmax: a sliding-window
maximum per column, then per row), and both against the closed form on the ramps. No GPU."""
import numpy as np
import pytest

import boxmax_cases as BC


def test_case_table_covers_what_it_says():
    assert 150 <= len(BC.CASES) <= 200
    assert len(set(BC.CASES)) == len(BC.CASES)
    for rows, cols in BC.SHAPES:
        wins = {w for r, c, w, _ in BC.CASES if (r, c) == (rows, cols)}
        assert wins == set(BC.windows_for(rows, cols))
        assert all(w <= min(rows, cols, BC.MAX_WIN) for w in wins)
        for edge in (rows, cols):
            assert (edge in wins) == (edge <= min(rows, cols, BC.MAX_WIN))
        assert {f for r, c, w, f in BC.CASES if (r, c) == (rows, cols)} == set(BC.FILLS)
    for fill in BC.FILLS:                                   # every fill meets every window size
        assert {w for _, _, w, f in BC.CASES if f == fill} >= set(BC.WINDOWS)
    assert any(cols % BC.PITCH_UNIT for _, cols in BC.SHAPES)
    assert {w for _, _, w, _ in BC.CASES} >= {BC.MAX_WIN, 1}


@pytest.mark.parametrize("rows,cols,win,fill", BC.CASES, ids=BC.CASE_IDS)
def test_plain_reference_matches_oracle_and_closed_form(oracle, rows, cols, win, fill):
    grid, want = BC.case_arrays(rows, cols, win, fill)
    assert want.dtype == np.uint16 and want.shape == (rows, cols)
    got = oracle.boxmax(grid, win)
    assert got.tobytes() == want.tobytes()
    sr, sc = BC.window_start(rows, win), BC.window_start(cols, win)
    if fill == "ramp_up":           # the window's far corner
        assert np.array_equal(want, grid[np.ix_(sr + win - 1, sc + win - 1)])
    if fill == "ramp_down":         # its near corner
        assert np.array_equal(want, grid[np.ix_(sr, sc)])


def test_slice_per_cell_agrees_on_an_odd_shape():
    """boxmax_plain takes all full windows at once; the definition read literally, one slice per
    output cell, gives the same bytes."""
    rows, cols, win = 33, 65, 5
    grid = BC.make_grid(rows, cols, win, "random")
    out = np.zeros_like(grid)
    for r in range(rows):
        for c in range(cols):
            s_r, s_c = min(r, rows - win), min(c, cols - win)
            out[r, c] = grid[s_r:s_r + win, s_c:s_c + win].max()
    assert np.array_equal(out, BC.boxmax_plain(grid, win))


@pytest.mark.parametrize("rows,cols,win", [(8, 8, 0), (8, 8, -1), (8, 8, 9), (8, 20, 9), (20, 8, 9), (40, 71, 41)])
def test_both_references_reject_a_window_that_does_not_fit(oracle, rows, cols, win):
    grid = np.ones((rows, cols), np.uint16)
    with pytest.raises(ValueError):
        BC.boxmax_plain(grid, win)
    with pytest.raises(ValueError):
        oracle.boxmax(grid, win)
