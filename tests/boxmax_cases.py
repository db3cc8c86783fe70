"""Box-maximum levels: a plain reference and the table of shapes, windows and fills that the CPU and
GPU tests share (test_cpu_boxmax_cases.py holds the reference, test_gpu_boxmax_levels.py the kernel).

The definition is the comment above k_boxmax_batch (csm_kernels.hip):

    out[r, c] = grid[s(r):s(r)+W, s(c):s(c)+W].max()      s(i) = min(i, n - W)

The shapes follow the kernel's constants (csm_device.hpp): an output tile of kBoxTR x kBoxTC = 32 x 64
cells, windows up to kBoxMaxWin = 64, rows pitched to a multiple of 8 columns."""
import functools

import numpy as np

TILE_ROWS, TILE_COLS, MAX_WIN, PITCH_UNIT = 32, 64, 64, 8

SHAPES = [
    (1, 1), (5, 300), (300, 5),                     # degenerate and thin grids
    (31, 63), (32, 64), (33, 65), (64, 128),        # one short of, exactly, one over whole tiles
    (95, 191),                                      # just under three tiles
    (97, 129),                                      # one over three by two tiles
    (64, 64), (65, 70),                             # for window 64
    (70, 57), (40, 71), (100, 121),                 # columns = 1, 7, 1 mod 8: pad columns exist
]
WINDOWS = (1, 2, 3, 5, 8, 16, 31, 32, 33, 63, 64)
FILLS = ("ramp_up", "ramp_down", "spikes", "random", "sparse")


def window_start(n, win):
    """s(i) = min(i, n - W) for i in [0, n): "repeat the last full window"."""
    return np.minimum(np.arange(n), n - win)


def boxmax_plain(grid, win):
    """The definition, cell by cell: the maximum of every full W x W window, and for output cell
    (r, c) the window that starts at (s(r), s(c))."""
    grid = np.asarray(grid)
    rows, cols = grid.shape
    if win < 1 or win > rows or win > cols:
        raise ValueError("window %d does not fit %dx%d" % (win, rows, cols))
    # full[i, j] = grid[i:i+W, j:j+W].max()
    full = np.lib.stride_tricks.sliding_window_view(grid, (win, win)).max(axis=(2, 3))
    return np.ascontiguousarray(full[np.ix_(window_start(rows, win), window_start(cols, win))])


def windows_for(rows, cols):
    """Every listed window that fits, plus W = rows and W = cols where the kernel takes them."""
    fit = min(rows, cols, MAX_WIN)
    wins = {w for w in WINDOWS if w <= fit}
    wins |= {w for w in (rows, cols) if w <= fit}
    return sorted(wins)


def make_grid(rows, cols, win, fill):
    """ramp_up: the maximum of a window is its far corner, so a window short by one fails.
    ramp_down: it is the near corner, so a window that starts one early or late fails.
    spikes: single 65535 cells at the grid's corners, around the first tile boundary and around
    the first window of the tail region. random: full-range uint16. sparse: 2 % non-zero."""
    assert rows * cols <= 65535         # the ramps stay strictly monotone in uint16
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    if fill == "ramp_up":
        return idx.astype(np.uint16)
    if fill == "ramp_down":
        return (rows * cols - 1 - idx).astype(np.uint16)
    if fill == "spikes":
        g = np.zeros((rows, cols), np.uint16)
        for r, c in ((0, 0), (rows - 1, cols - 1), (TILE_ROWS - 1, TILE_COLS - 1), (TILE_ROWS, TILE_COLS),
                     (rows - win, cols - win), (rows - win - 1, cols - win - 1)):
            if 0 <= r < rows and 0 <= c < cols:
                g[r, c] = 65535
        return g
    rng = np.random.RandomState((rows * 1000003 + cols * 1009 + win * 17 + FILLS.index(fill)) % (1 << 32))
    if fill == "random":
        return rng.randint(0, 65536, size=(rows, cols)).astype(np.uint16)
    if fill == "sparse":
        values = rng.randint(1, 65536, size=(rows, cols))
        return np.where(rng.rand(rows, cols) < 0.02, values, 0).astype(np.uint16)
    raise ValueError(fill)


def _cases():
    """Every (shape, window) once, the fills dealt out in turn so that each meets every shape and
    every window size; and all five fills at a shape's largest window, where the tail region (the
    cells whose window is the last full one) is largest."""
    out, turn = [], 0
    for rows, cols in SHAPES:
        wins = windows_for(rows, cols)
        for w in wins:
            first = FILLS[turn % len(FILLS)]
            turn += 1
            for fill in FILLS if w == wins[-1] else (first,):
                out.append((rows, cols, w, fill))
    return out


CASES = _cases()
CASE_IDS = ["%dx%d-w%d-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def case_arrays(rows, cols, win, fill):
    """(grid, boxmax_plain(grid, win)) of a case: computed once, shared, read-only."""
    grid = make_grid(rows, cols, win, fill)
    want = boxmax_plain(grid, win)
    grid.flags.writeable = False
    want.flags.writeable = False
    return grid, want
