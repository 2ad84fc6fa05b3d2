"""The address of an element of a tiled per-env frame table (include/macjd.h, macjd_motion_pe_io / macjd_motion_scan_pe_io),
as one NumPy expression: tests/test_episode_moving_scan_pe_cpu.py checks it against transposing gathers, and
tests/test_episode_moving_scan_pe_gpu.py builds its expected table values with it."""
import numpy as np


def tiled_index(e, f, row, rows, n_frames, tile):
    """Flat element index of row ``row`` of frame ``f`` of env ``e`` in a table [n_tiles, n_frames, rows, tile]:
    (((e / tile) * n_frames + f) * rows + row) * tile + e % tile.  The arguments broadcast; the positions table is passed
    with ``n_frames = F + 1``."""
    e, f, row = (np.asarray(x, dtype=np.int64) for x in (e, f, row))
    return (((e // tile) * n_frames + f) * rows + row) * tile + e % tile


def gather_frames(table, e, f):
    """Rows [len(e), rows] of a tiled table (numpy [n_tiles, n_frames, rows, tile]) at frame ``f[i]`` of env ``e[i]``."""
    n_tiles, n_frames, rows, tile = table.shape
    e, f = np.asarray(e, dtype=np.int64), np.asarray(f, dtype=np.int64)
    idx = tiled_index(e[:, None], f[:, None], np.arange(rows)[None, :], rows, n_frames, tile)
    return np.ascontiguousarray(table).reshape(-1)[idx]
