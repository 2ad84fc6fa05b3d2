"""Float64 statement of the static-state mixer update (include/macjd_nets.h, ``macjd_mixer_fused_train_static``) on top
of tests/mixer_f64_model.py, and the inputs of its tests.  Nothing imported from the package.

Rows (b, t) of a [B, T1] batch are cut into 16-row tiles that never straddle two episodes: tile b * TPE + k, with
TPE = ceil(T1 / 16), owns t = 16 k .. 16 k + 15 of episode b; rows t >= T1 are dead and contribute nothing.  When the state
of every row that receives a loss gradient equals the state of its tile's row 0, each weight gradient
sum_m g[m]^T x[m] is sum_tiles (sum of the tile's rows of g)^T x[tile's row 0]."""
import numpy as np
import torch

import mixer_f64_model as mm

TILE = 16
HH, EM, NRELU, N1 = mm.HH, mm.EM, mm.NRELU, mm.N1
SUMMED = ("gout1", "g_w1raw", "g_wfraw", "g_v")     # per-tile sums over the rows
ROW0 = ("sn", "xhat", "act")                        # per-tile copies of the tile's row 0
# (B, T1) -> filled steps L per episode (the episode ends at row e = L - 1: terminated there unless L = T1 - 1, filled
# False from row L on).  e at the FIRST row of a tile: (3,5) ep 0, (2,16) ep 0, (3,33) ep 0 (e = 16), (1,101) (e = 96);
# at the LAST row of a tile: (2,17) ep 0 and (3,33) ep 1 (e = 15); mid-tile: the others.  (3,5): one tile with 11 dead
# rows; (2,16): an exact tile; (2,17), (3,33): a last tile with one live row (t = T1 - 1, no gradient); (1,101): the real T1.
CASES = {(3, 5): (1, 3, 4), (2, 16): (1, 15), (2, 17): (16, 8), (3, 33): (17, 16, 8), (1, 101): (97,)}


def tiles_per_episode(T1):
    return (T1 + TILE - 1) // TILE


def tile_rows(B, T1):
    """[(first row, one past the last row)] of every tile, in launch order."""
    tpe = tiles_per_episode(T1)
    return [(b * T1 + TILE * k, b * T1 + min(TILE * (k + 1), T1)) for b in range(B) for k in range(tpe)]


def compact(rows, B, T1):
    """Per-row float64 tensors (names of SUMMED and ROW0, [B * T1, ...]) -> the compact [n_tiles, ...] forms."""
    tr = tile_rows(B, T1)
    out = {}
    for k in SUMMED:
        x = mm.f64(rows[k]).reshape(B * T1, -1)
        out[k] = torch.stack([x[lo:hi].sum(0) for lo, hi in tr])
    for k in ROW0:
        x = mm.f64(rows[k]).reshape(B * T1, -1)
        out[k] = torch.stack([x[lo] for lo, _ in tr])
    return out


def grads_from_compact(c, W1):
    """The parameter gradients (mixer_f64_model's names) as the five products over K = n_tiles rows + the LayerNorm
    parameter gradients from the merged first layer's input gradient."""
    gout1, g_w1, g_wf, g_v = c["gout1"], c["g_w1raw"], c["g_wfraw"], c["g_v"].reshape(-1)
    sn, xhat, act = c["sn"], c["xhat"], c["act"]
    G = gout1 @ mm.f64(W1)
    return {"W1": gout1.T @ sn, "b1": gout1.sum(0), "W2": g_w1.T @ act[:, :HH], "b2": g_w1.sum(0),
            "Wf2": g_wf.T @ act[:, HH:2 * HH], "bf2": g_wf.sum(0), "wV2": g_v @ act[:, 2 * HH:NRELU],
            "bV2": g_v.sum().reshape(1), "ln_w": (G * xhat).sum(0), "ln_b": G.sum(0)}


def static_inputs(J, B, T1, lens=None, last_row_zero=True, salt=13):
    """mixer_f64_model.td_inputs with the state constant within each episode — except, with ``last_row_zero``, row
    T1 - 1, which is zeros as in the runner's stage buffers (no loss gradient reaches it) — and the episode ends of CASES
    (or ``lens``)."""
    pe, pt, q_e, q_t, state, reward, _, _ = mm.td_inputs(J, B, T1, salt=salt)
    state = np.repeat(state[:, :1], T1, axis=1).copy()
    if last_row_zero:
        state[:, -1] = 0.0
    lens = np.asarray(CASES[(B, T1)] if lens is None else lens, dtype=np.int64)
    assert lens.shape == (B,) and lens.min() >= 1 and lens.max() <= T1 - 1
    steps = np.arange(T1)[None, :, None]
    filled = steps < lens[:, None, None]
    terminated = (steps == lens[:, None, None] - 1) & (lens < T1 - 1)[:, None, None]
    return pe, pt, q_e, q_t, state, reward, terminated, filled
