"""The algebra of the static-state mixer update without a GPU (tests/mixer_static_model.py on tests/mixer_f64_model.py, float64):
with states constant per episode, the parameter gradients formed from operands summed per 16-row tile of one episode
times ONE input row per tile equal the model's row-by-row gradients — with dead rows in a tile (t >= T1), tiles that
begin past a short episode's end (every gradient row zero), the all-zero state row T1 - 1 of the runner's stage buffers,
and not when a row that receives gradient has another state than its tile's row 0 (the comparison is not vacuous)."""
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO  # noqa: F401

sys.path.insert(0, os.path.dirname(__file__))
import mixer_f64_model as mm  # noqa: E402
import mixer_static_model as ms  # noqa: E402

from macjd_amd import _native, options  # noqa: E402


def _row_by_row(J, B, T1, **kw):
    pe, pt, q_e, q_t, state, reward, terminated, filled = ms.static_inputs(J, B, T1, **kw)
    tq = mm.target_values(pt, q_t, state)
    ref, _ = mm.td_reference(pe, q_e, state, tq, reward, terminated, filled, mm.GAMMA)
    return pe, ref, filled


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("B,T1", sorted(ms.CASES))
def test_tile_summed_operands_give_the_row_by_row_gradients(J, B, T1):
    pe, ref, filled = _row_by_row(J, B, T1)
    c = ms.compact(ref, B, T1)
    n_tiles = B * ms.tiles_per_episode(T1)
    assert c["gout1"].shape == (n_tiles, ms.N1) and c["sn"].shape == (n_tiles, pe["W1"].shape[1])
    got = ms.grads_from_compact(c, pe["W1"])
    for k, want in ref["grads"].items():
        assert float(want.abs().max()) > 0, k
        np.testing.assert_allclose(got[k].numpy(), want.numpy(), rtol=1e-11, atol=1e-13 * float(want.abs().max()), err_msg=k)
    # tiles that begin at or past the episode's end, or hold only row T1 - 1: every summed operand is exactly zero
    lens = filled.reshape(B, T1).sum(1)
    dead = [b * ms.tiles_per_episode(T1) + k for b in range(B) for k in range(ms.tiles_per_episode(T1))
            if ms.TILE * k >= min(int(lens[b]), T1 - 1)]
    if (B, T1) in ((2, 17), (3, 33)):
        assert len(dead) >= 2
    for k in ms.SUMMED:
        assert bool((c[k][dead] == 0).all()), k


def test_a_changing_state_breaks_the_identity():
    """One gradient-carrying row with a state of its own: the tile-summed form no longer gives the gradients."""
    J, B, T1 = 3, 2, 17
    pe, pt, q_e, q_t, state, reward, terminated, filled = ms.static_inputs(J, B, T1)
    assert filled[0, 3, 0]
    state[0, 3, 0] += 5.0   # (not a shift of the whole row: LayerNorm would remove it)
    tq = mm.target_values(pt, q_t, state)
    ref, _ = mm.td_reference(pe, q_e, state, tq, reward, terminated, filled, mm.GAMMA)
    got = ms.grads_from_compact(ms.compact(ref, B, T1), pe["W1"])
    want = ref["grads"]["W1"]
    assert float((got["W1"] - want).abs().max()) > 1e-6 * float(want.abs().max())


def test_switch_and_binding():
    """MACJD_MIXER_STATIC_STATE is a known switch, on by default; the library exports the entry point and the ctypes
    mirror of macjd_mixer_static_io has the header's eight 8-byte members."""
    import ctypes
    assert options._DEFAULTS["MIXER_STATIC_STATE"] in ("0", "1")
    assert "macjd_mixer_fused_train_static" in _native.EXPORTS
    assert ctypes.sizeof(_native.MixerStaticIO) == 64
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    body = hdr.split("typedef struct macjd_mixer_static_io {")[1].split("} macjd_mixer_static_io;")[0]
    names = [f for f, _ in _native.MixerStaticIO._fields_]
    pos = [body.index(" " + n + ";") if n != "sn" else body.index("* sn;") for n in names]
    assert pos == sorted(pos), names
