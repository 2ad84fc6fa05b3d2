"""The package's MACJD_* switches: read from the environment ONCE (first use) into a table; ``reload()`` re-reads them
(tests and A/B scripts that change a switch inside a running process; the native library has its own:
``_native.reload_options()``).  Every switch selects a TESTED alternative of a default code path; nothing here is needed
for normal operation.

    MACJD_UPDATE_STREAMS      2 | 1      captured update on two streams (scan / prefetch beside the chain) or one
    MACJD_UPDATES_PER_GRAPH   K          updates captured per replayed graph when the caller does not say (bench / main: 20)
    MACJD_PIPELINED_GROUP     1 | 0      inside a group: next update's draw / gather / scan beside the current tail, target
                                         branch beside the head, loss gradient formed in the mixer's backward launch
    MACJD_SHARED_BODY         1 | 0      frozen agent body evaluated once for eval + target controller
    MACJD_LEARNER_STATIC_OBS  1 | 0      static observations: agent body once per sequence instead of per step
    MACJD_ACTOR_IN_SCAN       1 | 0      actor rows in the scan launch's prologue / as their own launch
    MACJD_DEVICE_SAMPLER      1 | 0      next batch drawn by the update's last launch / host draw + pinned upload
    MACJD_LN_IN_SQNORM        1 | 0      LayerNorm-parameter gradients inside the optimiser's first launch
    MACJD_NORM_IN_REDUCE      1 | 0      single process, default learner: LayerNorm-parameter gradients and the squared gradient norm
                                         formed by the weight-gradient launch pair, optimiser step as ONE launch / the
                                         squared-norm (+ LayerNorm) launch between the two
    MACJD_WGRAD_OUTER         1 | 0      Q-head ReLU-backward operand formed inside the weight-gradient launch
    MACJD_QHEAD_TAKEN         1 | 0      taken-action Q-head as one launch / input rows + GEMM + row-dot
    MACJD_QHEAD_DOUBLE_Q      1 | 0      Double-DQN target values as one launch from the hidden states / library GEMM bases +
                                         two Q-head launches
    MACJD_QHEAD_DOUBLE_Q_H128 0 | 1      the same choice at rnn_hidden_dim 128, where the one-launch form measured slower inside
                                         the update: two-launch form / one launch (needs MACJD_QHEAD_DOUBLE_Q != 0)
    MACJD_PAIRED_HEADS        1 | 0      pipelined update: both Q-head launches as one grid and both mixers as one grid on
                                         the chain's stream / target branch on the side stream beside the eval head
    MACJD_MIXER_TRAIN         1 | 0      paired update at 2 / 3 agents: both mixers, the loss gradient and the mixer backward
                                         as one launch / the mixer pair + the backward launch
    MACJD_MIXER_STATIC_STATE  1 | 0      that launch on a buffer with static observations / states: weight-gradient operands
                                         summed per 16-row tile of one episode ([n_tiles, ...], K = n_tiles) / written per row
    MACJD_WGRAD_IN_TRAIN      1 | 0      that static-state launch also leaves the Q-head's weight-gradient partials and the LayerNorm
                                         contraction as one slot per tile and the reduce launch forms the mixer's five products from
                                         the compact rows: no partial-products launch (default learner, f32 mixer, H = 64, A <= 15) /
                                         the partial-products launch
    MACJD_ROWS_STAGED         1 | 0      the reduce launch's row products: blocks of 256 outputs, one per thread, on operand rows
                                         staged once per block into LDS (bit-identical results) / two global loads per lane and term
    MACJD_PREFETCH_LAUNCH     1 | 0      pipelined group: a later update's draw, gather, mask sum and scan as ONE launch, the
                                         draw read-only at a baked counter offset / the four launches one behind the other
    MACJD_PREFETCH_AHEAD      2 | 1      that launch for the batches of TWO consecutive updates, issued two updates before the
                                         first of them (four staging sets) / one launch per update, issued by the one before it
    MACJD_GRAPHED_ALLREDUCE   0 | 1      with ranks: RCCL all-reduce captured inside the update graph
    MACJD_CLOSED_LOOP_ROLLOUT 0 | 1      scanning radars: step-by-step rollout / agent and env of an episode batch in one launch
                                         (shared scenario tables and per-env scanning scenario batches, pattern or not)
    MACJD_MOVING_EPISODE_ROLLOUT 0 | 1   moving scenarios: step-by-step rollout / one launch for the per-frame agent inputs, the
                                         agent's steps of an episode batch as one launch, the env's steps as another
    MACJD_CLOSED_LOOP_MOVING_ROLLOUT 0 | 1   moving scenarios under scanning radars: step-by-step rollout / agent and env of an
                                         episode batch in one launch on the frame tables
    MACJD_MOVING_PE_EPISODE_ROLLOUT 0 | 1   per-env moving scenario batches: step-by-step rollout / the agent's steps of an
                                         episode batch as one launch on every env's own frames, the env's steps as another
    MACJD_CLOSED_LOOP_MOVING_PE_ROLLOUT 0 | 1   per-env moving scanning scenario batches: step-by-step rollout / agent and env of
                                         an episode batch in one launch on every env's own frame tables
"""
from __future__ import annotations

import os

_DEFAULTS = {
    "UPDATE_STREAMS": "2", "UPDATES_PER_GRAPH": "1", "PIPELINED_GROUP": "1", "SHARED_BODY": "1",
    "LEARNER_STATIC_OBS": "1", "ACTOR_IN_SCAN": "1", "DEVICE_SAMPLER": "1", "LN_IN_SQNORM": "1", "NORM_IN_REDUCE": "1", "WGRAD_OUTER": "1",
    "QHEAD_TAKEN": "1", "QHEAD_DOUBLE_Q": "1", "QHEAD_DOUBLE_Q_H128": "0", "PAIRED_HEADS": "1", "MIXER_TRAIN": "1", "MIXER_STATIC_STATE": "1", "WGRAD_IN_TRAIN": "1", "ROWS_STAGED": "1", "GRAPHED_ALLREDUCE": "0",
    "PREFETCH_LAUNCH": "1", "PREFETCH_AHEAD": "2",
    "CLOSED_LOOP_ROLLOUT": "0", "MOVING_EPISODE_ROLLOUT": "0", "CLOSED_LOOP_MOVING_ROLLOUT": "0",
    "MOVING_PE_EPISODE_ROLLOUT": "0", "CLOSED_LOOP_MOVING_PE_ROLLOUT": "0",
}
_values = None


def reload() -> None:
    global _values
    _values = {k: os.environ.get("MACJD_" + k, d) for k, d in _DEFAULTS.items()}


def get(name: str) -> str:
    if _values is None:
        reload()
    return _values[name]


def on(name: str) -> bool:
    """The switch is not "0"."""
    return get(name) != "0"
