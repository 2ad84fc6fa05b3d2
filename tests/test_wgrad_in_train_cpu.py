"""Host logic of the update without a partial-products launch (MACJD_WGRAD_IN_TRAIN): ``ops.norm_in_reduce_plan`` on
problems of the new kinds (``macjd_wgrad_io.kind``) — the shape the learner records, and each reason to refuse — the slot
layout arithmetic the host checks of ``macjd_mixer_fused_train_static_wgrad`` and the reduce launch share, and the
switch / exports.  Addresses are made up; nothing is launched."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(__file__))

from macjd_amd import _native, ops  # noqa: E402
from test_norm_in_reduce_cpu import BASE, COVER, OFF, _io  # noqa: E402

ORD, EXT, ROWS = _native.WGRAD_ORDINARY, _native.WGRAD_EXT_SLOTS, _native.WGRAD_ROW_PRODUCTS
N_TILES = 224


def _planned():
    """The default learner's problems as the planned update records them: W1 (row products over the compact rows), the
    contracted problem with the training launch's LayerNorm slots, and the Q-head-like problem from external slots."""
    g1, G = 0x500000, 0x600000
    ios = [_io(N_TILES, 384, 46, g1, 0x510000, BASE + 4 * OFF["W1"], BASE + 4 * OFF["b1"]),
           _io(N_TILES, 384, 46, g1, 0x520000, G, None),
           _io(1, 64, 32, None, None, BASE + 4 * OFF["W2"], BASE + 4 * OFF["b2"])]
    ios[0].kind, ios[0].workspace = ROWS, None
    ios[1].kind, ios[1].ext_chunks = EXT, N_TILES
    ios[2].kind, ios[2].ext_chunks = EXT, N_TILES
    ln = _native.LnParamIO()
    ln.C, ln.K, ln.W, ln.w_ld, ln.G, ln.g_ld = 384, 46, 0x700000, 46, G, 46
    ln.gb, ln.dgamma, ln.dbeta = BASE + 4 * OFF["b1"], BASE + 4 * OFF["gamma"], BASE + 4 * OFF["beta"]
    return ios, ln


def test_planned_update_is_taken():
    ios, ln = _planned()
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) == 1
    # the kinds may be mixed with ordinary problems
    ios[2].kind, ios[2].K, ios[2].gout, ios[2].inp = ORD, 808, 0x530000, 0x540000
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) == 1


def test_each_reason_to_refuse_a_kind():
    # external slots: none there, or no workspace
    ios, ln = _planned()
    ios[2].ext_chunks = 0
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    ios, ln = _planned()
    ios[1].workspace = None
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    # row products: with an operand formed on the fly, without rows, with more rows than an int counts
    ios, ln = _planned()
    ios[0].outer_vec = ios[0].outer_w = 0x770000
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    for K in (0, 2 ** 31):
        ios, ln = _planned()
        ios[0].K = K
        assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    # the contracted problem as row products: the reduce has no contraction of its own
    ios, ln = _planned()
    ios[1].kind = ROWS
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    # a kind nobody knows
    ios, ln = _planned()
    ios[2].kind = 3
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    # and the old reasons still hold for them: a gradient of the flat vector that the pair does not write
    ios, ln = _planned()
    assert ops.norm_in_reduce_plan(ios[:2], [ln], COVER) is None


def test_slot_layout_arithmetic():
    """Slot c of an [M, N] problem lies at c Mp Np (Mp / Np: M / N padded to 64), the bias rows behind all slots: what
    macjd_wgrad_slot_floats sizes, the mixer launch writes and the reduce launch reads."""
    lib = _native.load()
    pad = lambda v: (v + 63) // 64 * 64
    for M, N, slots in ((64, 74, N_TILES), (1, 64, N_TILES), (64, 70, 4), (64, 64, 1), (65, 129, 3)):
        assert int(lib.macjd_wgrad_slot_floats(M, N, slots)) == slots * pad(M) * pad(N) + slots * pad(M)
    # one slot per 64-row chunk is the ordinary problem's own workspace
    for K in (1, 64, 65, 9696):
        chunks = -(-K // 64)
        assert int(lib.macjd_wgrad_slot_floats(64, 74, chunks)) == int(lib.macjd_linear_wgrad_workspace_floats(K, 64, 74))
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0)):
        assert int(lib.macjd_wgrad_slot_floats(*bad)) == -1
    # kinds and work items of the partial-products launch (host tables only: nothing is launched)
    ios, _ = _planned()
    arr = (_native.WgradIO * 3)(*ios)
    assert int(lib.macjd_linear_wgrad_many_norm_work_items(arr, 3, 1)) == 0
    assert int(lib.macjd_linear_wgrad_many_norm_partials(arr, 3, 1)) == -(-((384 * 46 + 384) + 2 * 46 + (64 * 32 + 64)) // 64)
    ios[0].kind, ios[0].workspace = ORD, 0x900000
    arr = (_native.WgradIO * 3)(*ios)
    assert int(lib.macjd_linear_wgrad_many_norm_work_items(arr, 3, 1)) == 6 * 1 * 4     # 384 x 46 over 224 rows
    ios[2].ext_chunks = 0
    assert int(lib.macjd_linear_wgrad_many_norm_work_items((_native.WgradIO * 3)(*ios), 3, 1)) == -1


def test_struct_mirrors_switch_and_exports():
    from macjd_amd import options
    assert options._DEFAULTS["WGRAD_IN_TRAIN"] == "1" and "MACJD_WGRAD_IN_TRAIN" in options.__doc__
    assert ops.wgrad_in_train_supported(64, 9) and ops.wgrad_in_train_supported(64, 15) and ops.wgrad_in_train_supported(64, 1)
    assert not ops.wgrad_in_train_supported(64, 16) and not ops.wgrad_in_train_supported(128, 9) and not ops.wgrad_in_train_supported(64, 0)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "macjd_nets.h")).read()
    for name in ("macjd_mixer_fused_train_static_wgrad", "macjd_linear_wgrad_many_norm_work_items", "macjd_wgrad_slot_floats"):
        assert name in _native.EXPORTS and f"{name}(" in hdr
    # the C structs: the old block with two ints behind it, resp. the block's 17 eight-byte units
    assert ctypes.sizeof(_native.WgradIO) == 8 + 4 + 4 + 10 * 8 + 8
    assert [f[0] for f in _native.WgradIO._fields_][-2:] == ["kind", "ext_chunks"]
    assert ctypes.sizeof(_native.MixerWgradBlock) == 17 * 8
