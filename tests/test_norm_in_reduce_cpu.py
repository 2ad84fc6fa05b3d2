"""``ops.norm_in_reduce_plan``: when the grouped weight-gradient launch pair may also form the LayerNorm gradients and the
squared gradient norm (MACJD_NORM_IN_REDUCE) — and when the three-launch tail has to stay.  Pure host logic on the ctypes
descriptors; the addresses are made up."""
import os
import sys

sys.path.insert(0, os.path.dirname(__file__))

from macjd_amd import _native, ops  # noqa: E402

BASE = 0x10000   # the flat gradient vector: W1 [384, 46] | b1 [384] | gamma [46] | pad 2 | beta [46] | pad 2 | W2 [64, 32] | b2 [64]
OFF = {"W1": 0, "b1": 384 * 46, "gamma": 384 * 46 + 384, "beta": 384 * 46 + 384 + 48, "W2": 384 * 46 + 384 + 96,
       "b2": 384 * 46 + 384 + 96 + 64 * 32}
SIZE = {"W1": 384 * 46, "b1": 384, "gamma": 46, "beta": 46, "W2": 64 * 32, "b2": 64}
COVER = [(BASE + 4 * OFF[k], 4 * SIZE[k]) for k in OFF]


def _io(K, M, N, gout, inp, dW, db, dw_ld=None):
    io = _native.WgradIO()
    io.K, io.M, io.N, io.gout, io.gout_ld, io.inp, io.inp_ld = K, M, N, gout, M, inp, N
    io.dW, io.dw_ld, io.db, io.workspace = dW, dw_ld or N, db, 0x900000
    return io


def _default():
    g1, G = 0x500000, 0x600000
    ios = [_io(808, 384, 46, g1, 0x510000, BASE + 4 * OFF["W1"], BASE + 4 * OFF["b1"]),
           _io(808, 384, 46, g1, 0x520000, G, None),
           _io(808, 64, 32, 0x530000, 0x540000, BASE + 4 * OFF["W2"], BASE + 4 * OFF["b2"])]
    ln = _native.LnParamIO()
    ln.C, ln.K, ln.W, ln.w_ld, ln.G, ln.g_ld = 384, 46, 0x700000, 46, G, 46
    ln.gb, ln.dgamma, ln.dbeta = BASE + 4 * OFF["b1"], BASE + 4 * OFF["gamma"], BASE + 4 * OFF["beta"]
    return ios, ln


def test_default_learner_shape_is_taken():
    ios, ln = _default()
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) == 1


def test_old_path_kept_where_required():
    ios, ln = _default()
    # a gradient of the flat vector that this launch pair does not write (another launch's, or flushed early)
    assert ops.norm_in_reduce_plan(ios[:2], [ln], COVER) is None
    assert ops.norm_in_reduce_plan(ios, [ln], COVER + [(BASE + 4 * 30000, 4 * 100)]) is None
    # no LayerNorm launch, or two
    assert ops.norm_in_reduce_plan(ios, [], COVER) is None
    assert ops.norm_in_reduce_plan(ios, [ln, ln], COVER) is None
    # more problems than one launch pair holds
    assert ops.norm_in_reduce_plan(ios + [ios[2]] * 6, [ln], COVER) is None
    # gb is not the column sums of the contracted problem's operand
    ios, ln = _default()
    ios[0].gout = 0x5f0000
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    # G is nobody's output; G has a bias output; N above one column tile
    ios, ln = _default()
    ln.G = 0x660000
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    ios, ln = _default()
    ios[1].db = 0x670000
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    ios, ln = _default()
    ios[1].N = ln.K = 65
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None
    # a strided weight-gradient output leaves gaps nobody writes: not counted as written
    ios, ln = _default()
    ios[2].dw_ld = 40
    assert ops.norm_in_reduce_plan(ios, [ln], COVER) is None


def test_switch_and_exports():
    from macjd_amd import options
    assert options._DEFAULTS["NORM_IN_REDUCE"] == "1"
    for name in ("macjd_linear_wgrad_many_norm", "macjd_linear_wgrad_many_norm_partials", "macjd_clip_adam_step_reduced"):
        assert name in _native.EXPORTS
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "macjd_nets.h")).read()
    for name in ("macjd_wgrad_norm_io", "macjd_linear_wgrad_many_norm(", "macjd_clip_adam_step_reduced("):
        assert name in hdr
