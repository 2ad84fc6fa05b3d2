"""``macjd_mlp_forward`` / ``macjd_mlp_forward_pair`` (csrc/macjd_mlp.hip) against the float64 model of their contract
(tests/rollout_agent_model.py, proved on the CPU in tests/test_rollout_agent_cpu.py), through the C-ABI: row counts around
the 16-row strip and the 64-row tile, then 256 tiles (one per workgroup of the capped grid) and 257 tiles (one workgroup
takes two, the last ragged) for a resident chain and for the 12j/16r actor, whose layers are staged one at a time and whose
tile loop restages layer 0 over the last layer's image; three passes of the grid on a one-layer chain; input widths around
the 16-column quad and at the limit, 16-byte aligned (16-byte DMA) and with x or W one float off (4-byte DMA, up to four
passes per row); every supported output tile count, inner and last; every activation in an inner and the last position
(an inner sigmoid of width 9 leaves 0.5 in the strip's pad columns); one to three layers; a broadcast input row, padded
input and output rows; pairs of different forms and sizes, bit for bit against the single launches; every refusal.

Every output sits in a NaN-filled allocation between NaN margins, padded rows carry NaN gaps: what a launch may not write
must survive bit for bit.  Tolerance: min(the model's running forward bound, 1e-5 max(1, max|y|)) per element.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import rollout_agent_model as m  # noqa: E402
from nan_slab import Slab, dense, offsets, stream, strided  # noqa: E402

pytestmark = pytest.mark.gpu
OK, EINVAL, EUNSUPPORTED = 0, -1, -4     # include/macjd.h
f32, f64 = np.float32, np.float64
_WORST = {}


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def _x_ld(c):
    K0 = c["dims"][0]
    return {0: 0, "min": K0, "pad": K0 + 4 + c["x_off"]}[c["x_ld"]]


def _io(_native, c, x=None):
    """-> (io, buffers, y offsets); x: other input rows than the case's own."""
    x0, layers = m.mlp_data(c)
    x = x0 if x is None else x
    io = _native.MlpIO()
    io.n_rows, io.n_layers = c["rows"], len(layers)
    for l, d in enumerate(c["dims"]):
        io.dims[l] = d
    bufs = {}
    ld = _x_ld(c)
    bufs["x"], _ = strided(x, (ld if ld else c["dims"][0], 1), off=c["x_off"])
    io.x, io.x_ld = bufs["x"].ptr, ld
    for l, (W, b, act) in enumerate(layers):
        bufs[f"W{l}"], bufs[f"b{l}"] = dense(W, off=c["w_off"]), dense(b, off=(l + 1) % 2)
        io.W[l], io.b[l], io.act[l] = bufs[f"W{l}"].ptr, bufs[f"b{l}"].ptr, act
    N = c["dims"][-1]
    y_ld = N + c["y_pad"]
    yo = offsets((c["rows"], N), (y_ld, 1))
    bufs["y"] = Slab(int(yo.max()) + 1, off=c["y_pad"] % 2)
    io.y, io.y_ld = bufs["y"].ptr, y_ld
    return io, bufs, yo


def _dma16(c, io):
    """What the contract promises for this layout: (x moves 16 bytes per lane, W_0 does)."""
    K0 = c["dims"][0]
    return (K0 % 4 == 0 and io.x_ld % 4 == 0 and io.x % 16 == 0), (K0 % 4 == 0 and io.W[0] % 16 == 0)


def _check(key, c, bufs, yo):
    y, tol = m.mlp_expect(c)
    got = bufs["y"].read(yo).astype(f64)
    assert np.isfinite(got).all(), c["name"]
    ratio = np.abs(got - y) / tol
    r = float(ratio.max())
    assert r <= 1.0, (c["name"], r, float(np.abs(got - y).max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
    assert bufs["y"].rest_intact(yo), c["name"]
    assert all(bufs[k].rest_intact() for k in bufs if k != "y"), c["name"]      # inputs are not written
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    return r


def _run(key, names):
    _native, lib = _lib()
    for name in names:
        c = m.mlp_case(name)
        io, bufs, yo = _io(_native, c)
        x16, w16 = _dma16(c, io)
        K0 = c["dims"][0]
        assert x16 == (K0 % 4 == 0 and not c["x_off"]) and w16 == (K0 % 4 == 0 and not c["w_off"]), (name, "takes the DMA width it is meant to take")
        assert lib.macjd_mlp_forward(ctypes.byref(io), stream()) == OK, name
        torch.cuda.synchronize()
        print(name, m.mlp_form(c["dims"]), "|got - model| / tol", round(_check(key, c, bufs, yo), 3))
    print(key, "worst", round(_WORST[key], 3))


GROUPS = {
    "rows resident": [c["name"] for c in m.mlp_cases() if c["name"].startswith("rows") and c["name"].endswith("resident")],
    "rows staged": [c["name"] for c in m.mlp_cases() if c["name"].startswith("rows") and c["name"].endswith("staged")],
    "three grid passes": ["rows49153-onelayer"],
    "input width aligned": [c["name"] for c in m.mlp_cases() if c["name"].endswith("-aligned")],
    "input width x off": [c["name"] for c in m.mlp_cases() if c["name"].endswith("-xodd") and c["name"].startswith("k")],
    "input width W off": [c["name"] for c in m.mlp_cases() if c["name"].endswith("-wodd")],
    "output width": [c["name"] for c in m.mlp_cases() if c["name"].startswith("n")],
    "activations": [c["name"] for c in m.mlp_cases() if c["name"].startswith("act")],
    "broadcast row": [c["name"] for c in m.mlp_cases() if c["name"].startswith("bcast")],
}


def test_groups_cover_the_table():
    assert sorted(n for g in GROUPS.values() for n in g) == sorted(c["name"] for c in m.mlp_cases())


@pytest.mark.parametrize("group", list(GROUPS))
def test_mlp_against_the_model(group):
    _run("mlp y " + group, GROUPS[group])


def test_a_non_finite_input_row_stays_in_its_row():
    """Rows are independent.  16449 rows of a chain without ReLU (fmaxf would drop a NaN): workgroup 0 takes tiles 0 and 256,
    so row 16384 + 5 is staged into the strip row that held the NaN activations of row 5, whose columns 46 and 47 are pad
    columns of the 46-wide input: they must be zeroed again, 0 x NaN is NaN."""
    _native, lib = _lib()
    c = m.mlp_case("rows16449-linear-resident")
    x = m.mlp_data(c)[0].copy()
    x[5, 7] = np.nan
    io, bufs, yo = _io(_native, c, x=x)
    assert lib.macjd_mlp_forward(ctypes.byref(io), stream()) == OK
    torch.cuda.synchronize()
    y, tol = m.mlp_expect(c)
    got = bufs["y"].read(yo).astype(f64)
    assert np.isnan(got[5]).all()
    rest = np.arange(c["rows"]) != 5
    assert np.isfinite(got[rest]).all(), np.nonzero(~np.isfinite(got).all(axis=1))[0][:8]
    assert (np.abs(got - y)[rest] <= tol[rest]).all() and bufs["y"].rest_intact(yo)


@pytest.mark.parametrize("a,b", m.MLP_PAIRS)
def test_pair_equals_the_single_launches_bit_for_bit(a, b):
    _native, lib = _lib()
    ca, cb = m.mlp_case(a), m.mlp_case(b)
    single = []
    for c in (ca, cb):
        io, bufs, yo = _io(_native, c)
        assert lib.macjd_mlp_forward(ctypes.byref(io), stream()) == OK
        torch.cuda.synchronize()
        single.append(bufs["y"].read(yo))
    (io0, b0, y0), (io1, b1, y1) = _io(_native, ca), _io(_native, cb)
    assert lib.macjd_mlp_forward_pair(ctypes.byref(io0), ctypes.byref(io1), stream()) == OK
    torch.cuda.synchronize()
    for c, bufs, yo, one in ((ca, b0, y0, single[0]), (cb, b1, y1, single[1])):
        r = _check("mlp y pair", c, bufs, yo)
        assert np.array_equal(bufs["y"].read(yo).view(np.uint32), one.view(np.uint32)), (a, b, c["name"])
    print(a, b, m.mlp_form(ca["dims"]), m.mlp_form(cb["dims"]), "worst", round(_WORST["mlp y pair"], 3), round(r, 3))


def test_pair_refuses_a_problem_without_rows():
    _native, lib = _lib()
    for zero in (0, 1):
        ios = [_io(_native, m.mlp_case("rows17-resident")), _io(_native, m.mlp_case("rows17-staged"))]
        ios[zero][0].n_rows = 0
        assert lib.macjd_mlp_forward_pair(ctypes.byref(ios[0][0]), ctypes.byref(ios[1][0]), stream()) == EINVAL
        torch.cuda.synchronize()
        assert ios[0][1]["y"].rest_intact() and ios[1][1]["y"].rest_intact()
    io, bufs, _ = _io(_native, m.mlp_case("rows17-resident"))
    assert lib.macjd_mlp_forward_pair(ctypes.byref(io), None, stream()) == EINVAL
    assert lib.macjd_mlp_forward_pair(None, ctypes.byref(io), stream()) == EINVAL
    io.n_rows = 0                                       # the single launch: nothing to do, nothing written
    assert lib.macjd_mlp_forward(ctypes.byref(io), stream()) == OK
    torch.cuda.synchronize()
    assert bufs["y"].rest_intact()


@pytest.mark.parametrize("dims", m.MLP_UNSUPPORTED, ids=["-".join(map(str, d)) for d in m.MLP_UNSUPPORTED])
def test_unsupported_sizes_are_refused_with_outputs_untouched(dims):
    _native, lib = _lib()
    assert m.mlp_form(dims) == "unsupported"
    rng = np.random.default_rng(len(dims) + dims[0])
    io = _native.MlpIO()
    io.n_rows, io.n_layers = 33, len(dims) - 1
    keep = [dense(rng.standard_normal((33, dims[0])))]
    io.x, io.x_ld = keep[0].ptr, dims[0]
    for l in range(len(dims) - 1):
        io.dims[l], io.dims[l + 1], io.act[l] = dims[l], dims[l + 1], m.ACT_RELU
        keep += [dense(rng.standard_normal((dims[l + 1], dims[l]))), dense(rng.standard_normal(dims[l + 1]))]
        io.W[l], io.b[l] = keep[-2].ptr, keep[-1].ptr
    y = Slab(33 * dims[-1])
    io.y, io.y_ld = y.ptr, dims[-1]
    assert lib.macjd_mlp_forward(ctypes.byref(io), stream()) == EUNSUPPORTED
    assert lib.macjd_mlp_forward_pair(ctypes.byref(io), ctypes.byref(io), stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert y.rest_intact()


def test_argument_errors_leave_the_output_alone():
    _native, lib = _lib()
    assert lib.macjd_mlp_forward(None, stream()) == EINVAL
    c = m.mlp_case("act-sigmoid-3layers")

    def attempt(change, what):
        io, bufs, _ = _io(_native, c)
        change(io)
        assert lib.macjd_mlp_forward(ctypes.byref(io), stream()) == EINVAL, what
        good, gb, _ = _io(_native, c)
        assert lib.macjd_mlp_forward_pair(ctypes.byref(good), ctypes.byref(io), stream()) == EINVAL, what
        torch.cuda.synchronize()
        assert bufs["y"].rest_intact() and gb["y"].rest_intact(), what

    def setter(name, value, idx=None):
        def f(io):
            if idx is None:
                setattr(io, name, value)
            else:
                getattr(io, name)[idx] = value
        return f, (name, idx, value)

    changes = [setter("n_layers", 0), setter("n_layers", 4), setter("n_layers", -1), setter("n_rows", -1), setter("x", None),
               setter("y", None), setter("x_ld", c["dims"][0] - 1), setter("x_ld", -1), setter("y_ld", c["dims"][-1] - 1), setter("y_ld", 0)]
    for l in range(3):
        changes += [setter("W", None, l), setter("b", None, l), setter("act", -1, l), setter("act", 3, l)]
    changes += [setter("dims", 0, k) for k in range(4)] + [setter("dims", -16, 1)]
    for f, what in changes:
        attempt(f, what)
