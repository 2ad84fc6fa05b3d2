"""``macjd_rowdot`` and ``macjd_splitrelu_backward`` (csrc/macjd_nets.hip) against the model of their contract
(tests/wgrad_f64_model.py, proved on the CPU in tests/test_wgrad_f64_cpu.py), through the C-ABI.

Row dot: K around the 64-column pass of a row's 16 lanes and at the limit, the 16-byte path and the scalar path (row stride
no multiple of 4, x or w one float off), row counts around the 16 rows of a workgroup and the 8192 workgroups of the capped
grid, bias NULL and given; "exact" data bit for bit, "bounded" data within the derived bound.
Split ReLU: one to four blocks with widths including 1, a NULL block first, inner and last, outer_w on none, some and all
blocks, Cp = 0 and > 0 with g_pass NULL and given, M = 0, 1, 7, item counts around a workgroup and around the capped grid,
act values +0.0, -0.0, the smallest normal and NaN; elementwise with at most one multiply, so always bit for bit.

Every buffer sits in a NaN-filled allocation between NaN margins, every padded row has NaN gaps.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import wgrad_f64_model as m  # noqa: E402
from nan_slab import Slab, dense, offsets, stream, strided  # noqa: E402

pytestmark = pytest.mark.gpu
OK, EINVAL = 0, -1                       # include/macjd.h
f32, f64, u32 = np.float32, np.float64, np.uint32
_WORST = {}


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


# ------------------------------------------------------------------------------------------------ macjd_rowdot
def _rowdot_io(_native, c, kind):
    d = m.rowdot_data(c, kind)
    rows, K = c["rows"], c["K"]
    x_ld = m.ld_of(K, c["x_ld"])
    bufs = {}
    if rows:
        bufs["x"], _ = strided(d["x"], (x_ld, 1), off=c["x_off"])
    else:
        bufs["x"] = Slab(K, off=c["x_off"])
    bufs["w"] = dense(d["w"], off=c["w_off"])
    bufs["y"] = Slab(max(rows, 4), off=1)
    io = _native.RowdotIO()
    io.n_rows, io.K, io.x, io.x_ld, io.w, io.y = rows, K, bufs["x"].ptr, x_ld, bufs["w"].ptr, bufs["y"].ptr
    if c["bias"]:
        bufs["b"] = dense(d["b"], off=3)
        io.b = bufs["b"].ptr
    vec = x_ld % 4 == 0 and io.x % 16 == 0 and io.w % 16 == 0
    assert vec == m.rowdot_vec(c), (c["name"], "takes the path the table says")
    return io, bufs


ROWDOT_GROUPS = {f"k{K}": [c["name"] for c in m.rowdot_cases() if c["name"].startswith(f"k{K}-")] for K in m.ROWDOT_K}
ROWDOT_GROUPS["rows"] = [c["name"] for c in m.rowdot_cases() if c["name"].startswith("rows")]


def test_rowdot_groups_cover_the_table():
    assert sorted(n for g in ROWDOT_GROUPS.values() for n in g) == sorted(c["name"] for c in m.rowdot_cases())


@pytest.mark.parametrize("group", list(ROWDOT_GROUPS))
def test_rowdot_against_the_model(group):
    _native, lib = _lib()
    for name in ROWDOT_GROUPS[group]:
        c = m.rowdot_case(name)
        rows = c["rows"]
        for kind in m.KINDS:
            io, bufs = _rowdot_io(_native, c, kind)
            assert lib.macjd_rowdot(ctypes.byref(io), stream()) == OK, name
            torch.cuda.synchronize()
            written = np.arange(rows)
            assert bufs["y"].rest_intact(written if rows else None), (name, "y outside [n_rows]")
            assert all(bufs[k].rest_intact() for k in bufs if k != "y"), (name, "an operand was written")
            if not rows:
                continue
            y, tol = m.rowdot_expect(c, kind)
            got = bufs["y"].read(written)
            assert np.isfinite(got).all(), (name, kind)
            if kind == "exact":
                bad = np.flatnonzero(_bits(got) != _bits(y.astype(f32) + f32(0)))
                assert bad.size == 0, (name, len(bad), bad[:4].tolist(), got[bad[0]], y[bad[0]])
            else:
                ratio = np.abs(got.astype(f64) - y) / tol
                assert float(ratio.max()) <= 1.0, (name, float(ratio.max()), int(ratio.argmax()))
                _WORST["macjd_rowdot"] = max(_WORST.get("macjd_rowdot", 0.0), float(ratio.max()))
            first = got.copy()
            assert lib.macjd_rowdot(ctypes.byref(io), stream()) == OK
            torch.cuda.synchronize()
            assert np.array_equal(_bits(bufs["y"].read(written)), _bits(first)), (name, "two runs differ")
    print("macjd_rowdot worst |got - model| / bound", round(_WORST.get("macjd_rowdot", 0.0), 4))


def test_rowdot_refusals_launch_nothing():
    _native, lib = _lib()
    assert lib.macjd_rowdot(None, stream()) == EINVAL
    c = m.rowdot_case("k68-vec-gaps")
    changes = [("K", 0), ("K", 6), ("K", 1028), ("K", -4), ("x_ld", c["K"] - 1), ("x_ld", 0), ("n_rows", -1), ("x", None), ("w", None), ("y", None)]
    for name, value in changes:
        io, bufs = _rowdot_io(_native, c, "exact")
        setattr(io, name, value)
        assert lib.macjd_rowdot(ctypes.byref(io), stream()) == EINVAL, (name, value)
        torch.cuda.synchronize()
        assert bufs["y"].rest_intact(), (name, value)


# ------------------------------------------------------------------------------------------------ macjd_splitrelu_backward
def _splitrelu_io(_native, c):
    """-> (io, buffers, gout offsets or None when M = 0)"""
    d = m.splitrelu_data(c)
    M, widths, Cp = c["M"], c["widths"], c["Cp"]
    Cr = sum(widths)
    g_ld, gp_ld, act_ld, gout_ld = m.splitrelu_strides(c)
    bufs = {}
    io = _native.SplitReluBwdIO()
    io.M, io.n_blocks, io.Cp = M, len(widths), Cp

    def put(key, values, ld, off):
        v = np.asarray(values, f32)
        if v.size:
            bufs[key], _ = strided(v, (ld, 1), off=off)
        else:
            bufs[key] = Slab(4, off=off)               # nothing to read: M = 0 or a width of 0 columns
        return bufs[key].ptr

    io.act, io.act_ld = put("act", d["act"], act_ld, 1), act_ld
    for k, w in enumerate(widths):
        io.width[k], io.g_ld[k] = w, g_ld[k]
        if d["g"][k] is not None:
            setattr(io, f"g{k}", put(f"g{k}", d["g"][k].reshape(M, 1 if d["ow"][k] is not None else w), g_ld[k], k % 3))
        if d["ow"][k] is not None:
            bufs[f"ow{k}"] = dense(d["ow"][k], off=(k + 1) % 3)
            setattr(io, f"ow{k}", bufs[f"ow{k}"].ptr)
    if d["g_pass"] is not None:
        io.g_pass = put("gp", d["g_pass"], gp_ld, 2)
    io.gp_ld = gp_ld
    go = offsets((M, Cr + Cp), (gout_ld, 1)) if M else None
    bufs["gout"] = Slab(int(go.max()) + 1 if M else 4, off=3)
    io.gout, io.gout_ld = bufs["gout"].ptr, gout_ld
    return io, bufs, go


@pytest.mark.parametrize("name", [c["name"] for c in m.splitrelu_cases()])
def test_splitrelu_backward_bit_for_bit(name):
    _native, lib = _lib()
    c = m.splitrelu_case(name)
    io, bufs, go = _splitrelu_io(_native, c)
    assert lib.macjd_splitrelu_backward(ctypes.byref(io), stream()) == OK
    torch.cuda.synchronize()
    assert bufs["gout"].rest_intact(go), (name, "gout outside [M x (Cr + Cp)]")
    assert all(bufs[k].rest_intact() for k in bufs if k != "gout"), (name, "an operand was written")
    if go is None:
        return
    want, got = m.splitrelu_expect(c), bufs["gout"].read(go)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    if c["special"]:
        assert np.isnan(m.splitrelu_data(c)["act"]).any() and np.isfinite(got).all()       # NaN > 0 is false: 0


def test_splitrelu_refusals_launch_nothing():
    _native, lib = _lib()
    assert lib.macjd_splitrelu_backward(None, stream()) == EINVAL
    c = m.splitrelu_case("b4-null-inner")              # widths (3, 1, 5, 2), Cp 4, block 2 NULL, outer_w on blocks 1 and 3
    Cr = sum(c["widths"])

    def field(name, value, idx=None):
        def f(io):
            if idx is None:
                setattr(io, name, value)
            else:
                getattr(io, name)[idx] = value
        return f, (name, idx, value)

    changes = [field("n_blocks", 0), field("n_blocks", 5), field("n_blocks", -1), field("M", -1), field("Cp", -1), field("act", None), field("gout", None),
               field("width", 0, 0), field("width", 0, 3), field("width", -2, 1),
               field("g_ld", c["widths"][0] - 1, 0), field("g_ld", 0, 1), field("g_ld", 0, 3),          # plain block; outer_w blocks: g_ld >= 1
               field("gp_ld", c["Cp"] - 1), field("act_ld", Cr - 1), field("gout_ld", Cr + c["Cp"] - 1)]
    for f, what in changes:
        io, bufs, _ = _splitrelu_io(_native, c)
        f(io)
        assert lib.macjd_splitrelu_backward(ctypes.byref(io), stream()) == EINVAL, what
        torch.cuda.synchronize()
        assert bufs["gout"].rest_intact(), what
