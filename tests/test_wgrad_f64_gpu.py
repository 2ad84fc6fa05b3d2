"""``macjd_linear_wgrad`` / ``macjd_linear_wgrad_many`` (csrc/macjd_wgrad.hip) against the float64 model of their contract
(tests/wgrad_f64_model.py, proved on the CPU in tests/test_wgrad_f64_cpu.py), through the C-ABI: K at every edge of the
64-row chunk and of the reduce's rounds of eight chunks per wave and 32 per round, M and N around the 64-wide tiles, every
load width of the staging (16, 8 and 4 bytes, per operand, interior and ragged tile), padded dW rows, bias present and absent,
the operand formed from outer_vec / outer_w, one and eight problems per grouped launch, the cap of the reduce grid.

Every case runs twice over: with "exact" data the device must equal the model bit for bit (a dropped, doubled or mispaired
row cannot hide), with "bounded" data it must stay within the derived bound.  Every operand, output and workspace sits in a
NaN-filled allocation between NaN margins, padded rows carry NaN gaps: what a launch may not write must survive bit for bit,
and what it reads of its workspace it must have written.
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
OK, EINVAL, EUNSUPPORTED = 0, -1, -4     # include/macjd.h
f32, f64, u32 = np.float32, np.float64, np.uint32
_WORST = {}
CASES = [c["name"] for c in m.wgrad_cases()]


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def _io(_native, lib, c, kind, gout=None, inp=None):
    """-> (io, buffers, dW offsets); gout / inp: other operands than the case's own."""
    d = m.wgrad_data(c, kind)
    K, M, N = c["K"], c["M"], c["N"]
    g_ld, x_ld, dw_ld = m.wgrad_strides(c)
    bufs = {}
    bufs["gout"], _ = strided(d["gout"] if gout is None else gout, (g_ld, 1), off=c["g_off"])
    bufs["inp"], _ = strided(d["inp"] if inp is None else inp, (x_ld, 1), off=c["x_off"])
    dwo = offsets((M, N), (dw_ld, 1))
    bufs["dW"] = Slab(int(dwo.max()) + 1, off=c["dw_pad"] % 3)
    nws = lib.macjd_linear_wgrad_workspace_floats(K, M, N)
    assert nws == m.workspace_floats(K, M, N), (c["name"], "the chunk is not the 64 rows the table's K edges assume")
    bufs["ws"] = Slab(nws)
    io = _native.WgradIO()
    io.K, io.M, io.N = K, M, N
    io.gout, io.gout_ld, io.inp, io.inp_ld = bufs["gout"].ptr, g_ld, bufs["inp"].ptr, x_ld
    io.dW, io.dw_ld, io.workspace = bufs["dW"].ptr, dw_ld, bufs["ws"].ptr
    if c["bias"]:
        bufs["db"] = Slab(M, off=1)
        io.db = bufs["db"].ptr
    if c["outer"]:
        bufs["vec"], bufs["ow"] = dense(d["outer_vec"], off=1), dense(d["outer_w"], off=2)
        io.outer_vec, io.outer_w = bufs["vec"].ptr, bufs["ow"].ptr
    assert (io.gout % 16) // 4 == c["g_off"] and (io.inp % 16) // 4 == c["x_off"], (c["name"], "takes the load widths the table says")
    return io, bufs, dwo


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _outputs(c, bufs, dwo):
    return bufs["dW"].read(dwo), (bufs["db"].read() if c["bias"] else None)


def _untouched(c, bufs, dwo):
    assert bufs["dW"].rest_intact(dwo), (c["name"], "dW outside [M x N]")
    assert not c["bias"] or bufs["db"].rest_intact("all"), (c["name"], "db outside [M]")
    assert bufs["ws"].rest_intact("all"), (c["name"], "beyond macjd_linear_wgrad_workspace_floats")
    assert all(bufs[k].rest_intact() for k in bufs if k not in ("dW", "db", "ws")), (c["name"], "an operand was written")


def _ratio(got, want, tol):
    err = np.abs(got.astype(f64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))


def _check(key, c, kind, bufs, dwo):
    dW, db, tW, tb = m.wgrad_expect(c, kind)
    gW, gb = _outputs(c, bufs, dwo)
    assert np.isfinite(gW).all() and (gb is None or np.isfinite(gb).all()), (c["name"], kind, "read what it had not written")
    _untouched(c, bufs, dwo)
    if kind == "exact":         # (+ 0: the model's zero carries no sign)
        bad = np.argwhere(_bits(gW) != _bits(dW.astype(f32) + f32(0)))
        assert bad.size == 0, (c["name"], "dW", len(bad), bad[:4].tolist(), gW[tuple(bad[0])], dW[tuple(bad[0])])
        if gb is not None:
            bad = np.argwhere(_bits(gb) != _bits(db.astype(f32) + f32(0)))
            assert bad.size == 0, (c["name"], "db", len(bad), bad[:4].tolist(), gb[bad[0]], db[bad[0]])
        return 0.0
    rW = _ratio(gW, dW, tW)
    r = float(rW.max())
    assert r <= 1.0, (c["name"], "dW", r, np.unravel_index(int(rW.argmax()), rW.shape))
    if gb is not None:
        rb = _ratio(gb, db, tb)
        assert float(rb.max()) <= 1.0, (c["name"], "db", float(rb.max()), int(rb.argmax()))
        r = max(r, float(rb.max()))
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    return r


def _single(lib, io):
    assert lib.macjd_linear_wgrad(ctypes.byref(io), stream()) == OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", CASES)
def test_single_launch_against_the_model(name):
    _native, lib = _lib()
    c = m.wgrad_case(name)
    for kind in m.KINDS:
        io, bufs, dwo = _io(_native, lib, c, kind)
        _single(lib, io)
        r = _check("macjd_linear_wgrad", c, kind, bufs, dwo)
        first = _outputs(c, bufs, dwo)
        _single(lib, io)                                     # again, over its own workspace: the same bits
        again = _outputs(c, bufs, dwo)
        assert np.array_equal(_bits(first[0]), _bits(again[0])) and (first[1] is None or np.array_equal(_bits(first[1]), _bits(again[1])))
        _untouched(c, bufs, dwo)
        print(name, kind, m.wgrad_widths(c), "|got - model| / bound", round(r, 4))
    print("macjd_linear_wgrad worst |got - model| / bound", round(_WORST.get("macjd_linear_wgrad", 0.0), 4))


@pytest.mark.parametrize("which", ["gout-nan", "gout-inf", "inp-nan"])
def test_a_non_finite_operand_element_stays_in_its_row_or_column(which):
    """One NaN (one Inf) in the last row of the ragged last chunk and the last column of the ragged last tile: dW = gout^T inp
    takes it into row m (column n) alone, db into db[m] alone; everything else equals the clean run bit for bit."""
    _native, lib = _lib()
    c = m.wgrad_case("k2113")
    K, M, N = c["K"], c["M"], c["N"]
    assert K % m.CHUNK == 1 and M % m.TILE == 1 and N % m.TILE == 1
    d = m.wgrad_data(c, "bounded")
    io, bufs, dwo = _io(_native, lib, c, "bounded")
    _single(lib, io)
    cW, cb = _outputs(c, bufs, dwo)
    gout, inp = d["gout"].copy(), d["inp"].copy()
    if which == "inp-nan":
        inp[K - 1, N - 1] = np.nan
    else:
        gout[K - 1, M - 1] = np.nan if which == "gout-nan" else np.inf
    io, bufs, dwo = _io(_native, lib, c, "bounded", gout=gout, inp=inp)
    _single(lib, io)
    pW, pb = _outputs(c, bufs, dwo)
    _untouched(c, bufs, dwo)
    if which == "inp-nan":
        assert np.isnan(pW[:, N - 1]).all() and np.array_equal(_bits(pW[:, :N - 1]), _bits(cW[:, :N - 1]))
        assert np.array_equal(_bits(pb), _bits(cb))
    else:
        hit = np.isnan if which == "gout-nan" else np.isinf
        assert hit(pW[M - 1]).all() and hit(pb[M - 1])
        assert np.array_equal(_bits(pW[:M - 1]), _bits(cW[:M - 1])) and np.array_equal(_bits(pb[:M - 1]), _bits(cb[:M - 1]))


@pytest.mark.parametrize("name", [c["name"] for c in m.wgrad_cases() if c["outer"]])
def test_outer_form_equals_splitrelu_backward_then_the_ordinary_problem(name):
    """The operand formed while it is staged is the very expression of macjd_splitrelu_backward with an outer_w block: the
    materialised operand run as an ordinary problem gives the same bits (the comment in the kernel promises it)."""
    _native, lib = _lib()
    c = m.wgrad_case(name)
    g_ld = m.wgrad_strides(c)[0]
    for kind in m.KINDS:
        io, bufs, dwo = _io(_native, lib, c, kind)
        _single(lib, io)
        _check("macjd_linear_wgrad", c, kind, bufs, dwo)
        formed = _outputs(c, bufs, dwo)
        io2, bufs2, dwo2 = _io(_native, lib, c, kind)
        go = offsets((c["K"], c["M"]), (g_ld, 1))
        G = Slab(int(go.max()) + 1, off=c["g_off"])
        sio = _native.SplitReluBwdIO()
        sio.M, sio.n_blocks, sio.Cp = c["K"], 1, 0
        sio.width[0], sio.g0, sio.g_ld[0], sio.ow0 = c["M"], bufs2["vec"].ptr, 1, bufs2["ow"].ptr
        sio.act, sio.act_ld, sio.gout, sio.gout_ld = bufs2["gout"].ptr, g_ld, G.ptr, g_ld
        assert lib.macjd_splitrelu_backward(ctypes.byref(sio), stream()) == OK
        torch.cuda.synchronize()
        assert G.rest_intact(go)
        want = m.wgrad_operand(m.wgrad_data(c, kind)["gout"], m.wgrad_data(c, kind)["outer_vec"], m.wgrad_data(c, kind)["outer_w"])
        assert np.array_equal(_bits(G.read(go)), _bits(want.astype(f32)))
        io2.gout, io2.outer_vec, io2.outer_w = G.ptr, None, None
        _single(lib, io2)
        plain = _outputs(c, bufs2, dwo2)
        assert np.array_equal(_bits(formed[0]), _bits(plain[0])), (name, kind)
        assert formed[1] is None or np.array_equal(_bits(formed[1]), _bits(plain[1])), (name, kind)


@pytest.mark.parametrize("which", list(m.MANY_SETS))
def test_grouped_launch_against_the_model_and_the_single_launches(which):
    _native, lib = _lib()
    cases = [m.wgrad_case(n) for n in m.MANY_SETS[which]]
    for kind in m.KINDS:
        singles = []
        for c in cases:
            io, bufs, dwo = _io(_native, lib, c, kind)
            _single(lib, io)
            singles.append(_outputs(c, bufs, dwo))
        built = [_io(_native, lib, c, kind) for c in cases]
        ios = (_native.WgradIO * len(cases))(*[b[0] for b in built])
        assert lib.macjd_linear_wgrad_many(ios, len(cases), stream()) == OK
        torch.cuda.synchronize()
        for c, (_, bufs, dwo), one in zip(cases, built, singles):
            r = _check("macjd_linear_wgrad_many", c, kind, bufs, dwo)
            gW, gb = _outputs(c, bufs, dwo)
            assert np.array_equal(_bits(gW), _bits(one[0])), (which, kind, c["name"], "dW differs from the single launch")
            assert gb is None or np.array_equal(_bits(gb), _bits(one[1])), (which, kind, c["name"], "db differs from the single launch")
            print(which, kind, c["name"], "|got - model| / bound", round(r, 4))
        assert lib.macjd_linear_wgrad_many(ios, len(cases), stream()) == OK      # again: the same bits
        torch.cuda.synchronize()
        for c, (_, bufs, dwo), one in zip(cases, built, singles):
            gW, gb = _outputs(c, bufs, dwo)
            assert np.array_equal(_bits(gW), _bits(one[0])) and (gb is None or np.array_equal(_bits(gb), _bits(one[1])))
            _untouched(c, bufs, dwo)
    print("macjd_linear_wgrad_many worst |got - model| / bound", round(_WORST.get("macjd_linear_wgrad_many", 0.0), 4))


def _setter(name, value):
    return (lambda io: setattr(io, name, value)), (name, value)


def _refusals(c):
    ch = [_setter("K", 0), _setter("K", -1), _setter("M", 0), _setter("N", 0), _setter("N", -3), _setter("gout", None),
          _setter("inp", None), _setter("dW", None), _setter("workspace", None), _setter("gout_ld", c["M"] - 1),
          _setter("inp_ld", c["N"] - 1), _setter("dw_ld", c["N"] - 1), _setter("outer_vec", None), _setter("outer_w", None)]
    return [(f, what, EINVAL) for f, what in ch] + [(f, what, EUNSUPPORTED) for f, what in (_setter("kind", 1), _setter("kind", 2), _setter("kind", -1))]


def test_refusals_launch_nothing():
    _native, lib = _lib()
    c = m.wgrad_case("outer-k65")
    assert lib.macjd_linear_wgrad(None, stream()) == EINVAL and lib.macjd_linear_wgrad_many(None, 1, stream()) == EINVAL

    def still_nan(bufs):
        torch.cuda.synchronize()
        return bufs["dW"].rest_intact() and bufs["db"].rest_intact() and bufs["ws"].rest_intact()

    for change, what, rc in _refusals(c):
        io, bufs, _ = _io(_native, lib, c, "exact")
        change(io)
        assert lib.macjd_linear_wgrad(ctypes.byref(io), stream()) == rc, what
        assert still_nan(bufs), what
        # the grouped launch: a bad problem behind a good one refuses the whole call
        good, gb, _ = _io(_native, lib, m.wgrad_case("k1"), "exact")
        last, lb, _ = _io(_native, lib, m.wgrad_case("k63"), "exact")
        ios = (_native.WgradIO * 3)(good, io, last)
        assert lib.macjd_linear_wgrad_many(ios, 3, stream()) == rc, what
        assert still_nan(bufs) and still_nan(gb) and lb["dW"].rest_intact() and lb["ws"].rest_intact(), what
    io, bufs, _ = _io(_native, lib, c, "exact")
    ios = (_native.WgradIO * (m.MAX_BATCH + 1))(*([io] * (m.MAX_BATCH + 1)))
    for n in (0, -1, m.MAX_BATCH + 1):
        assert lib.macjd_linear_wgrad_many(ios, n, stream()) == EINVAL, n
    assert still_nan(bufs)
    # more chunks than the single launch's grid has: refused before any launch, so small buffers do
    io, bufs, _ = _io(_native, lib, m.wgrad_case("k1"), "exact")
    io.K = 65535 * m.CHUNK + 1
    assert lib.macjd_linear_wgrad_workspace_floats(io.K, 1, 1) == 65536 * (64 * 64 + 64)
    assert lib.macjd_linear_wgrad(ctypes.byref(io), stream()) == EUNSUPPORTED
    assert still_nan(bufs)
    for K, M, N in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert lib.macjd_linear_wgrad_workspace_floats(K, M, N) < 0
