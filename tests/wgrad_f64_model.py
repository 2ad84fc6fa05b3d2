"""Float64 model of three launches of the learner's backward, written from the contract in include/macjd_nets.h
(``macjd_wgrad_io``, ``macjd_rowdot_io``, ``macjd_splitrelu_bwd_io``) — not from the kernels — with the bounds and the case
tables that tests/test_wgrad_f64_cpu.py proves fair and tests/test_wgrad_f64_gpu.py and
tests/test_rowdot_splitrelu_f64_gpu.py run.  Plain NumPy; it shares no code with the package.

Weight gradient: dW = gout^T inp, db = sum_k gout in float64 from the float32 operands; with ``outer_vec`` the [K, M] operand
is (gout[k, m] > 0) ? f32(outer_vec[k] * outer_w[m]) : 0 — ONE float32 rounding, then the product in float64.
Row dot: y = x . w + b.  Split ReLU: the header's expression in float32 (elementwise, at most one multiply: bit for bit).

Bounds, u = 2^-24, gamma(k) = k u / (1 - k u), per output gamma(c) sum |terms|:
* weight gradient: c = 64 + 1 (a work item's 64-row sum in any order, a product rounding counted even where the hardware
  fuses it) + ceil(chunks / 32) + 3 + 2 (one of a wave's eight accumulators, their tree, the four waves — the reduce's chain
  as tests/test_wgrad_kinds_gpu.py counts it), chunks = ceil(K / 64).  db: the same c over the terms gout[k, m].
* row dot: c = 4 ceil(K / 64) + 4 + 1 (a lane's fused multiply-adds, the four shuffle steps, the bias), terms x w and b.
Nothing is measured into a bound.

Two kinds of data per shape:
* "bounded": normal draws with |x| clamped to [2^-6, 2^3] (no product is subnormal) — they check the rounding behaviour;
* "exact": nonzero multiples of 1/8 in [-1, 1] (outer_vec / outer_w: nonzero multiples of 1/4) — every product and every
  partial sum is exact in float32 in ANY order (K < 2^17), so the device must equal the model bit for bit.  This is what
  notices a dropped, doubled or mispaired row; the bound alone cannot.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
CHUNK = 64                # rows of the reduction per work item, as macjd_linear_wgrad_workspace_floats implies it
TILE = 64                 # output tile (rows of dW and columns of dW)
MAX_BATCH = 8             # MACJD_WGRAD_MAX_BATCH
RED_GROUP, RED_CAP = 64, 8192      # outputs per reduce workgroup, cap of the reduce grid
LO, HI = 2.0 ** -6, 2.0 ** 3
KINDS = ("bounded", "exact")


def gamma(k):
    return k * U / (1.0 - k * U)


def _rng(*key):
    return np.random.default_rng([ord(c) for k in key for c in str(k)] or [0])


def bounded(rng, shape):
    v = rng.standard_normal(shape)
    return (np.where(v < 0, -1.0, 1.0) * np.clip(np.abs(v), LO, HI)).astype(f32)


def eighths(rng, shape, step=8):
    """nonzero multiples of 1 / step in [-1, 1]"""
    v = rng.integers(1, step + 1, shape) * rng.choice([-1, 1], shape)
    return (v / step).astype(f32)


def draw(kind, rng, shape, step=8):
    return bounded(rng, shape) if kind == "bounded" else eighths(rng, shape, step)


# ------------------------------------------------------------------------------------------------ macjd_wgrad_io
def chunks_of(K):
    return -(-K // CHUNK)


def wgrad_c(K):
    return CHUNK + 1 + -(-chunks_of(K) // 32) + 3 + 2


def workspace_floats(K, M, N):
    Mp, Np = -(-M // TILE) * TILE, -(-N // TILE) * TILE
    return chunks_of(K) * Mp * Np + chunks_of(K) * Mp


def wgrad_operand(gout, outer_vec=None, outer_w=None):
    """The [K, M] operand in float64: gout itself, or the form of the header from the ReLU's output."""
    if outer_vec is None:
        return np.asarray(gout, f64)
    prod = (np.asarray(outer_vec, f32)[:, None] * np.asarray(outer_w, f32)[None, :]).astype(f32)     # one float32 rounding
    return np.where(np.asarray(gout, f32) > 0, prod, f32(0)).astype(f64)


def wgrad(gout, inp, outer_vec=None, outer_w=None):
    """-> dW [M, N], db [M], tolerance of dW, of db (float64)"""
    A, X = wgrad_operand(gout, outer_vec, outer_w), np.asarray(inp, f64)
    g = gamma(wgrad_c(A.shape[0]))
    return A.T @ X, A.sum(0), g * (np.abs(A).T @ np.abs(X)), g * np.abs(A).sum(0)


def ld_of(cols, mode):
    """row stride of a [*, cols] operand: "min", or padded — "pad4" a multiple of 4, "even" even only, "odd" odd"""
    if mode == "min":
        return cols
    if mode == "pad4":
        return (cols // 4 + 1) * 4
    if mode == "even":
        return next(v for v in range(cols + 1, cols + 5) if v % 4 == 2)
    assert mode == "odd"
    return next(v for v in range(cols + 1, cols + 3) if v % 2 == 1)


def load_width(base, ld, cols, tile):
    """Bytes per load with which the partial-products launch stages the 64 columns [64 tile, 64 tile + 64) of an operand
    whose base pointer is `base` floats off a 16-byte boundary: 16 (rows 16-byte aligned, tile inside the matrix), 8 (even
    row length and stride: a column pair is inside or outside as a whole) or 4."""
    if ld % 4 == 0 and base % 4 == 0 and TILE * tile + TILE <= cols:
        return 16
    if ld % 2 == 0 and cols % 2 == 0 and base % 2 == 0 and cols >= 2:
        return 8
    return 4


def _wc(name, K, M, N, g_ld="min", x_ld="min", g_off=0, x_off=0, dw_pad=0, bias=True, outer=False):
    return dict(name=name, K=K, M=M, N=N, g_ld=g_ld, x_ld=x_ld, g_off=g_off, x_off=x_off, dw_pad=dw_pad, bias=bias, outer=outer)


def wgrad_cases():
    """g_ld / x_ld: stride mode of gout / inp (ld_of); g_off / x_off: floats off a 16-byte boundary; dw_pad = dw_ld - N.
    The comment of a case names the K edge (in chunks of 64 rows) and the load widths (gout | inp, per column tile)."""
    return [
        _wc("k1", 1, 1, 1),                                                    # one row, one chunk; 4r | 4r
        _wc("k63", 63, 2, 63, x_off=1, dw_pad=1, bias=False),                  # a ragged single chunk; 8r | 4r
        _wc("k64", 64, 64, 64, dw_pad=4),                                      # a full single chunk; 16 | 16
        _wc("k65", 65, 65, 66, g_ld="pad4"),                                   # second chunk of one row; 16, 4r | 8, 8r
        _wc("k512", 512, 66, 65, g_ld="pad4", x_off=2, dw_pad=3),              # eight chunks: wave 0 alone; 16, 8r | 4, 4r
        _wc("k513", 513, 63, 2, g_ld="pad4", g_off=1, x_off=2),                # the ninth: wave 1's first; 4r | 8r
        _wc("k1536", 1536, 128, 1, x_ld="odd", bias=False),                    # 24 chunks: waves 0..2; 16, 16 | 4r
        _wc("k1537", 1537, 1, 128, g_ld="even", x_off=2, dw_pad=2),            # wave 3's first chunk; 4r | 8, 8
        _wc("k2048", 2048, 129, 64, g_ld="pad4", x_ld="even"),                 # 32 chunks: one full round; 16, 16, 4r | 8
        _wc("k2049", 2049, 64, 129, g_ld="odd", x_off=1, dw_pad=1, bias=False),  # the 33rd: wave 0's second round; 4 | 4, 4, 4r
        _wc("k2113", 2113, 129, 129, g_off=1, x_ld="pad4"),                    # 34 chunks, the last with one row; 4, 4, 4r | 16, 16, 4r
        _wc("m128-g8", 65, 128, 66, g_off=2, x_ld="pad4"),                     # 8, 8 | 16, 8r
        _wc("m66-g8", 130, 66, 128, g_ld="even"),                              # 8, 8r | 16, 16
        _wc("outer-k65", 65, 65, 65, x_ld="pad4", outer=True),                 # M across a tile edge, K across a chunk edge; 4, 4r | 16, 4r
        _wc("outer-k130", 130, 64, 7, g_ld="odd", x_off=1, dw_pad=1, bias=False, outer=True),
        _wc("outer-k2113", 2113, 129, 66, g_ld="pad4", x_ld="even", outer=True),
        _wc("cap-exact", 2, 512, 1023),                                        # M N + M = 8192 * 64: every reduce workgroup once
        _wc("cap-plus", 2, 700, 748, g_ld="pad4"),                             # 8192 * 64 + 12: workgroup 0 takes a second group
    ]


def wgrad_case(name):
    return next(c for c in wgrad_cases() if c["name"] == name)


def wgrad_strides(c):
    return ld_of(c["M"], c["g_ld"]), ld_of(c["N"], c["x_ld"]), c["N"] + c["dw_pad"]


def wgrad_widths(c):
    """[(operand, "interior" | "ragged", bytes)] over the column tiles of both operands"""
    g_ld, x_ld, _ = wgrad_strides(c)
    out = []
    for op, base, ld, cols in (("gout", c["g_off"], g_ld, c["M"]), ("inp", c["x_off"], x_ld, c["N"])):
        for t in range(-(-cols // TILE)):
            out.append((op, "interior" if TILE * t + TILE <= cols else "ragged", load_width(base, ld, cols, t)))
    return out


@functools.lru_cache(maxsize=None)
def _wgrad_data(name, kind):
    c = wgrad_case(name)
    rng = _rng("wgrad", name, kind)
    K, M, N = c["K"], c["M"], c["N"]
    d = dict(inp=draw(kind, rng, (K, N)), outer_vec=None, outer_w=None)
    if c["outer"]:      # gout is a ReLU's OUTPUT: about half zeros, every other one a -0.0
        pos = np.abs(bounded(rng, (K, M)))
        zero = np.where(rng.random((K, M)) < 0.5, f32(0.0), f32(-0.0))
        d["gout"] = np.where(rng.random((K, M)) < 0.5, pos, zero).astype(f32)
        d["outer_vec"], d["outer_w"] = draw(kind, rng, K, 4), draw(kind, rng, M, 4)
    else:
        d["gout"] = draw(kind, rng, (K, M))
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def wgrad_data(c, kind):
    return _wgrad_data(c["name"], kind)


@functools.lru_cache(maxsize=None)
def _wgrad_expect(name, kind):
    d = _wgrad_data(name, kind)
    out = wgrad(d["gout"], d["inp"], d["outer_vec"], d["outer_w"])
    for v in out:
        v.setflags(write=False)
    return out


def wgrad_expect(c, kind):
    """-> dW, db, tol dW, tol db of the case's own data (computed once)"""
    return _wgrad_expect(c["name"], kind)


# eight problems of different shapes: the one-tile "k64" between multi-tile ones, the bias-less "k63" and "k2049" between
# problems with a bias (their M dropped items in the reduce must not shift the neighbours), an outer form among them
MANY_SETS = {
    "one": ("k65",),
    "eight": ("k65", "k64", "k512", "k63", "k2048", "outer-k65", "k2049", "k1"),
    "eight-reversed": ("k1", "k2049", "outer-k65", "k2048", "k63", "k512", "k64", "k65"),
    "cap-exact": ("cap-exact",),
    "cap-plus": ("cap-plus",),
}


# ------------------------------------------------------------------------------------------------ macjd_rowdot_io
ROWDOT_K = (4, 60, 64, 68, 1020, 1024)
ROWDOT_ROWS = (0, 1, 15, 16, 17, RED_CAP * 16, RED_CAP * 16 + 1)


def rowdot_c(K):
    return 4 * -(-K // 64) + 4 + 1


def rowdot(x, w, b=None):
    """-> y [n], tolerance [n] (float64)"""
    x64, w64 = np.asarray(x, f64), np.asarray(w, f64)
    b64 = 0.0 if b is None else float(np.asarray(b, f64).reshape(-1)[0])
    return x64 @ w64 + b64, gamma(rowdot_c(x64.shape[1])) * (np.abs(x64) @ np.abs(w64) + abs(b64))


def _rc(name, rows, K, x_ld="min", x_off=0, w_off=0, bias=True):
    return dict(name=name, rows=rows, K=K, x_ld=x_ld, x_off=x_off, w_off=w_off, bias=bias)


ROWDOT_LAYOUTS = {       # name -> (x_ld mode, x_off, w_off, takes the 16-byte loads)
    "vec": ("min", 0, 0, True), "vec-gaps": ("pad4", 0, 0, True), "ld-odd": ("odd", 0, 0, False), "ld-even": ("even", 0, 0, False),
    "x-off": ("pad4", 1, 0, False), "w-off": ("min", 0, 1, False),
}


def rowdot_cases():
    """K around the 64-column pass (one pass of the 16 lanes of a row) and at the limit, in every layout; row counts around
    the 16 rows of a workgroup and around the 8192 workgroups of the capped grid, on the vector and the scalar path."""
    c = []
    for i, K in enumerate(ROWDOT_K):
        for j, (lay, (x_ld, x_off, w_off, _)) in enumerate(ROWDOT_LAYOUTS.items()):
            c.append(_rc(f"k{K}-{lay}", 17, K, x_ld, x_off, w_off, bias=(i + j) % 2 == 0))
    for i, rows in enumerate(ROWDOT_ROWS):
        c.append(_rc(f"rows{rows}-vec", rows, 68 if rows < 100 else 4, "pad4", bias=i % 2 == 0))
        c.append(_rc(f"rows{rows}-scalar", rows, 68 if rows < 100 else 4, "odd", x_off=1, bias=i % 2 == 1))
    return c


def rowdot_case(name):
    return next(c for c in rowdot_cases() if c["name"] == name)


def rowdot_vec(c):
    """whether the contract's 16-byte loads apply: x rows and w 16-byte aligned"""
    return ld_of(c["K"], c["x_ld"]) % 4 == 0 and c["x_off"] % 4 == 0 and c["w_off"] % 4 == 0


@functools.lru_cache(maxsize=None)
def _rowdot_data(name, kind):
    c = rowdot_case(name)
    rng = _rng("rowdot", name, kind)
    d = dict(x=draw(kind, rng, (c["rows"], c["K"])), w=draw(kind, rng, c["K"]), b=draw(kind, rng, 1) if c["bias"] else None)
    return d


def rowdot_data(c, kind):
    return _rowdot_data(c["name"], kind)


def rowdot_expect(c, kind):
    d = rowdot_data(c, kind)
    return rowdot(d["x"], d["w"], d["b"])


# ------------------------------------------------------------------------------------------------ macjd_splitrelu_bwd_io
def splitrelu(M, widths, Cp, act, g, outer_w, g_pass):
    """float32, the header's expression: g[k] None counts as zero; outer_w[k] given: g[k] is [M] and block k's gradient is
    g[k][m] * outer_w[k][c]; g_pass None counts as zero.  -> gout [M, Cr + Cp] float32"""
    Cr = int(sum(widths))
    out = np.zeros((M, Cr + Cp), f32)
    start = 0
    for k, w in enumerate(widths):
        if g[k] is None:
            gv = np.zeros((M, w), f32)
        elif outer_w[k] is not None:
            gv = (np.asarray(g[k], f32).reshape(M, 1) * np.asarray(outer_w[k], f32).reshape(1, w)).astype(f32)
        else:
            gv = np.asarray(g[k], f32).reshape(M, w)
        with np.errstate(invalid="ignore"):
            out[:, start:start + w] = np.where(np.asarray(act, f32)[:, start:start + w] > 0, gv, f32(0))
        start += w
    if Cp and g_pass is not None:
        out[:, Cr:] = np.asarray(g_pass, f32).reshape(M, Cp)
    return out


def _sc(name, M, widths, Cp=0, null=(), ow=(), gpass=True, special=False):
    return dict(name=name, M=M, widths=tuple(widths), Cp=Cp, null=tuple(null), ow=tuple(ow), gpass=gpass, special=special)


def splitrelu_cases():
    """null: blocks whose gradient is NULL; ow: blocks with an outer_w (their g is [M], g_ld = 1); gpass: g_pass given (it is
    ignored when Cp = 0); special: act carries +0.0, -0.0, the smallest normal and NaN.  Every row stride is padded."""
    return [
        _sc("b1-w1", 257, (1,)),                                               # M W = 257: the second workgroup's first item
        _sc("b1-ow", 7, (5,), Cp=3, ow=(0,)),
        _sc("b2", 7, (1, 6), Cp=2, ow=(1,), gpass=False),                      # Cp > 0 and g_pass NULL: zeros
        _sc("b3-null-first", 7, (4, 1, 3), Cp=1, null=(0,)),
        _sc("b4-null-inner", 7, (3, 1, 5, 2), Cp=4, null=(2,), ow=(1, 3)),
        _sc("b4-null-last", 7, (2, 7, 1, 4), null=(3,), gpass=False),          # Cp = 0, g_pass NULL
        _sc("b4-ow-all", 7, (6, 1, 2, 9), ow=(0, 1, 2, 3), special=True),      # Cp = 0, g_pass given: not read
        _sc("b4-ow-none", 7, (1, 1, 1, 1), Cp=5, special=True),
        _sc("m0", 0, (3, 2), Cp=2),
        _sc("m1", 1, (3, 2), Cp=2, ow=(0,), special=True),
        _sc("mw255", 15, (9, 4), Cp=4, ow=(1,)),                               # one short of a workgroup
        _sc("mw256", 16, (5, 5, 2), Cp=4, null=(1,)),                          # exactly one
        _sc("grid-cap", RED_CAP, (100, 1, 90, 33), Cp=32, ow=(0, 3)),          # M W = 8192 * 256: every workgroup once
        _sc("grid-cap-plus", 5419, (129, 64, 1, 130), Cp=63, null=(1,), ow=(2,)),   # 8192 * 256 + 1: workgroup 0 twice
    ]


def splitrelu_case(name):
    return next(c for c in splitrelu_cases() if c["name"] == name)


def splitrelu_strides(c):
    """-> g_ld per block, gp_ld, act_ld, gout_ld: every one padded"""
    Cr = sum(c["widths"])
    g_ld = [1 if k in c["ow"] else w + 1 + k for k, w in enumerate(c["widths"])]
    return g_ld, c["Cp"] + 2, Cr + 3, Cr + c["Cp"] + 1


SMALLEST_NORMAL = np.float32(2.0 ** -126)


@functools.lru_cache(maxsize=None)
def _splitrelu_data(name):
    c = splitrelu_case(name)
    rng = _rng("splitrelu", name)
    M, Cr = c["M"], sum(c["widths"])
    act = np.maximum(bounded(rng, (M, Cr)), f32(0))
    act = np.where((act == 0) & (rng.random((M, Cr)) < 0.5), f32(-0.0), act).astype(f32)
    if c["special"] and M:
        flat = act.reshape(-1)
        flat[:4] = [0.0, -0.0, SMALLEST_NORMAL, np.nan][:flat.size]
        flat[-1] = np.nan
    g, ow = [], []
    for k, w in enumerate(c["widths"]):
        g.append(None if k in c["null"] else bounded(rng, M if k in c["ow"] else (M, w)))
        ow.append(bounded(rng, w) if k in c["ow"] else None)
    g_pass = bounded(rng, (M, c["Cp"])) if c["gpass"] else None
    return dict(act=act, g=g, ow=ow, g_pass=g_pass)


def splitrelu_data(c):
    return _splitrelu_data(c["name"])


def splitrelu_expect(c):
    d = splitrelu_data(c)
    return splitrelu(c["M"], c["widths"], c["Cp"], d["act"], d["g"], d["ow"], d["g_pass"])
