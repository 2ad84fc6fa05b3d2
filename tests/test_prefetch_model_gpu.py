"""``macjd_prefetch_batch`` / ``macjd_prefetch_batches`` (csrc/macjd_nets.hip ``prefetch_batch_kernel``) against
``gru_scan_model.prefetch_model`` — independent of the sibling launches, whose device functions it shares: the drawn
indices against the host mirror of the sampler (t mod N below the batch size), the counter (only read), the gathered
bytes with the pad bytes of a wider destination pitch surviving, the mask count exactly, h and P within the model's
tolerance rule.  Cases (gru_scan_model.PREFETCH_CASES): 1, 2 and 4 batches in one launch; B in {1, 2, 5}, J in {1, 3},
2, 4 and 5 scan steps; 1 (< B), 7, 8 and 9 stored episodes of a ring of 9; counter offsets 0 .. 3; "no draw" on some
batches only and on all; 1, 3, the default and more gather workgroups than row parts; rows of 4, 12, 16 and 48 bytes, the
16-byte multiples with aligned bases and 4 bytes off; 1 and 8 tensors; presets naming the last ring row; B = 1024; and
every refusal, with nothing written — among them outputs of two batches that overlap without sharing a base.

Tolerance: gru_scan_model's rule (floor 12.5 ulp = 1.49e-6 for h, 2 ulp for P; caps 1e-5 and 1e-6 + 1e-5 |P|).  Largest
|got - model| / tolerance on MI355X over all cases: h 0.133, P 0.193 (must be <= 1); the float32 restatement's largest
deviation is 1.3 % (h) and 1.0 % (P) of the cap.  The file runs in about 3 s.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import gru_scan_model as gm  # noqa: E402
from test_gru_scan_gpu import DEV, EINVAL, EUNSUPPORTED, OK, Slab, _lib, _ratio, _stream, _WORST, dense, strided  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENTINEL = -7777
GUARD = 64


class Bytes:
    """``n`` bytes, ``off`` bytes behind a 16-byte boundary, inside an allocation of known content with guards."""

    def __init__(self, n, off, rng, values=None):
        self.host = rng.integers(0, 256, size=2 * GUARD + off + n, dtype=np.uint8)
        self.base, self.n = GUARD + off, n
        if values is not None:
            self.host[self.base:self.base + n] = np.asarray(values, np.uint8).reshape(-1)
        self.t = torch.from_numpy(self.host).to(DEV)
        self.ptr = self.t.data_ptr() + self.base
        assert self.ptr % 16 == off % 16

    def got(self):
        return self.t.cpu().numpy()


class Shared:
    """What all batches of a launch share: the ring, the weights, the sampler's scalars."""

    def __init__(self, _native, key):
        self.case = next(c for c in gm.PREFETCH_CASES if c[0] == key)
        _, self.n, self.B, self.J, self.T1, self.N, self.slots, self.G, self.tensors, (self.S, self.Ah, self.A) = self.case
        self.d = d = gm.prefetch_case_data(key)
        self.rng = gm._rng("prefetch gpu", key)
        ring, w = d["ring"], d["w"]
        self.sj = self.S + 3
        self.sb = self.T1 * self.J * self.sj + 5
        self.obs, _ = strided(ring["obs"], (self.sb, self.J * self.sj, self.sj, 1), off=1)
        self.filled = torch.from_numpy(ring["filled"]).to(DEV)
        self.srcs = [Bytes(s.size, so, self.rng, s) for s, (_, _, so, _) in zip(ring["srcs"], self.tensors)]
        self.w = {k: dense(w[k]) for k in ("w_hh", "b_hh", "fc1_w", "fc1_b", "w_ih", "b_ih")}
        self.act = [(dense(ww), dense(bb, off=1)) for ww, bb in w["actor"]]
        self.n_stored = torch.tensor([-1, self.N, -1], dtype=torch.int32, device=DEV)
        self.counter = torch.tensor([-1, gm.PREFETCH_COUNTER, -1], dtype=torch.int64, device=DEV)

    def scalars_intact(self):
        return self.n_stored.cpu().tolist() == [-1, self.N, -1] and self.counter.cpu().tolist() == [-1, gm.PREFETCH_COUNTER, -1]


class Batch:
    """The outputs of one batch; ``slack``: every buffer twice as long as needed (refusal tests: an overlapping pointer
    still addresses memory that the test owns)."""

    def __init__(self, sh, i, slack=1):
        B, J, T1, A = sh.B, sh.J, sh.T1, sh.A
        self.h, self.p, self.tot = Slab(slack * B * T1 * J * 64), Slab(slack * B * J * A, off=1), Slab(slack)
        self.nh, self.np_ = B * T1 * J * 64, B * J * A
        self.idx = torch.full((2 * 32 + slack * B,), SENTINEL, dtype=torch.int64, device=DEV)
        self.idx[32:32 + B] = torch.tensor(sh.d["presets"][i], dtype=torch.int64)
        self.idx_ptr = self.idx.data_ptr() + 32 * 8
        self.dst = []
        for rb, pitch, _, do in sh.tensors:
            self.dst.append(Bytes(slack * B * (pitch or rb), do, sh.rng))

    def io(self, _native, sh, i):
        off, nd = sh.slots[i]
        io = _native.PrefetchIO()
        g = io.gru
        g.n_nets, g.B, g.T, g.J, g.H = 1, sh.B, sh.T1, sh.J, 64
        g.obs, g.obs_sb, g.obs_sj, g.S = sh.obs.ptr, sh.sb, sh.sj, sh.S
        g.w_hh[0], g.b_hh[0], g.fc1_w[0], g.fc1_b[0], g.w_ih[0], g.b_ih[0] = (
            sh.w[k].ptr for k in ("w_hh", "b_hh", "fc1_w", "fc1_b", "w_ih", "b_ih"))
        for l, (ww, bb) in enumerate(sh.act):
            g.act_w[0][l], g.act_b[0][l] = ww.ptr, bb.ptr
        g.Ah, g.A, g.h_out[0], g.p_out[0] = sh.Ah, sh.A, self.h.ptr, self.p.ptr
        ga = io.gather
        ga.n_tensors, ga.n_rows = len(sh.tensors), sh.B
        for k, (rb, pitch, _, _) in enumerate(sh.tensors):
            ga.src[k], ga.dst[k], ga.row_bytes[k], ga.dst_row_bytes[k] = sh.srcs[k].ptr, self.dst[k].ptr, rb, pitch
        sp = io.sampler
        sp.idx_out, sp.n, sp.reserved = self.idx_ptr, sh.B, off
        sp.n_stored, sp.counter, sp.seed = sh.n_stored[1:].data_ptr(), sh.counter[1:].data_ptr(), gm.PREFETCH_SEED
        m = io.mask
        m.B, m.Tm1, m.filled, m.f_sb, m.f_st = sh.B, sh.d["Tm1"], sh.filled.data_ptr(), sh.filled.stride(0), sh.filled.stride(1)
        io.tot_m, io.no_draw, io.gather_blocks = self.tot.ptr, nd, sh.G
        return io

    def untouched(self, sh, i):
        ok = self.h.rest_intact() and self.p.rest_intact() and self.tot.rest_intact()
        want = torch.full_like(self.idx, SENTINEL)
        want[32:32 + sh.B] = torch.tensor(sh.d["presets"][i], dtype=torch.int64)
        ok = ok and bool(torch.equal(self.idx, want))
        return ok and all(np.array_equal(b.got(), b.host) for b in self.dst)


def _ios(_native, sh, batches):
    arr = (_native.PrefetchIO * len(batches))()
    for i, b in enumerate(batches):
        arr[i] = b.io(_native, sh, i)
    return arr


@pytest.mark.parametrize("key", [c[0] for c in gm.PREFETCH_CASES])
def test_prefetch_against_the_model(key):
    _native, lib = _lib()
    sh = Shared(_native, key)
    assert lib.macjd_prefetch_batches_supported(1, 64, sh.B, sh.n) == 1
    batches = [Batch(sh, i) for i in range(sh.n)]
    arr = _ios(_native, sh, batches)
    if sh.n == 1:
        rc = lib.macjd_prefetch_batch(ctypes.byref(arr[0]), _stream())
    else:
        rc = lib.macjd_prefetch_batches(arr, sh.n, _stream())
    torch.cuda.synchronize()
    assert rc == OK
    assert sh.scalars_intact()                                   # the launch only reads the counter
    ring, w, Tm1 = sh.d["ring"], sh.d["w"], sh.d["Tm1"]
    for i, b in enumerate(batches):
        idx = sh.d["idx"][i]
        got_idx = b.idx.cpu().tolist()
        assert got_idx[32:32 + sh.B] == idx and set(got_idx[:32] + got_idx[32 + sh.B:]) == {SENTINEL}, (key, i)
        m64 = gm.prefetch_model(ring, idx, w, sh.T1, Tm1)
        m32 = gm.prefetch_model(ring, idx, w, sh.T1, Tm1, f32)
        rh = _ratio("prefetch h", b.h.read(), m64["h"], gm.tolerance("h", m64["h"], m32["h"])[0])
        rp = _ratio("prefetch P", b.p.read(), m64["P"], gm.tolerance("p", m64["P"], m32["P"])[0])
        assert b.h.rest_intact("all") and b.p.rest_intact("all")
        assert b.tot.read()[0] == float(m64["tot_m"]) and b.tot.rest_intact("all"), (key, i)
        for k, ((rb, pitch, _, _), dst, rows) in enumerate(zip(sh.tensors, b.dst, m64["rows"])):
            want = dst.host.copy()
            for r in range(sh.B):
                o = dst.base + r * (pitch or rb)
                want[o:o + rb] = rows[r]
            assert np.array_equal(dst.got(), want), (key, i, k)    # the rows, and pads / guards as they were
        print(key, i, "h", round(rh, 3), "P", round(rp, 3), "tot_m", m64["tot_m"])
    assert sh.obs.rest_intact() and all(np.array_equal(s.got(), s.host) for s in sh.srcs)
    print({k: round(v, 3) for k, v in _WORST.items() if k.startswith("prefetch")})


def test_batch_sizes_past_the_limit_are_unsupported():
    _native, lib = _lib()
    assert lib.macjd_prefetch_batch_supported(1, 64, 1024) == 1 and lib.macjd_prefetch_batch_supported(1, 64, 1025) == 0
    assert lib.macjd_prefetch_batch_supported(1, 64, 0) == 0 and lib.macjd_prefetch_batch_supported(2, 64, 4) == 0
    assert lib.macjd_prefetch_batch_supported(1, 128, 4) == 0
    assert lib.macjd_prefetch_batches_supported(1, 64, 4, 4) == 1 and lib.macjd_prefetch_batches_supported(1, 64, 4, 5) == 0
    assert lib.macjd_prefetch_batches_supported(1, 64, 4, 0) == 0


def _attempt(_native, lib, key, change, rc_want=EINVAL, n=None):
    """A valid launch of case ``key`` with one thing changed by ``change(ios)``: refused with rc_want, nothing written."""
    sh = Shared(_native, key)
    n = sh.n if n is None else n
    batches = [Batch(sh, i, slack=2) for i in range(sh.n)]
    arr = _ios(_native, sh, batches)
    what = change(arr, sh, batches)
    assert lib.macjd_prefetch_batches(arr, n, _stream()) == rc_want, what
    torch.cuda.synchronize()
    assert sh.scalars_intact() and all(b.untouched(sh, i) for i, b in enumerate(batches)), what


def test_refusals_of_one_batch():
    _native, lib = _lib()
    assert lib.macjd_prefetch_batches(None, 1, _stream()) == EINVAL and lib.macjd_prefetch_batch(None, _stream()) == EINVAL

    def field(path, value):
        def f(arr, sh, batches):
            o = arr[0]
            *head, last = path.split(".")
            for p in head:
                o = getattr(o, p)
            if "[" in last:
                name, k = last[:-1].split("[")
                a = getattr(o, name)
                if "," in k:
                    k0, k1 = (int(x) for x in k.split(","))
                    a[k0][k1] = value
                else:
                    a[int(k)] = value
            else:
                setattr(o, last, value)
            return (path, value)
        return f

    for path, value in (("gru.B", 1025), ("gru.B", 0), ("gru.n_nets", 2), ("gru.H", 128)):
        _attempt(_native, lib, "few", field(path, value), EUNSUPPORTED)
    changes = [("gru.T", 0), ("gru.J", 0), ("gru.obs", None), ("gru.S", 0), ("gru.S", 257), ("gru.Ah", 0), ("gru.Ah", 257),
               ("gru.A", 0), ("gru.A", 65), ("sampler.idx_out", None), ("sampler.n", 3), ("sampler.n_stored", None),
               ("sampler.counter", None), ("sampler.reserved", -1), ("gather.n_rows", 3), ("gather.n_tensors", 0),
               ("gather.n_tensors", 9), ("gather.src[2]", None), ("gather.dst[7]", None), ("gather.row_bytes[0]", 0),
               ("gather.row_bytes[1]", 6), ("gather.dst_row_bytes[1]", 22), ("gather.dst_row_bytes[1]", 8), ("mask.B", 3),
               ("mask.Tm1", 0), ("mask.filled", None), ("tot_m", None), ("gather_blocks", -1)]
    changes += [(f"gru.{n}[0]", None) for n in ("w_hh", "b_hh", "h_out", "p_out", "fc1_w", "fc1_b", "w_ih", "b_ih")]
    changes += [(f"gru.act_{wb}[0,{l}]", None) for wb in "wb" for l in range(3)]
    for path, value in changes:
        _attempt(_native, lib, "few", field(path, value))

    def misaligned(arr, sh, batches):
        arr[0].gru.w_hh[0] = arr[0].gru.w_hh[0] + 4
        return "w_hh + 4 bytes"
    _attempt(_native, lib, "few", misaligned)
    for n in (0, 5, -1):
        _attempt(_native, lib, "pair", lambda arr, sh, b: ("n", n), n=n)


def test_refusals_of_batches_that_differ_or_overlap():
    _native, lib = _lib()

    def differ(path, make):
        def f(arr, sh, batches):
            o = arr[1]
            *head, last = path.split(".")
            for p in head:
                o = getattr(o, p)
            if "[" in last:
                name, k = last[:-1].split("[")
                getattr(o, name)[int(k)] = make(getattr(o, name)[int(k)], sh)
            else:
                setattr(o, last, make(getattr(o, last), sh))
            return ("differs", path)
        return f

    # batch 1 differs from batch 0 in something the batches of a launch share (each value valid on its own)
    for path, make in (("gru.T", lambda v, sh: v - 1), ("gru.b_hh[0]", lambda v, sh: v + 4), ("gru.obs_sb", lambda v, sh: v - 1),
                       ("sampler.seed", lambda v, sh: v + 1), ("sampler.n_stored", lambda v, sh: sh.n_stored.data_ptr()),
                       ("sampler.counter", lambda v, sh: sh.counter.data_ptr()), ("mask.Tm1", lambda v, sh: v - 1),
                       ("mask.f_sb", lambda v, sh: v + 1), ("gather.n_tensors", lambda v, sh: v - 1),
                       ("gather.src[0]", lambda v, sh: v + 4), ("gather.row_bytes[3]", lambda v, sh: v - 4),
                       ("gather_blocks", lambda v, sh: v + 1)):
        _attempt(_native, lib, "pair", differ(path, make))

    # two batches share an output, or overlap without sharing its base (every pointer stays inside memory the test owns:
    # the buffers of these attempts are twice as long as a batch needs)
    def out(name, delta_of):
        def f(arr, sh, batches):
            b0 = arr[0]
            d = delta_of(sh)
            if name == "h_out":
                arr[1].gru.h_out[0] = b0.gru.h_out[0] + d
            elif name == "p_out":
                arr[1].gru.p_out[0] = b0.gru.p_out[0] + d
            elif name == "tot_m":
                arr[1].tot_m = b0.tot_m + d
            elif name == "idx_out":
                arr[1].sampler.idx_out = b0.sampler.idx_out + d
            elif name == "tot_m in h_out":
                arr[1].tot_m = b0.gru.h_out[0] + d
            elif name == "p_out in h_out":
                arr[1].gru.p_out[0] = b0.gru.h_out[0] + d
            else:
                k = int(name[3:])
                arr[1].gather.dst[k] = b0.gather.dst[k] + d
            return ("overlap", name, d)
        return f

    row_h = lambda sh: 4 * sh.T1 * sh.J * 64      # noqa: E731  one batch entry of h_out, in bytes
    for name, delta in (("h_out", lambda sh: 0), ("h_out", row_h), ("h_out", lambda sh: 4 * 64),
                        ("h_out", lambda sh: row_h(sh) * sh.B - 4), ("p_out", lambda sh: 0), ("p_out", lambda sh: 4 * sh.J * sh.A),
                        ("tot_m", lambda sh: 0), ("dst0", lambda sh: 0), ("dst3", lambda sh: 64), ("dst7", lambda sh: 52 * (sh.B - 1)),
                        ("dst1", lambda sh: 20 * (sh.B - 1) + 8), ("tot_m in h_out", lambda sh: 8), ("p_out in h_out", row_h)):
        _attempt(_native, lib, "pair", out(name, delta))
    # the drawn indices: "four7" draws in batches 1 .. 3 and reads batch 0's as found
    for a, b, delta in ((1, 2, 0), (1, 2, 8), (2, 3, 8), (0, 1, 0), (0, 2, 8)):
        def f(arr, sh, batches, a=a, b=b, delta=delta):
            arr[b].sampler.idx_out = arr[a].sampler.idx_out + delta
            return ("idx_out", a, b, delta)
        _attempt(_native, lib, "four7", f)


def test_two_batches_that_only_read_may_share_their_indices():
    """no_draw on both: idx_out is an input, and one tensor may serve both batches."""
    _native, lib = _lib()
    sh = Shared(_native, "last")
    batches = [Batch(sh, i) for i in range(2)]
    arr = _ios(_native, sh, batches)
    arr[1].sampler.idx_out = arr[0].sampler.idx_out
    assert lib.macjd_prefetch_batches(arr, 2, _stream()) == OK
    torch.cuda.synchronize()
    idx = sh.d["idx"][0]
    m64, m32 = (gm.prefetch_model(sh.d["ring"], idx, sh.d["w"], sh.T1, sh.d["Tm1"], dt) for dt in (f64, f32))
    for b in batches:
        _ratio("prefetch h", b.h.read(), m64["h"], gm.tolerance("h", m64["h"], m32["h"])[0])
        assert b.tot.read()[0] == float(m64["tot_m"])
    assert batches[0].idx.cpu().tolist()[32:32 + sh.B] == idx
