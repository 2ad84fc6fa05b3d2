"""Device buffers of the C-ABI tests that pin the rollout's agent launches: a typed allocation filled with a sentinel (NaN
for floats, -7777 for integers) between sentinel margins.  Inputs are put at element offsets (everything else keeps the
sentinel: the gaps of a padded layout); after a launch ``read`` returns values at offsets and ``rest_intact`` tells whether
every other element still holds its original bits — margins, gaps and rows past the end included."""
import numpy as np
import torch

MARGIN = 64
DEV = "cuda:0"
INT_FILL = -7777


class Slab:
    def __init__(self, n, off=0, dtype=np.float32):
        fill = np.nan if np.issubdtype(dtype, np.floating) else INT_FILL
        self.host = np.full(2 * MARGIN + off + n, fill, dtype)
        self.base, self.n, self.dtype = MARGIN + off, n, np.dtype(dtype)
        self.t = None

    def put(self, offsets, values):
        self.host[self.base + np.asarray(offsets).reshape(-1)] = np.asarray(values, self.dtype).reshape(-1)
        return self

    @property
    def ptr(self):
        if self.t is None:
            self.t = torch.from_numpy(self.host).to(DEV)
        return self.t.data_ptr() + self.dtype.itemsize * self.base

    def read(self, offsets=None):
        got = self.t.cpu().numpy()
        if offsets is None:
            return got[self.base:self.base + self.n]
        return got[self.base + np.asarray(offsets).reshape(-1)].reshape(np.shape(offsets))

    def rest_intact(self, offsets=None):
        """offsets None: nothing may have been written; "all": the n elements were; else: exactly these offsets."""
        bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[self.dtype.itemsize]
        got = self.t.cpu().numpy().view(bits)
        keep = np.ones(got.size, bool)
        if isinstance(offsets, str):
            keep[self.base:self.base + self.n] = False
        elif offsets is not None:
            keep[self.base + np.asarray(offsets).reshape(-1)] = False
        return bool(np.array_equal(got[keep], self.host.view(bits)[keep]))


def dense(values, off=0, dtype=np.float32):
    v = np.asarray(values, dtype)
    s = Slab(v.size, off, dtype)
    s.host[s.base:s.base + v.size] = v.reshape(-1)
    return s


def offsets(shape, strides):
    """Element offsets of an array of ``shape`` laid out with the given element strides."""
    o = np.zeros(shape, np.int64)
    for ax, s in enumerate(strides):
        sh = [1] * len(shape)
        sh[ax] = shape[ax]
        o = o + (np.arange(shape[ax]) * s).reshape(sh)
    return o


def strided(values, strides, off=0, dtype=np.float32):
    """values laid out with the given element strides -> (Slab, element offsets of every value)."""
    v = np.asarray(values, dtype)
    o = offsets(v.shape, strides)
    return Slab(int(o.max()) + 1, off, dtype).put(o, v), o


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream
