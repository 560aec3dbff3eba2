"""Placement and checking helper of the bounds suite (bounds_cases.py, test_bounds_cpu.py, test_bounds_gpu.py).

An Arena lays the tensors of ONE call of an entry point out in ONE flat byte buffer -- numpy on the CPU (the host twins
and the helper's own tests), a torch uint8 tensor on a device -- so that what lies beside every tensor is known:

    front guard | tensor | back guard | front guard | next tensor | back guard | ...

Rules
  * Guard size.  Every guard is at least one full row-block of the tensor it protects -- innermost two extents x item
    size, a whole [W][D] slab of a volume, a whole map of an [H][W] image -- and never less than 4 KiB (MIN_GUARD).
    A kernel that is one tile, one row or one hypothesis slot off therefore lands in a guard, not in the next tensor.
  * Contents.  The whole buffer is filled with a seeded byte pattern, then the inputs are copied in; outputs keep the
    pattern (the prefill), so an element the call never writes is visible.  Two kinds of pattern, by the seed's parity:
        even seed  (k * 167 + seed) & 0x7F          every byte below 0x80, neighbours differ
        odd seed   every byte at or above 0x80, bytes 3 and 7 of every aligned 8 equal to 0xFF and byte 6 at or above
                   0xF0: every aligned float32 and float64 word is a NaN, every uint8 is high, every int32 negative
    The two patterns differ in EVERY byte.  SEEDS holds one of each; every case runs under both and the caller
    compares the outputs bit for bit: a result that a guard byte or a stale output byte reached differs.
  * Tensor start.  A tensor starts at its natural alignment and at nothing coarser: the offset from the 256-byte
    aligned base is a multiple of the item size and an ODD multiple of it modulo 16 (1, 3, 5.. for bytes, 4 or 12
    for 4-byte items, 8 for 8-byte items).  align=N asks for a coarser start for an entry whose header states one.
  * Batches.  A tensor given with `stride` (ELEMENTS between consecutive maps of its leading axis, 0 = dense) has
    the gaps between its maps filled and checked like guards.
  * check() asserts, on the device for torch, that every byte outside the outputs -- guards, gaps and inputs -- is
    what it was before the call, names the first region that is not, and returns the outputs as numpy arrays.
    In-place tensors (inout) are outputs: their gaps and guards are still held.
  * Deferred inputs (tests/test_stream_order_gpu.py).  build(deferred=True) makes two images of the buffer.  `buf`
    holds the DECOY image when build returns: the pattern everywhere, and in every in / inout tensor a decoy of its
    data that stays inside the tensor's domain -- uint8 and floating data reversed in flat order (the same multiset of
    values), int32 data (arm maps, arm volumes, integer disparities: upper bounds of walks) all equal to the tensor's
    own minimum; a name in `keep` keeps its data, one in `decoys` gets the array given there.  The TRUE image, what
    build() makes otherwise, waits in a second tensor of the same kind; arrive() copies it over the whole of buf --
    outputs and guards included -- with
    buf.copy_(true, non_blocking=True): on a device, one device-to-device copy on torch's current stream.  A call
    that reads before arrive() computes from decoys, one that writes before it has its output overwritten by the
    prefill; check() and initial() refer to the true image.  decoyed() names the tensors whose decoy differs.
"""
import ctypes as C

import numpy as np

MIN_GUARD = 4096
SEEDS = (0x2A, 0xD5)
BASE_ALIGN = 256


def pattern(n, seed, start=0):
    """n pattern bytes for buffer offsets start .. start + n"""
    k = np.arange(start, start + n, dtype=np.int64)
    h = (k * 167 + seed) & 0xFF
    if seed % 2 == 0:
        return (h & 0x7F).astype(np.uint8)
    out = 0x80 | (h & 0x3F)
    out = np.where(k % 8 == 6, 0xF0 | (h & 0x0F), out)
    out = np.where(k % 4 == 3, 0xFF, out)
    return out.astype(np.uint8)


assert all((pattern(64, SEEDS[0]) != pattern(64, SEEDS[1])).tolist())
assert np.isnan(pattern(64, SEEDS[1]).view(np.float32)).all() and np.isnan(pattern(64, SEEDS[1]).view(np.float64)).all()


class _T:
    __slots__ = ("name", "role", "shape", "dtype", "stride", "data", "off", "span", "align", "guard")


class Arena:
    def __init__(self, seed, device=None):
        """device None: numpy (host pointers); else a torch device"""
        self.seed, self.device = int(seed), device
        self._t, self._order, self.buf = {}, [], None
        self.extra = {}                 # what a call copies back from buffers the library owns, by name

    # ---- declaration -------------------------------------------------------------------------------------------
    def _add(self, name, role, shape, dtype, data, stride, align):
        assert self.buf is None and name not in self._t
        t = _T()
        t.name, t.role, t.shape, t.dtype = name, role, tuple(int(s) for s in shape), np.dtype(dtype)
        inner = int(np.prod(t.shape[1:])) if stride else 0
        assert stride == 0 or (len(t.shape) >= 2 and stride >= inner), (name, stride, inner)
        t.stride = int(stride)
        n = int(np.prod(t.shape))
        t.span = ((t.shape[0] - 1) * t.stride + inner if stride else n) * t.dtype.itemsize
        t.data = None if data is None else np.ascontiguousarray(data, t.dtype).reshape(t.shape).copy()
        t.align = int(align or 0)
        t.guard = max(MIN_GUARD, int(np.prod(t.shape[-2:])) * t.dtype.itemsize)
        self._t[name] = t
        self._order.append(name)
        return name

    def inp(self, name, data, stride=0, align=0):
        data = np.asarray(data)
        return self._add(name, "in", data.shape, data.dtype, data, stride, align)

    def out(self, name, shape, dtype, stride=0, align=0):
        return self._add(name, "out", shape, dtype, None, stride, align)

    def inout(self, name, data, stride=0, align=0):
        data = np.asarray(data)
        return self._add(name, "inout", data.shape, data.dtype, data, stride, align)

    # ---- layout ------------------------------------------------------------------------------------------------
    def _maps(self, t):
        """(byte offset, bytes) of every contiguous piece of t"""
        if not t.stride:
            return [(t.off, t.span)]
        inner = int(np.prod(t.shape[1:])) * t.dtype.itemsize
        return [(t.off + b * t.stride * t.dtype.itemsize, inner) for b in range(t.shape[0])]

    def _decoy(self, t):
        """the decoy of t's data: same shape and dtype, inside the tensor's domain"""
        if t.name in self._own_decoy:
            d = np.ascontiguousarray(self._own_decoy[t.name], t.dtype)
            assert d.shape == t.shape, (t.name, d.shape, t.shape)
            return d
        if t.dtype == np.int32:
            return np.full_like(t.data, t.data.min())
        assert t.dtype == np.uint8 or t.dtype.kind == "f", (t.name, t.dtype)
        return np.ascontiguousarray(t.data.reshape(-1)[::-1]).reshape(t.shape)

    def _fill(self, host, decoy):
        for t in self._t.values():
            if t.data is None:
                continue
            data = self._decoy(t) if decoy and t.name not in self._keep_true else t.data
            for b, (off, nb) in enumerate(self._maps(t)):
                src = data[b] if t.stride else data
                host[off:off + nb] = np.ascontiguousarray(src).view(np.uint8).reshape(-1)

    def build(self, deferred=False, keep=(), decoys=None):
        """deferred: buf holds the decoy image until arrive(); keep: inputs that keep their data in the decoy image;
        decoys: {name: array} for inputs whose decoy the caller states instead of the rule (the caller answers for its
        domain)"""
        self.deferred, self._keep_true, self._own_decoy = bool(deferred), frozenset(keep), dict(decoys or {})
        assert set(self._own_decoy) <= set(self._t), sorted(set(self._own_decoy) - set(self._t))
        assert self._keep_true <= set(self._t), sorted(self._keep_true - set(self._t))
        cur = 0
        for k, name in enumerate(self._order):
            t = self._t[name]
            isz = t.dtype.itemsize
            cur += t.guard
            if t.align:
                cur = -(-cur // t.align) * t.align
            else:
                cur = -(-cur // 16) * 16 + (isz * (1 + 2 * (k % 2))) % 16
                assert cur % isz == 0 and ((cur % 16) // isz) % 2 == 1
            t.off = cur
            cur += t.span + t.guard
        self.nbytes = cur
        raw = np.empty(cur + BASE_ALIGN, np.uint8)
        shift = (-raw.ctypes.data) % BASE_ALIGN
        host = raw[shift:shift + cur]
        host[:] = pattern(cur, self.seed)
        written = np.zeros(cur, bool)              # bytes the call may change
        for t in self._t.values():
            for off, nb in self._maps(t):
                if t.role != "in":
                    written[off:off + nb] = True
        true = None
        if deferred:
            true = host.copy()
            self._fill(true, decoy=False)
        self._fill(host, decoy=deferred)           # what buf holds when build returns
        if self.device is None:
            self.buf, self._keep = host, raw
            self._init, self._held = (true if deferred else host.copy()), ~written
            self.base = host.ctypes.data
        else:
            import torch
            self.buf = torch.from_numpy(host.copy()).to(self.device)
            self._init = torch.from_numpy(true).to(self.device) if deferred else self.buf.clone()
            self._held = torch.from_numpy(~written).to(self.device)
            self.base = self.buf.data_ptr()
            if deferred:
                torch.cuda.synchronize(self.device)
        assert self.base % BASE_ALIGN == 0
        return self

    def arrive(self):
        """the true image over the whole of buf, outputs and guards included; on a device asynchronously, on torch's
        current stream"""
        assert self.deferred
        if self.device is None:
            self.buf[:] = self._init
        else:
            self.buf.copy_(self._init, non_blocking=True)

    def decoyed(self):
        """the in / inout tensors whose decoy differs from their data (a one-element or constant tensor does not)"""
        if not self.deferred:
            return []
        return [t.name for t in self._t.values() if t.data is not None and t.name not in self._keep_true
                and not np.array_equal(self._decoy(t).view(np.uint8), t.data.view(np.uint8))]

    def addr(self, name):
        return self.base + self._t[name].off

    def ptr(self, name):
        """void* of the tensor; None (NULL) for name None"""
        return None if name is None else C.c_void_p(self.addr(name))

    def initial(self, name):
        """what the tensor held before the call: the data of an input, the prefill bytes of an output"""
        return self._read(name, self._init)

    # ---- after the call ----------------------------------------------------------------------------------------
    def _where(self, k):
        for t in self._t.values():
            if t.off - t.guard <= k < t.off:
                return f"front guard of {t.name}, {t.off - k} bytes before its start"
            if t.off + t.span <= k < t.off + t.span + t.guard:
                return f"back guard of {t.name}, {k - t.off - t.span} bytes past its end"
            if t.off <= k < t.off + t.span:
                for b, (off, nb) in enumerate(self._maps(t)):
                    if off <= k < off + nb:
                        return f"input {t.name}, map {b}, byte {k - off}"
                return f"batch gap of {t.name}, byte {k - t.off} of its span"
        return f"buffer offset {k}"

    def _read(self, name, buf):
        t = self._t[name]
        host = buf if self.device is None else None
        parts = []
        for off, nb in self._maps(t):
            piece = buf[off:off + nb]
            piece = piece.copy() if host is not None else piece.cpu().numpy()
            parts.append(piece)
        return np.concatenate(parts).view(t.dtype).reshape(t.shape)

    def check(self, buf=None):
        """-> {name: numpy array} of the outputs and in-place tensors, read from `buf` (default: the arena's buffer; a
        snapshot of it otherwise).  AssertionError names the first held byte that changed."""
        buf = self.buf if buf is None else buf
        assert buf.shape == self.buf.shape
        if self.device is None:
            bad = (buf != self._init) & self._held
            n = int(bad.sum())
            first = int(np.flatnonzero(bad)[0]) if n else -1
        else:
            import torch
            bad = (buf != self._init) & self._held          # on the device
            n = int(bad.sum().item())
            first = int(torch.nonzero(bad)[0].item()) if n else -1
        assert n == 0, f"{n} bytes outside the outputs changed; first: {self._where(first)}"
        return {name: self._read(name, buf) for name, t in self._t.items() if t.role != "in"}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_two_seeds(make, device=None, sync=None, deferred=False):
    """make(arena) declares the tensors of one call and returns call(arena) -> status.  Runs it under both seeds,
    check()s each, asserts the status is 0 and the outputs are bit-identical; -> (outputs, arena of the last seed).
    deferred: the arena holds decoys until call(arena) itself lets the inputs arrive()."""
    outs = []
    for seed in SEEDS:
        A = Arena(seed, device)
        call = make(A)
        A.build(deferred=deferred)
        rc = call(A)
        if sync is not None:
            sync()
        assert rc == 0, f"status {rc}"
        outs.append(A.check())
    for name in outs[0]:
        assert same_bytes(outs[0][name], outs[1][name]), (
            f"{name} depends on the prefill or on the guards: {int((outs[0][name].view(np.uint8) != outs[1][name].view(np.uint8)).sum())} "
            f"bytes differ between the two seeds")
    return outs[0], A
