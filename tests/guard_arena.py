"""TEST INFRASTRUCTURE: guard-band arenas for the static entry points of include/cdvslam_hip.h.

The parity tests hand the library tensors that come out of torch's caching allocator: a store one row past the end, a
16-byte store over the end of a tile array or a load past the last pose lands in memory the process owns, nothing faults and
the rows a test looks at are right.  An Arena carves every tensor of one call out of ONE uint8 buffer, each tensor flush
between two guard bands:

    | guard | tensor 0 | guard | pad to 256 | tensor 1 | guard | ...

  * a tensor starts 256-byte aligned (what a fresh torch allocation has at the least) and its back guard starts at the byte
    after its last element, wherever that is (7 x f32 end 28 bytes in);
  * a guard is at least `row_bytes + 256` bytes and never below 4 KiB: one stray vector store and one stray row both land in it;
  * what a guard holds is chosen per tensor so that a stray READ can change a result but never an address:
        float / half tensors   pass A: a NaN with a payload (the sentinels of tests/stream_audit.py, the low nine bits
                               varied per tensor: no two of up to 512 tensors share a payload), pass B: zeros
        index tensors          pass A: 0, pass B: the largest index valid for that list (`index_max`)
        anything else (bytes)  pass A: 0xA5 varied per tensor (top bit always set), pass B: zeros
    never a huge or negative index: the audit makes strays visible, it cannot cause a fault;
  * check() asserts that every guard byte still holds what was written and names the tensor, the side and the distance of the
    first difference;
  * run_twice(fn) runs fn in a pass-A and a pass-B arena, checks both, and asserts that the outputs of the two passes are
    bit-identical -- a result that moved with the guard contents has read outside its arguments.

Works on device="cpu" (tests/test_guard_arena_cpu.py shows on numpy stand-ins that it rejects what it is meant to reject)."""
import numpy as np
import torch

ALIGN = 256
MIN_GUARD = 4096
F16_NAN = 0x7E5A            # tests/stream_audit.py CORR_SENTINEL
F32_NAN = 0x7FA5A5A5        # tests/stream_audit.py COORDS_SENTINEL
F64_NAN = 0x7FF8A5A5A5A5A5A5
BYTE_FILL = 0xA5

_FLOAT_NAN = {torch.float16: (np.uint16, F16_NAN), torch.float32: (np.uint32, F32_NAN), torch.float64: (np.uint64, F64_NAN)}
_INT = {torch.int64: np.int64, torch.int32: np.int32}
_NP2T = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
         np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8,
         np.dtype(np.bool_): torch.uint8}


def guard_bytes(row_bytes):
    """width of one guard band for a call whose widest output row has row_bytes bytes, a multiple of ALIGN"""
    g = max(int(row_bytes) + 256, MIN_GUARD)
    return (g + ALIGN - 1) // ALIGN * ALIGN


def guard_pattern(dtype, nbytes, which, index_max=0, salt=0):
    """the nbytes a guard of a `dtype` tensor holds in pass `which` ("A" / "B"), as a uint8 numpy array.  The pattern is laid
    from the START of the band in whole elements, so the front band of a tensor (which ends element-aligned at the tensor) and
    its back band (which starts element-aligned at the tensor's end) both read as whole elements next to the tensor.  `salt`
    (the tensor's number in its arena) varies the NaN payload (nine bits: the f16 NaN keeps its top mantissa bit) / fill
    byte, so that a kernel which COPIES one element too many from an input's guard into an output's guard does not write what
    is already there."""
    assert which in ("A", "B")
    out = np.zeros(nbytes, np.uint8)
    if dtype in _FLOAT_NAN:
        if which == "A":
            ut, bits = _FLOAT_NAN[dtype]
            n = nbytes // np.dtype(ut).itemsize
            out[: n * np.dtype(ut).itemsize] = np.full(n, bits ^ (salt & 0x1FF), ut).view(np.uint8)
    elif dtype in _INT:
        if which == "B":
            assert 0 <= int(index_max) < 2 ** 31, "index guards hold valid indices only"
            it = _INT[dtype]
            n = nbytes // np.dtype(it).itemsize
            out[: n * np.dtype(it).itemsize] = np.full(n, int(index_max), it).view(np.uint8)
    elif which == "A":
        out[:] = 0x80 | ((BYTE_FILL ^ salt) & 0x7F)
    return out


class GuardError(AssertionError):
    pass


class Arena:
    """see the module docstring.  Usage: a = Arena(dev, "A", row_bytes); x = a.tensor("x", array); ...; the call; a.check().
    The buffer is allocated up front (`capacity` bytes), so every view is valid as soon as tensor() returns it."""

    def __init__(self, device, which="A", row_bytes=0, capacity=1 << 22):
        self.device, self.which = torch.device(device), which
        self.guard = guard_bytes(row_bytes)
        self.buf = torch.zeros(int(capacity), dtype=torch.uint8, device=self.device)
        base = self.buf.data_ptr()
        self._skew = (-base) % ALIGN          # torch allocations are 256-aligned on the device; a CPU buffer need not be
        self._top = self._skew                # next free byte (ALIGN-aligned relative to the address)
        self.entries = []                     # (name, start, nbytes, dtype, front pattern, back pattern)

    def tensor(self, name, data, dtype=None, index_max=0, fill=None):
        """carve a tensor: `data` an array (copied in) or a shape (then filled with `fill`, default: left zero).  dtype: torch
        dtype (default: from the array).  index_max: for index tensors, the largest valid index of the list it points into."""
        if isinstance(data, (tuple, list, int)) and not isinstance(data, np.ndarray):
            shape = (data,) if isinstance(data, int) else tuple(int(s) for s in data)
            arr = None
            assert dtype is not None
        else:
            arr = np.ascontiguousarray(data.detach().cpu().numpy() if torch.is_tensor(data) else data)
            shape = arr.shape
            dtype = dtype or _NP2T[arr.dtype]
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        g = self.guard
        start = self._top + g                                   # front guard [start - g, start), start is ALIGN-aligned
        end = start + nbytes
        top = self._skew + (end + g - self._skew + ALIGN - 1) // ALIGN * ALIGN
        if top > self.buf.numel():
            raise MemoryError("arena capacity %d too small for %s (%d bytes)" % (self.buf.numel(), name, nbytes))
        # the front band's pattern is laid so that whole elements END at the tensor: g is a multiple of 256, hence of 8
        front = guard_pattern(dtype, g, self.which, index_max, salt=len(self.entries))
        back = front.copy()
        self.buf[start - g:start] = torch.from_numpy(front).to(self.device)
        self.buf[end:end + g] = torch.from_numpy(back).to(self.device)
        view = self.buf[start:end].view(dtype).view(shape) if nbytes else torch.empty(shape, dtype=dtype, device=self.device)
        if arr is not None and nbytes:
            src = torch.from_numpy(arr.view(np.uint8) if arr.dtype == np.bool_ else arr)
            view.copy_(src.view(dtype) if src.dtype != dtype else src)
        elif fill is not None and nbytes:
            view.fill_(fill)
        self.entries.append((name, start, nbytes, dtype, front, back))
        self._top = top
        assert view.numel() == 0 or view.data_ptr() % ALIGN == 0
        return view

    def span(self, name):
        for e in self.entries:
            if e[0] == name:
                return e[1], e[1] + e[2]
        raise KeyError(name)

    def first_difference(self):
        """None, or (tensor name, "front" / "back", distance in bytes from the tensor, byte found, byte expected) of the first
        guard byte (in address order) that no longer holds what was written"""
        host = self.buf.cpu().numpy()
        g = self.guard
        for name, start, nbytes, _, front, back in self.entries:
            d = np.nonzero(host[start - g:start] != front)[0]
            if d.size:
                i = int(d[-1])          # nearest to the tensor first: that is where an off-by-one lands
                return name, "front", g - i, int(host[start - g + i]), int(front[i])
            end = start + nbytes
            d = np.nonzero(host[end:end + g] != back)[0]
            if d.size:
                i = int(d[0])
                return name, "back", i + 1, int(host[end + i]), int(back[i])
        return None

    def check(self, what=""):
        d = self.first_difference()
        if d is not None:
            raise GuardError("%s: guard of tensor '%s' overwritten, %s side, %d byte(s) from the tensor (found 0x%02x, wrote 0x%02x) "
                             "[pass %s]" % (what or "arena", d[0], d[1], d[2], d[3], d[4], self.which))


def bits(t):
    """a tensor / array as raw bytes on the host, for bit-for-bit comparison (NaNs compare by payload)"""
    if torch.is_tensor(t):
        t = t.detach().contiguous().cpu()
        return t.view(torch.uint8).numpy().copy() if t.numel() else np.zeros(0, np.uint8)
    a = np.ascontiguousarray(t)
    return a.view(np.uint8).reshape(-1).copy()


def same_bits(a, b):
    a, b = bits(a).reshape(-1), bits(b).reshape(-1)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def run_twice(fn, device, row_bytes=0, capacity=1 << 22, what=""):
    """fn(arena) -> dict name -> tensor (outputs, read back after the call; fn synchronises nothing itself).  Runs it in a
    pass-A and a pass-B arena, checks the guards of both, asserts the outputs are bit-identical; returns pass A's outputs
    (host copies: torch CPU tensors)."""
    outs = []
    for which in ("A", "B"):
        a = Arena(device, which, row_bytes, capacity)
        o = fn(a)
        if a.device.type == "cuda":
            torch.cuda.synchronize(a.device)
        a.check("%s pass %s" % (what, which))
        outs.append({k: v.detach().cpu().clone() for k, v in o.items() if v is not None})
    assert outs[0].keys() == outs[1].keys()
    for k in outs[0]:
        if not same_bits(outs[0][k], outs[1][k]):
            x, y = bits(outs[0][k]), bits(outs[1][k])
            i = int(np.nonzero(x != y)[0][0])
            raise GuardError("%s: output '%s' differs between guard pass A and pass B (first at byte %d of %d): the call read "
                             "outside its arguments" % (what or "arena", k, i, x.size))
    return outs[0]
