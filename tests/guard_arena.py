"""A guarded arena for the raw C-ABI tests of the handle-less ops: every buffer an op is handed sits between two bands of a
known byte, at no better alignment than include/cotr_hip.h promises for that argument, and ``check()`` says afterwards
whether a band byte or an input byte changed.  The GPU sanitizers cannot be used on shared machines; this carries the same
question - does a kernel stay inside what it was given - with plain tensors.

An arena is one ``torch.uint8`` tensor on one device (``'cpu'`` works: tests/test_scratch_guard_cpu.py checks the arena
itself there).  Buffers are added by name and placed when ``build()`` is called:

    [front band | pad][buffer][rear band] [front band | pad][buffer][rear band] ...

* A buffer ends exactly where its rear band begins; the pad that brings its start to the wanted residue belongs to the
  front band.  The residues (``KINDS``) are the documented minimum and deliberately no more: scratch at 16 (mod 256), a
  ``double*`` at 8 (mod 16), ``float*`` / ``int32_t*`` at 4 (mod 8), ``uint8_t*`` at an odd address.  A kernel that
  quietly needs more than the header says meets an address that has no more.
* Each band is ``BAND`` = 64 KiB wide.  That is a condition, not a measurement: the widest store one workgroup of these
  kernels can make past an end is 1024 threads x 16 bytes = 16 KiB, and the band is four times that, so an overrun of a
  whole workgroup lands in the band and not in the neighbouring buffer.
* Bands, scratch and every output start as the byte ``fill``; an input starts as its data.  ``check()`` asserts that every
  band byte still is ``fill`` and that every input is byte-identical to what was uploaded; a failure names the buffer, the
  side and the first and last offending offsets.  Offsets are relative to the end of the buffer the band touches: a rear
  band's to the byte after the buffer's last one (0 is the first byte past the end), a front band's to the buffer's first
  byte (-1 is the byte before it).
* ``early_rear_band=k`` is a control: that buffer's rear band starts k bytes before the buffer's true end while callers still
  pass the true size on, so a kernel that writes the buffer in full must trip ``check()`` (offsets -k .. -1).  The whole
  buffer stays inside the arena."""
import ctypes

import numpy as np
import torch

BAND = 64 * 1024
# kind -> (residue, modulus) of the buffer's first byte
KINDS = {'scratch': (16, 256), 'f64': (8, 16), 'f32': (4, 8), 'i32': (4, 8), 'i64': (8, 16), 'u8': (1, 2),
         'a8': (8, 16), 'a16': (16, 32)}     # an argument of any type documented as 8- or as 16-byte aligned
NP_KIND = {np.dtype(np.float64): 'f64', np.dtype(np.float32): 'f32', np.dtype(np.int32): 'i32', np.dtype(np.int64): 'i64',
           np.dtype(np.uint64): 'i64', np.dtype(np.uint8): 'u8'}


class GuardError(AssertionError):
    pass


class _Buf:
    def __init__(self, name, nbytes, kind, data, early):
        self.name, self.nbytes, self.kind, self.data, self.early = name, int(nbytes), kind, data, int(early)
        self.front = self.start = self.rear = 0          # offsets in the arena: front band, buffer, rear band


class Arena:
    def __init__(self, device, fill):
        assert 0 <= fill <= 255
        self.device, self.fill = torch.device(device), int(fill)
        self.bufs, self.mem = {}, None

    # ---- registration ----------------------------------------------------------------------------------------------------
    def add(self, name, nbytes, kind, early_rear_band=0):
        """an output or scratch buffer of ``nbytes`` bytes (0 is allowed: it still has an address between two bands)"""
        assert self.mem is None and name not in self.bufs and kind in KINDS and 0 <= early_rear_band <= min(nbytes, BAND // 2)
        self.bufs[name] = _Buf(name, nbytes, kind, None, early_rear_band)
        return self

    def add_output(self, name, dtype, shape, early_rear_band=0, kind=None):
        dt = np.dtype(dtype)
        return self.add(name, int(np.prod(shape, dtype=np.int64)) * dt.itemsize, kind or NP_KIND[dt], early_rear_band)

    def add_input(self, name, array, kind=None):
        """``array``: a numpy array, uploaded as it is; ``check()`` compares its bytes afterwards"""
        a = np.ascontiguousarray(array)
        assert self.mem is None and name not in self.bufs
        self.bufs[name] = _Buf(name, a.nbytes, kind or NP_KIND[a.dtype], a, 0)
        return self

    # ---- placement -------------------------------------------------------------------------------------------------------
    def build(self):
        assert self.mem is None
        total = sum(b.nbytes + 2 * BAND + 256 for b in self.bufs.values()) + 256
        self.mem = torch.full((total,), self.fill, dtype=torch.uint8, device=self.device)
        base, cur = self.mem.data_ptr(), 0
        guard = np.zeros(total, dtype=bool)
        for b in self.bufs.values():
            res, mod = KINDS[b.kind]
            b.front = cur
            b.start = cur + BAND + (res - (base + cur + BAND)) % mod
            b.rear = b.start + b.nbytes - b.early
            cur = b.rear + BAND
            guard[b.front:b.start] = True
            guard[b.rear:cur] = True
            if b.data is not None:
                guard[b.start:b.start + b.nbytes] = True
                if b.nbytes:
                    self.mem[b.start:b.start + b.nbytes] = torch.from_numpy(b.data.reshape(-1).view(np.uint8)).to(self.device)
        assert cur <= total
        self.used = cur
        self._guard = torch.from_numpy(guard).to(self.device)
        self._want = self.mem.clone()
        return self

    def set_input(self, name, array):
        """after ``build()``: the bytes of an input that could not be known before (a table of device addresses taken from
        ``addr``); the input was added with a placeholder of the same size"""
        b = self.bufs[name]
        a = np.ascontiguousarray(array)
        assert self.mem is not None and b.data is not None and a.nbytes == b.nbytes
        b.data = a
        if b.nbytes:
            t = torch.from_numpy(a.reshape(-1).view(np.uint8)).to(self.device)
            self.mem[b.start:b.start + b.nbytes] = t
            self._want[b.start:b.start + b.nbytes] = t

    # ---- access ----------------------------------------------------------------------------------------------------------
    def addr(self, name):
        return self.mem.data_ptr() + self.bufs[name].start

    def ptr(self, name):
        return ctypes.c_void_p(self.addr(name))

    def nbytes(self, name):
        return self.bufs[name].nbytes

    def raw(self, name):
        """the buffer's bytes as a uint8 view of the arena"""
        b = self.bufs[name]
        return self.mem[b.start:b.start + b.nbytes]

    def view(self, name, dtype, shape):
        """the buffer's bytes as a host numpy array of ``dtype`` and ``shape`` (a copy: the buffer may sit at an address numpy
        and torch would not take for that type)"""
        host = self.raw(name).cpu().numpy().copy()
        return host.view(np.dtype(dtype)).reshape(shape)

    def poke(self, offset, value):
        """write one byte at an arena offset with a torch index assignment (the harness control)"""
        self.mem[offset] = value

    # ---- the check -------------------------------------------------------------------------------------------------------
    def check(self):
        """after a device synchronize: every band byte is ``fill`` and every input is what was uploaded, or GuardError"""
        bad = (self.mem != self._want) & self._guard
        if not bool(bad.any()):
            return
        idx = torch.nonzero(bad).reshape(-1).cpu().numpy()
        msgs = []
        for b in self.bufs.values():
            end = b.start + b.nbytes
            for side, lo, hi, origin in (('front', b.front, b.start, b.start), ('rear', b.rear, b.rear + BAND, end)):
                hit = idx[(idx >= lo) & (idx < hi)]
                if hit.size:
                    msgs.append(f"{side} band of '{b.name}' ({b.kind}, {b.nbytes} bytes): {hit.size} bytes are not fill 0x{self.fill:02X}, "
                                f'offsets {int(hit[0]) - origin} .. {int(hit[-1]) - origin} from the buffer\'s {"start" if side == "front" else "end"}')
            if b.data is not None:
                hit = idx[(idx >= b.start) & (idx < end)]
                if hit.size:
                    msgs.append(f"input '{b.name}' was modified: {hit.size} bytes differ, offsets {int(hit[0]) - b.start} .. {int(hit[-1]) - b.start}")
        raise GuardError('; '.join(msgs))

    def all_fill(self, name):
        """True when every byte of the buffer still is the fill"""
        return bool((self.raw(name) == self.fill).all())


def fill_value(fill, dtype):
    """the value a buffer element of ``dtype`` has when every byte of it is ``fill`` (as a numpy scalar array of size 1)"""
    dt = np.dtype(dtype)
    return np.full(dt.itemsize, fill, dtype=np.uint8).view(dt)[0]


def is_fill(array, fill):
    """elementwise: every byte of the element is ``fill`` (works where the fill is a NaN)"""
    a = np.ascontiguousarray(array)
    if a.size == 0:
        return np.ones(a.shape, dtype=bool)
    return (a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize) == fill).all(axis=1).reshape(a.shape)
