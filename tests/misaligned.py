"""Device arrays at pointers that are aligned to their element type only (tests/test_gpu_alignment.py).

Every array of the GPU suite comes from ``DeviceArray.empty`` / ``from_host``: pool memory aligned to 256 bytes.  A caller of
the C ABI hands over ``DeviceArray.slab`` views of odd-N clouds, ``ptr + 12 * off`` and ``ptr + 4 * at`` (device.py, transforms.py,
models.py), Julia views and torch slices: pointers aligned to 4 bytes.  ``place`` builds such a pointer on purpose, inside a
buffer whose surroundings are filled so that a vector access running over the array's head or tail shows:

  inputs   float arrays between NaN words (0x7fc00000), index arrays between 0x7fffffff: a read past the array poisons the result
           or indexes far out of range;
  outputs  between 0xA5 bytes, and ``Placed.check_pads`` asserts after the call that both pads still hold them.

``fx`` is the package (or, in tests/test_misaligned_host.py, a stand-in with the same ``DeviceArray`` surface over host memory).
"""
import numpy as np

OFFSETS = (0, 4, 8, 12)
PAD = 64
NAN_WORD = 0x7FC00000
INDEX_WORD = 0x7FFFFFFF
OUTPUT_BYTE = 0xA5


def _fill(total, kind):
    """`total` bytes of the pad pattern of `kind`, laid on the buffer's own 4-byte grid."""
    if kind == "output":
        return np.full(total, OUTPUT_BYTE, np.uint8)
    word = NAN_WORD if kind == "float" else INDEX_WORD
    return np.full((total + 3) // 4, word, np.uint32).view(np.uint8)[:total].copy()


class Placed:
    """One array placed at ``base + pad + offset``.  ``arr`` is the non-owning DeviceArray handed to the call (it keeps ``buf``
    alive), ``ptr`` its address."""

    def __init__(self, buf, arr, offset, pad, kind):
        self.buf, self.arr, self.offset, self.pad, self.kind = buf, arr, offset, pad, kind

    @property
    def ptr(self):
        return self.arr.ptr

    @property
    def lo(self):
        return self.pad + self.offset

    @property
    def hi(self):
        return self.lo + self.arr.nbytes

    def to_host(self):
        return self.arr.to_host()

    def touched(self):
        """Byte positions, relative to the array's first byte (negative: the head pad; >= nbytes: the tail pad), where a
        pad no longer holds its pattern."""
        img = np.asarray(self.buf.to_host()).reshape(-1).view(np.uint8)
        want = _fill(img.size, self.kind)
        bad = np.flatnonzero(img != want)
        bad = bad[(bad < self.lo) | (bad >= self.hi)]
        return bad - self.lo

    def check_pads(self, what=""):
        bad = self.touched()
        assert bad.size == 0, (f"{what}: {bad.size} pad bytes written around an array of {self.arr.nbytes} bytes at offset "
                               f"{self.offset}; first at byte {int(bad[0])}, last at byte {int(bad[-1])} relative to the array")


def place(fx, host_array, offset, pad=PAD, output=False):
    """``host_array`` on the device at ``base + pad + offset`` of a buffer of ``nbytes + 2 * pad + 16`` bytes (``base`` aligned to
    256 bytes, ``offset`` in {0, 4, 8, 12}).  ``output``: the array is written by the call -- 0xA5 pads, checked by
    ``Placed.check_pads``; its initial contents are still ``host_array``'s (an accumulating or in-place call reads them)."""
    assert offset in OFFSETS, offset
    assert pad >= 16 and pad % 16 == 0, pad
    host = np.asfortranarray(host_array)
    assert host.dtype.itemsize <= 4 or offset % host.dtype.itemsize == 0, "an array is placed at its element type's alignment"
    kind = "output" if output else ("float" if host.dtype.kind == "f" else "index")
    total = host.nbytes + 2 * pad + 16
    img = _fill(total, kind)
    img[pad + offset:pad + offset + host.nbytes] = host.reshape(-1, order="F").view(np.uint8)
    buf = fx.DeviceArray.empty((total,), np.uint8)
    assert buf.ptr % 256 == 0, hex(buf.ptr)
    buf.copy_(img)
    arr = fx.DeviceArray(buf.ptr + pad + offset, host.shape, host.dtype, owned=False, keep=buf)
    return Placed(buf, arr, offset, pad, kind)


def cases(args):
    """The pointer patterns of one test, as {argument name: offset}: each array argument alone at offset 4 with the others
    aligned, then all of them together at 4, 8 and 12."""
    args = list(args)
    out = [{a: (4 if a == one else 0) for a in args} for one in args]
    out += [{a: off for a in args} for off in (4, 8, 12)]
    return [c for i, c in enumerate(out) if c not in out[:i]]  # (one argument: "alone at 4" is "all at 4")


def case_id(case):
    offs = sorted(set(case.values()))
    if offs == [0, 4] and list(case.values()).count(4) == 1:
        return next(a for a, o in case.items() if o == 4) + "+4"
    return "all+%d" % offs[-1] if offs else "none"
