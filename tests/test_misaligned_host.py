"""tests/misaligned.py against a stand-in allocator over host memory: the offsets, the pad bytes and the pad checker.  No device."""
import ctypes

import numpy as np
import pytest

import misaligned as mis


class _FakeArray:
    """The surface of DeviceArray that misaligned.py uses, over a host allocation aligned to 256 bytes."""

    def __init__(self, ptr, shape, dtype, owned=False, keep=None):
        self.ptr, self.shape, self.dtype, self._keep = ptr, tuple(int(s) for s in shape), np.dtype(dtype), keep

    @classmethod
    def empty(cls, shape, dtype=np.float32):
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        raw = np.zeros(n + 256, np.uint8)
        ptr = (raw.ctypes.data + 255) & ~255
        return cls(ptr, shape, dtype, keep=raw)

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    def copy_(self, host):
        host = np.asfortranarray(host, dtype=self.dtype)
        assert host.nbytes == self.nbytes
        ctypes.memmove(self.ptr, host.ctypes.data, self.nbytes)
        return self

    def to_host(self):
        out = np.empty(self.shape, self.dtype, order="F")
        ctypes.memmove(out.ctypes.data, self.ptr, self.nbytes)
        return out


class _FakeFx:
    DeviceArray = _FakeArray


def _poke(p, rel, value=0):
    """Write one byte at `rel` bytes from the placed array's first byte."""
    ctypes.c_uint8.from_address(p.ptr + rel).value = value


@pytest.mark.parametrize("offset", mis.OFFSETS)
@pytest.mark.parametrize("pad", [16, 64])
def test_place_offsets_contents_and_buffer_size(offset, pad):
    x = np.asfortranarray(np.arange(3 * 5 * 2, dtype=np.float32).reshape(3, 5, 2, order="F"))
    p = mis.place(_FakeFx, x, offset, pad=pad)
    assert p.buf.ptr % 256 == 0 and p.buf.nbytes == x.nbytes + 2 * pad + 16
    assert p.ptr == p.buf.ptr + pad + offset and p.ptr % 16 == offset and p.ptr % 4 == 0
    assert p.arr.shape == x.shape and p.arr.dtype == x.dtype and p.arr._keep is p.buf
    assert np.array_equal(p.to_host(), x)
    assert p.hi + (pad + 16 - offset) == p.buf.nbytes and pad + 16 - offset >= pad  # the tail pad is never shorter than `pad`


def test_place_rejects_offsets_off_the_element_grid():
    x = np.zeros(4, np.float32)
    for bad in (1, 2, 6, 16, -4):
        with pytest.raises(AssertionError):
            mis.place(_FakeFx, x, bad)
    with pytest.raises(AssertionError):
        mis.place(_FakeFx, np.zeros(4, np.float64), 4)  # an 8-byte element type is not placed at 4
    mis.place(_FakeFx, np.zeros(4, np.float64), 8)


@pytest.mark.parametrize("offset", mis.OFFSETS)
def test_pad_patterns(offset):
    f = mis.place(_FakeFx, np.ones((3, 7), np.float32), offset)
    img = f.buf.to_host()
    for lo, hi in ((0, f.lo), (f.hi, img.size)):
        words = img[lo:hi].view(np.uint32)
        assert np.all(words == mis.NAN_WORD) and np.all(np.isnan(words.view(np.float32)))
    i = mis.place(_FakeFx, np.zeros((3, 7), np.int32), offset)
    img = i.buf.to_host()
    assert np.all(img[:i.lo].view(np.int32) == 0x7FFFFFFF) and np.all(img[i.hi:].view(np.int32) == 0x7FFFFFFF)
    o = mis.place(_FakeFx, np.zeros((3, 7), np.float32), offset, output=True)
    img = o.buf.to_host()
    assert np.all(img[:o.lo] == 0xA5) and np.all(img[o.hi:] == 0xA5) and np.all(img[o.lo:o.hi] == 0)
    b = mis.place(_FakeFx, np.zeros(7, np.uint8), offset, output=True)  # a byte array (the normals' winner mask)
    assert b.hi - b.lo == 7 and b.touched().size == 0


@pytest.mark.parametrize("offset", mis.OFFSETS)
def test_checker_sees_every_pad_byte_and_nothing_inside(offset):
    x = np.zeros(10, np.float32)
    p = mis.place(_FakeFx, x, offset, output=True)
    p.check_pads()
    for rel in range(0, x.nbytes):  # writes inside the array are the call's business
        _poke(p, rel, 0x11)
    p.check_pads()
    total = p.buf.nbytes
    for rel in list(range(-p.lo, 0)) + list(range(x.nbytes, total - p.lo)):
        q = mis.place(_FakeFx, x, offset, output=True)
        _poke(q, rel, 0x00)
        assert list(q.touched()) == [rel]
        with pytest.raises(AssertionError, match="pad bytes written"):
            q.check_pads("probe")


def test_checker_catches_a_vector_store_running_over_head_or_tail():
    """The case the pads are for: a 16-byte store rounded down to its 16-byte line at the head, or started on the last element."""
    x = np.zeros(8, np.float32)
    p = mis.place(_FakeFx, x, 4, output=True)
    ctypes.memset(p.ptr - 4, 0, 16)            # the aligned line under the first element
    assert list(p.touched()) == [-4, -3, -2, -1]
    p = mis.place(_FakeFx, x, 12, output=True)
    ctypes.memset(p.ptr + x.nbytes - 4, 0, 16)  # a float4 store at the last element
    assert list(p.touched()) == list(range(x.nbytes, x.nbytes + 12))
    p = mis.place(_FakeFx, x, 8, output=True)
    ctypes.memset(p.ptr + x.nbytes, 0xA5, 16)   # writing the pattern itself cannot be seen; anything else is
    p.check_pads()


def test_cases_patterns():
    cs = mis.cases(["x", "y", "idx"])
    assert cs == [{"x": 4, "y": 0, "idx": 0}, {"x": 0, "y": 4, "idx": 0}, {"x": 0, "y": 0, "idx": 4},
                  {"x": 4, "y": 4, "idx": 4}, {"x": 8, "y": 8, "idx": 8}, {"x": 12, "y": 12, "idx": 12}]
    assert [mis.case_id(c) for c in cs] == ["x+4", "y+4", "idx+4", "all+4", "all+8", "all+12"]
    assert mis.cases(["x"]) == [{"x": 4}, {"x": 8}, {"x": 12}]
    assert [mis.case_id(c) for c in mis.cases(["x"])] == ["all+4", "all+8", "all+12"]
    assert mis.cases([]) == [{}] and mis.case_id({}) == "none"
