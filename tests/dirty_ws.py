"""Workspaces as a caller of the C ABI hands them over: recycled memory of exactly the queried size (tests/test_gpu_workspace.py).

The rest of the GPU suite takes its scratch from ``device.workspace`` (grow-only, at least 4096 bytes, fresh from the allocator
or left by the same entry point) or from ``DeviceArray.zeros``: contents always benign, size always generous.  ``Workspace``
places a buffer of EXACTLY ``nbytes`` bytes -- nothing rounded up, a 0-byte query is ``ptr`` None -- with ``misaligned.place``:
at a 256-byte aligned address between guard pads of 0xA5 bytes, GUARD bytes at least on each side (a layout that overruns does
so by a row, not a word), which ``check`` holds intact.  ``patterns`` then walks the fills, benign before adversarial:

  ZERO   0x00 bytes: what the suite ran on so far, the baseline;
  STALE  what the same entry point left in this very buffer after one run on OTHER inputs of the same shape (``prime``), with no
         refill: sums that are accumulated but never reset, counters that are not returned, "already built" flags;
  INF    32-bit words 0x7F800000: +Inf as Float32, an index of about 2.1e9 as int32, a finite 1e306 as Float64;
  ONES   0xFF bytes: NaN in both float widths, -1 as int32, 65535 as a 16-bit index.

``fx`` is the package (or, in tests/test_dirty_ws_host.py, a stand-in with the same ``DeviceArray`` surface over host memory)."""
import numpy as np

import misaligned as mis

PATTERNS = ("ZERO", "STALE", "INF", "ONES")
GUARD = 4096
INF_WORD = 0x7F800000
ALIGN = 256


def fill_bytes(nbytes, pattern):
    """The `nbytes` bytes of one of the filled patterns (STALE has none: it is what a run left)."""
    if pattern == "ZERO":
        return np.zeros(nbytes, np.uint8)
    if pattern == "ONES":
        return np.full(nbytes, 0xFF, np.uint8)
    assert pattern == "INF", pattern
    return np.full((nbytes + 3) // 4, INF_WORD, np.uint32).view(np.uint8)[:nbytes].copy()


def other_inputs(host):
    """"Other inputs of the same shape" for the run that primes STALE: a float array reversed end to end (points, channels and
    clouds change places; the multiset of values, and with it every size that depends on the data, stays), an index array as
    it is (it has to stay in range; tests/test_gpu_workspace.py reverses the order of face and edge lists on top, so that the
    builders that take nothing but indices get other inputs too)."""
    host = np.asfortranarray(host)
    if host.dtype.kind != "f":
        return host
    return np.asfortranarray(host.ravel(order="F")[::-1].reshape(host.shape, order="F"))


class Workspace:
    """`nbytes` bytes of scratch between guard pads.  ``ptr`` / ``nbytes`` are what the call gets."""

    def __init__(self, fx, nbytes, guard=GUARD):
        self.nbytes = int(nbytes)
        assert self.nbytes >= 0 and guard >= GUARD and guard % ALIGN == 0
        self.placed = mis.place(fx, np.zeros(self.nbytes, np.uint8), 0, pad=guard, output=True) if self.nbytes else None
        assert self.placed is None or (self.placed.ptr % ALIGN == 0 and self.placed.arr.nbytes == self.nbytes)

    @property
    def ptr(self):
        return self.placed.ptr if self.placed else None

    def fill(self, pattern):
        if self.placed:
            self.placed.arr.copy_(fill_bytes(self.nbytes, pattern))

    def image(self):
        """The workspace's bytes (what a refused call must leave as they were)."""
        return self.placed.to_host() if self.placed else np.zeros(0, np.uint8)

    def check(self, what=""):
        """No byte before `ptr` or at / after `ptr + nbytes` was written."""
        if self.placed:
            self.placed.check_pads(f"workspace of {self.nbytes} bytes, {what}")


def patterns(ws, prime):
    """Prepare `ws` for each pattern in turn and yield the pattern's name; the caller runs its call on `ws` at every step.
    STALE: ``prime()`` -- the same call on other inputs, on this buffer -- and nothing written afterwards."""
    for pattern in PATTERNS:
        if pattern == "STALE":
            prime()
        else:
            ws.fill(pattern)
        yield pattern
