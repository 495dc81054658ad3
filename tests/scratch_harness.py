"""Poisoned, exact-size device scratch and poisoned outputs for the operators of kinectpy_amd.ops -- TEST INFRASTRUCTURE ONLY.

`scratch(pattern, exact=True, poison_outputs=False)` replaces kinectpy_amd._lib.workspace for the duration of a `with` block
("carved scratch"):

  * every hand-out returns ONE 256-byte-aligned base inside a buffer this module owns -- nested operators share it, as they share
    the real per-stream workspace;
  * with exact=True the size reported to the C entry point is exactly the `nbytes` the operator asked for (the real workspace
    never reports less than 1 MiB, so a short kpx_*_workspace_bytes answer lands in slack there); otherwise max(nbytes, 1 MiB);
  * before every hand-out [base, base + nbytes) is filled with `pattern` on the calling stream, and the GUARD bytes before the
    base and after base + nbytes with CANARY;
  * the guards of a hand-out are checked (after a stream synchronise) before the next hand-out repaints them, and on exit; the
    largest `nbytes` seen is kept for the report.  A damaged guard raises GuardError on exit.

Patterns: 0x00, 0xFF (NaN, -1, UINT_MAX, all-ones keys), 0x7F (large finite floats, large positive ints) and "leftover" (no
fill: the scratch holds what the previous call left, the guards are still painted).

poison_outputs=True also wraps torch.empty / torch.empty_like: a device result with numel() > 0 is filled bytewise with the
pattern before it is returned, so an output element the kernels skip shows as NaN / -1 and not as an allocator leftover.
(empty_like goes beyond the contract's torch.empty: ops.py makes some outputs with it.  Tensors made any other way -- torch.zeros,
new_empty, empty_strided -- are not poisoned: where ops.py hands a kernel a torch.zeros counter, as halfspace_select and slab_split
do, a kernel that relies on that zero is within its rights and outside what is tested here.)

No environment variable, no preload, nothing that outlives the `with` block.
"""
import contextlib
import ctypes as C

import torch

GUARD = 64 << 10
CANARY = 0xA5                       # differs from every fill pattern
PATTERNS = (0x00, 0xFF, 0x7F, "leftover")
ALIGN = 256
MIN_REAL = 1 << 20                  # what _lib.Workspace.get hands out at least
_real_empty, _real_empty_like = torch.empty, torch.empty_like


class GuardError(AssertionError):
    pass


class Arena:
    """The guarded region inside one uint8 tensor (device or host: the guard logic is the same and is tested on CPU tensors)."""

    def __init__(self, buf):
        assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous()
        self.buf = buf
        self.lo = GUARD + (-(buf.data_ptr() + GUARD)) % ALIGN          # offset of the base: GUARD bytes before it, aligned
        self.capacity = buf.numel() - self.lo - GUARD
        assert self.capacity >= 0, "buffer too small for two guards"
        self.base = buf.data_ptr() + self.lo

    def paint(self, nbytes, pattern):
        assert 0 <= nbytes <= self.capacity
        lo = self.lo
        self.buf[lo - GUARD:lo].fill_(CANARY)
        self.buf[lo + nbytes:lo + nbytes + GUARD].fill_(CANARY)
        if pattern != "leftover" and nbytes:
            self.buf[lo:lo + nbytes].fill_(int(pattern))

    def damage(self, nbytes):
        """-> list of (offset relative to the base, byte found) of the first damaged byte of each guard of a hand-out of nbytes"""
        lo, out = self.lo, []
        for start in (lo - GUARD, lo + nbytes):
            bad = torch.nonzero(self.buf[start:start + GUARD] != CANARY)
            if bad.numel():
                first = start + int(bad[0])
                out.append((first - lo, int(self.buf[first])))
        return out


class Scratch:
    def __init__(self, pattern, exact, capacity):
        assert pattern in PATTERNS, pattern
        self.pattern, self.exact, self.capacity = pattern, exact, capacity
        self.arena = None
        self.last = None                # nbytes of the hand-out whose guards stand unchecked
        self.largest = 0
        self.handouts = 0
        self.problems = []

    def _check_last(self):
        if self.last is not None and self.arena is not None:
            torch.cuda.current_stream().synchronize()
            for off, byte in self.arena.damage(self.last):
                self.problems.append(f"hand-out {self.handouts} of {self.last} bytes: guard byte at base{off:+d} is 0x{byte:02X}"
                                     + (f" ({off - self.last} past the end)" if off >= 0 else ""))
            self.last = None

    def workspace(self, nbytes):
        from kinectpy_amd import _lib
        nbytes = int(nbytes)
        self._check_last()
        if self.arena is None or nbytes > self.arena.capacity:
            # (a regrow moves the base: the default capacity holds every case of the registry, so it happens in no test)
            cap = max(self.capacity, 2 * nbytes)
            self.arena = Arena(_real_empty(cap + 2 * GUARD + ALIGN, dtype=torch.uint8, device=_lib.device()))
        self.arena.paint(nbytes, self.pattern)
        self.last, self.largest, self.handouts = nbytes, max(self.largest, nbytes), self.handouts + 1
        return C.c_void_p(self.arena.base), C.c_size_t(nbytes if self.exact else max(nbytes, MIN_REAL))

    def finish(self):
        self._check_last()
        if self.problems:
            raise GuardError("scratch guard damaged (largest hand-out %d bytes): %s" % (self.largest, "; ".join(self.problems)))


def _poisoned(real, pattern):
    def make(*args, **kwargs):
        t = real(*args, **kwargs)
        if t.is_cuda and t.numel() > 0 and t.is_contiguous():
            t.view(torch.uint8).fill_(pattern)
        return t
    make.__wrapped__ = real
    return make


@contextlib.contextmanager
def scratch(pattern, exact=True, poison_outputs=False, monkeypatch=None, capacity=128 << 20, state=None):
    """See the module docstring.  monkeypatch: pytest's fixture (the patches are also undone here, on every exit).  state: the
    Scratch of an earlier block, to go on with the same buffer ("leftover" after a larger case)."""
    from kinectpy_amd import _lib
    s = Scratch(pattern, exact, capacity)
    if state is not None:
        s.arena = state.arena
    saved = (_lib.workspace, torch.empty, torch.empty_like)
    setter = monkeypatch.setattr if monkeypatch is not None else setattr
    try:
        setter(_lib, "workspace", s.workspace)
        if poison_outputs and pattern != "leftover":
            setter(torch, "empty", _poisoned(_real_empty, int(pattern)))
            setter(torch, "empty_like", _poisoned(_real_empty_like, int(pattern)))
        yield s
        s.finish()
    finally:
        setattr(_lib, "workspace", saved[0])
        setattr(torch, "empty", saved[1])
        setattr(torch, "empty_like", saved[2])
