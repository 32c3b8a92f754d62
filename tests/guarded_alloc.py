"""Test infrastructure: a guarded, poisoning stand-in for ``torch.empty`` / ``torch.empty_like``.

Every device buffer the library works in -- the network tape, the gradient workspaces, the loss-head, warp, augment, evaluate,
display and JPEG workspaces, every output tensor -- is allocated by the Python side with ``torch.empty`` and handed to the C ABI as
a pointer, sized by an ``endo_*_floats`` / ``endo_*_bytes`` query.  The ABI promises (include/endo_hip.h, "Workspace contract"):

  1. a call writes nothing outside the buffers it was given;
  2. a call does not depend on what a scratch or output buffer held on entry.

Neither is visible to an ordinary test: a stray write lands in some other live block of the caching allocator, and fresh or
recycled memory holds zeros or finite floats that a zero weight hides.  Inside ``with guarded():`` both become observable:

  * every ``torch.empty`` / ``torch.empty_like`` on the selected device is carved out of ONE uint8 block of
    ``guard + nbytes + guard`` bytes taken from the ordinary allocator; the caller gets a contiguous view of the interior.
    ``guard`` is a multiple of 512 bytes, the caching allocator's own granularity, so every pointer keeps the alignment it
    has in production and every ``% 16`` / ``% 4`` dispatch predicate of the library takes its production branch;
  * the guards hold the byte 0xA5 (not the poison, not zero, not a NaN in any float format); ``check()`` compares every guard
    byte, one device reduction per block, and names the allocation site, the side and the first and last offending offset;
  * the interior holds 0xFF bytes: NaN as fp32 / fp64 / fp16 / bf16, -1 as int32 / int64, 255 as uint8.  ``fill="zeros"`` gives
    the twin of a poisoned run that differs in nothing but the initial contents.

``torch.zeros`` / ``torch.full`` / ``.to()`` / ``.clone()`` are not touched: what the code fills on purpose stays filled.  Host and
pinned tensors, ``out=``, non-contiguous ``empty_like`` sources and everything else the replacement does not model go to the real
functions.  The module is a plain helper (no conftest, no plugin): it acts only inside its ``with`` block and puts the very same
function objects back on exit.
"""
import os
import sys

import torch

GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF
DEFAULT_GUARD = 64 * 1024          # a condition, not a measurement: an overrun starts at the buffer's edge
ALIGN = 512

_ITEMSIZE = {torch.float64: 8, torch.int64: 8, torch.float32: 4, torch.int32: 4, torch.float16: 2, torch.bfloat16: 2, torch.int16: 2,
             torch.uint8: 1, torch.int8: 1}          # the dtypes the replacement models; bool, complex, quantized go to the real function
_HERE = os.path.abspath(__file__)
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep

_active = []          # the stack of open contexts, innermost last


class GuardViolation(AssertionError):
    pass


class _Block(object):
    __slots__ = ("base", "guard", "nbytes", "site", "shape", "dtype", "ptr")

    def __init__(self, base, guard, nbytes, site, shape, dtype):
        self.base, self.guard, self.nbytes, self.site, self.shape, self.dtype = base, guard, nbytes, site, shape, dtype
        self.ptr = base.data_ptr() + guard

    def interior(self):
        return self.base[self.guard:self.guard + self.nbytes]


def _call_site():
    """file:line of the nearest caller outside this module and outside torch (autograd.Function.apply and the like)."""
    frame = sys._getframe(1)
    while frame is not None:
        name = os.path.abspath(frame.f_code.co_filename)
        if name != _HERE and not name.startswith(_TORCH_DIR):
            shown = os.path.relpath(name, _ROOT) if name.startswith(_ROOT + os.sep) else name
            return "%s:%d" % (shown, frame.f_lineno)
        frame = frame.f_back
    return "<unknown>"


def _default_device():
    return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")


class guarded(object):
    """``with guarded(device="cuda") as g:`` -- see the module docstring.  device: a device, a device type ("cuda" selects every
    GPU, "cuda:0" one) or a list of them.  guard: bytes on each side, a multiple of 512.  fill: "poison" (0xFF) or "zeros"."""

    def __init__(self, device="cuda", guard=DEFAULT_GUARD, fill="poison"):
        if guard <= 0 or guard % ALIGN:
            raise ValueError("guard must be a positive multiple of %d bytes" % ALIGN)
        if fill not in ("poison", "zeros"):
            raise ValueError("fill is 'poison' or 'zeros'")
        devices = device if isinstance(device, (list, tuple)) else [device]
        self.devices = [torch.device(d) for d in devices]
        self.guard, self.fill = int(guard), fill
        self.blocks = []
        self._by_ptr = {}
        self._saved = None

    # ---- context ------------------------------------------------------------------------------
    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("this guarded() context is already open")
        self._saved = (torch.empty, torch.empty_like)
        real_empty, real_empty_like = self._saved
        owner = self

        def empty(*size, **kw):
            return owner._empty(real_empty, size, kw)

        def empty_like(src, **kw):
            return owner._empty_like(real_empty, real_empty_like, src, kw)

        torch.empty, torch.empty_like = empty, empty_like
        _active.append(self)
        return self

    def __exit__(self, exc_type, exc, tb):
        torch.empty, torch.empty_like = self._saved
        self._saved = None
        _active.remove(self)
        if exc_type is None:
            self.check()
        else:
            try:
                self.check()
            except GuardViolation as violation:          # the body's own failure stands; say that the guards were hit as well
                sys.stderr.write("guarded_alloc: while handling %s: %s\n" % (exc_type.__name__, violation))
        return False

    # ---- the replacements ---------------------------------------------------------------------
    def _selected(self, device):
        for d in self.devices:
            if d.type == device.type and (d.index is None or device.index is None or d.index == device.index):
                return True
        return False

    def _empty(self, real_empty, size, kw):
        unknown = set(kw) - {"size", "dtype", "device", "layout", "requires_grad", "pin_memory", "memory_format"}
        if unknown or kw.get("pin_memory") or kw.get("requires_grad") or kw.get("layout", torch.strided) is not torch.strided \
                or kw.get("memory_format", torch.contiguous_format) is not torch.contiguous_format or ("size" in kw and size):
            return real_empty(*size, **kw)
        if "size" in kw:
            shape = kw["size"]
        elif len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            shape = size[0]
        else:
            shape = size
        try:
            shape = tuple(int(s) for s in shape)
        except (TypeError, ValueError):
            return real_empty(*size, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = torch.device(kw["device"]) if kw.get("device") is not None else _default_device()
        if dtype not in _ITEMSIZE or not self._selected(device) or any(s < 0 for s in shape):
            return real_empty(*size, **kw)
        return self._carve(real_empty, shape, dtype, device)

    def _empty_like(self, real_empty, real_empty_like, src, kw):
        unknown = set(kw) - {"dtype", "device", "layout", "requires_grad", "pin_memory", "memory_format"}
        if unknown or not isinstance(src, torch.Tensor) or kw.get("pin_memory") or kw.get("requires_grad") \
                or kw.get("layout", torch.strided) is not torch.strided or src.layout is not torch.strided \
                or kw.get("memory_format", torch.preserve_format) not in (torch.preserve_format, torch.contiguous_format) \
                or not src.is_contiguous():
            return real_empty_like(src, **kw)
        dtype = kw.get("dtype") or src.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else src.device
        if dtype not in _ITEMSIZE or not self._selected(device):
            return real_empty_like(src, **kw)
        return self._carve(real_empty, tuple(src.shape), dtype, device)

    def _carve(self, real_empty, shape, dtype, device):
        nbytes = _ITEMSIZE[dtype]
        for s in shape:
            nbytes *= s
        total = self.guard + nbytes + self.guard
        base = real_empty(total, dtype=torch.uint8, device=device)
        if base.data_ptr() % ALIGN:          # host memory only: the GPU's caching allocator hands out 512-byte-aligned blocks by itself
            raw = real_empty(total + ALIGN, dtype=torch.uint8, device=device)
            skip = (-raw.data_ptr()) % ALIGN
            base = raw[skip:skip + total]
        base[:self.guard].fill_(GUARD_BYTE)
        base[self.guard + nbytes:].fill_(GUARD_BYTE)
        base[self.guard:self.guard + nbytes].fill_(POISON_BYTE if self.fill == "poison" else 0)
        block = _Block(base, self.guard, nbytes, _call_site(), shape, dtype)
        self.blocks.append(block)
        self._by_ptr[(base.device, block.ptr)] = block          # (base.device: "cuda" has become "cuda:0")
        return block.interior().view(dtype).view(shape)

    # ---- registry -----------------------------------------------------------------------------
    def block_of(self, tensor):
        """The registry entry whose interior starts where ``tensor`` does, or None."""
        return self._by_ptr.get((tensor.device, tensor.data_ptr()))

    def check(self):
        """Every guard byte of every block, one device reduction per block; raises GuardViolation naming every block that was hit.
        Returns the number of blocks checked."""
        problems = []
        for block in self.blocks:
            g, n = block.guard, block.nbytes
            if int((torch.cat([block.base[:g], block.base[g + n:]]) != GUARD_BYTE).sum()) == 0:
                continue
            for side, part in (("before", block.base[:g]), ("after", block.base[g + n:])):
                bad = torch.nonzero(part != GUARD_BYTE).reshape(-1)
                if bad.numel() == 0:
                    continue
                first, last = int(bad[0]), int(bad[-1])
                if side == "before":
                    first, last = first - g, last - g          # relative to the buffer's first byte: -1 is the byte in front of it
                else:
                    first, last = first + n, last + n          # relative to the buffer's first byte: nbytes is the first byte behind it
                problems.append("%s: buffer of %d bytes (%s %s) was written %s its range: %d guard bytes changed, byte offsets %d .. %d from its start" % (
                    block.site, n, tuple(block.shape), str(block.dtype).replace("torch.", ""), side, int(bad.numel()), first, last))
        if problems:
            raise GuardViolation("guard bytes overwritten:\n  " + "\n  ".join(problems))
        return len(self.blocks)

    def release(self):
        """check(), then forget the blocks seen so far (their memory goes back to the allocator when their last view dies): keeps a
        long case from holding every tape it ever made."""
        count = self.check()
        self.blocks = []
        self._by_ptr = {}
        return count

    def repoison(self, what):
        """Refill cached workspaces -- a tensor, or any nesting of dicts / lists / tuples of tensors; None is skipped -- with this
        context's fill, so that the next call finds them as a first call would.  A tensor this context handed out is refilled over
        its whole interior; one allocated elsewhere over its own extent.  Returns the number of tensors refilled."""
        if what is None:
            return 0
        if isinstance(what, torch.Tensor):
            if not self._selected(what.device) or what.numel() == 0:
                return 0
            value = POISON_BYTE if self.fill == "poison" else 0
            block = self.block_of(what)
            if block is not None:
                block.interior().fill_(value)
            else:
                if not what.is_contiguous() or what.dtype not in _ITEMSIZE:
                    raise ValueError("repoison: cannot refill a non-contiguous tensor or one of dtype %s" % what.dtype)
                what.detach().reshape(-1).view(torch.uint8).fill_(value)
            return 1
        if isinstance(what, dict):
            what = list(what.values())
        return sum(self.repoison(item) for item in what)


def active():
    """The innermost open context, or None."""
    return _active[-1] if _active else None
