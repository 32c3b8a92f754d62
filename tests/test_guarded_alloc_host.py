"""The guarded, poisoning allocator of tests/guarded_alloc.py on the CPU: that it hands out what torch.empty would (shape, dtype,
contiguity, alignment), that its poison reads as NaN / -1 / 255, that ONE byte written one element outside a buffer is reported
with the allocation site, the side and the offset, and that it leaves torch exactly as it found it.  The stray writes below go
through the registry's own base block -- host memory this test owns -- with plain tensor indexing."""
import pytest
import torch

import guarded_alloc
from guarded_alloc import GuardViolation, guarded

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.uint8]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("shape", [(7,), (3, 5), (2, 1, 37, 53), (), (0, 3)], ids=str)
def test_shape_dtype_alignment_and_poison(shape, dtype):
    with guarded(device="cpu") as g:
        forms = [torch.empty(shape, dtype=dtype), torch.empty(*shape, dtype=dtype) if shape else torch.empty((), dtype=dtype),
                 torch.empty(size=shape, dtype=dtype, device="cpu"), torch.empty_like(torch.zeros(shape, dtype=dtype))]
        for t in forms:
            assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
            assert t.data_ptr() % 512 == 0
            if t.numel():          # (an empty tensor has no address to find its block by; its two guards are checked all the same)
                assert g.block_of(t) is not None and g.block_of(t).nbytes == t.numel() * t.element_size()
            if dtype.is_floating_point:
                assert bool(torch.isnan(t).all())
            elif dtype == torch.uint8:
                assert bool((t == 255).all())
            else:
                assert bool((t == -1).all())
        assert g.check() == len(forms)


def test_default_dtype_and_zero_mode():
    with guarded(device="cpu", fill="zeros") as g:
        t = torch.empty(4, 6)
        assert t.dtype == torch.get_default_dtype() and t.shape == (4, 6) and bool((t == 0).all())
        u = torch.empty_like(t, dtype=torch.int64)
        assert u.dtype == torch.int64 and bool((u == 0).all())
        t.fill_(3.0)
        g.repoison([t, {"u": u}, None])
        assert bool((t == 0).all())
    with guarded(device="cpu") as g:
        t = torch.empty(5, dtype=torch.float32)
        t.fill_(1.0)
        outside = torch.ones(9, dtype=torch.float64)          # not from this context: refilled over its own extent
        assert g.repoison({"a": t, "b": (outside,)}) == 2
        assert bool(torch.isnan(t).all()) and bool(torch.isnan(outside).all())
        g.check()


def test_guard_must_be_a_multiple_of_512():
    for bad in (0, 100, 513, -512):
        with pytest.raises(ValueError):
            guarded(device="cpu", guard=bad)
    with guarded(device="cpu", guard=512) as g:
        t = torch.empty(3, dtype=torch.float64)
        assert t.data_ptr() % 512 == 0 and g.block_of(t).base.numel() == 512 + 24 + 512


def test_writes_inside_the_buffer_pass():
    with guarded(device="cpu") as g:
        t = torch.empty((3, 11), dtype=torch.float32)
        t.copy_(torch.arange(33.0).view(3, 11))
        u = torch.empty(1, dtype=torch.uint8)
        u[0] = 7
        assert g.check() == 2
        assert g.release() == 2 and g.check() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.uint8], ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("side", ["before", "after"])
def test_one_stray_byte_is_reported(side, dtype):
    """One byte, one element in front of the interior or one element behind its last: check() names this file, the buffer's size, the
    side and the byte offset (from the buffer's start: negative in front of it, >= its size behind it)."""
    g = guarded(device="cpu")
    with pytest.raises(GuardViolation) as caught:
        with g:
            quiet = torch.empty(16, dtype=torch.float32)
            t = torch.empty((5, 3), dtype=dtype)          # the allocation site the report has to name
            site_line = _line_of("t = torch.empty((5, 3), dtype=dtype)")
            block = g.block_of(t)
            item, nbytes = t.element_size(), 15 * t.element_size()
            assert block.nbytes == nbytes and g.check() == 2
            offset = -item if side == "before" else nbytes + item - 1          # the first byte of the element in front / the last byte of the element behind
            block.base[block.guard + offset] = 0
    text = str(caught.value)
    assert text.count("\n") == 1, text          # the untouched block is not reported
    assert "test_guarded_alloc_host.py:%d" % site_line in text
    assert "buffer of %d bytes" % nbytes in text and ("written %s its range" % side) in text
    assert "1 guard bytes changed" in text and "byte offsets %d .. %d " % (offset, offset) in text
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE          # restored although the exit raised


def test_a_range_of_stray_bytes_reports_first_and_last():
    with pytest.raises(GuardViolation) as caught:
        with guarded(device="cpu", guard=1024) as g:
            t = torch.empty(100, dtype=torch.float32)
            block = g.block_of(t)
            block.base[block.guard + 400 + 8:block.guard + 400 + 40] = 0          # 32 bytes, 8 bytes behind the end
            block.base[block.guard - 1024] = 1                                        # and the very first guard byte
    text = str(caught.value)
    assert "byte offsets 408 .. 439 " in text and "32 guard bytes changed" in text and "written after" in text
    assert "byte offsets -1024 .. -1024 " in text and "written before" in text


def test_poison_valued_and_zero_stray_writes_are_both_seen():
    """The guard pattern is neither the poison nor zero: a kernel that spills NaN poison, or clears too much, changes it either way."""
    assert guarded_alloc.GUARD_BYTE not in (0, guarded_alloc.POISON_BYTE)
    pattern = torch.full((4,), guarded_alloc.GUARD_BYTE, dtype=torch.uint8)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        assert not bool(torch.isnan(pattern.view(dtype)).any())
    assert not bool(torch.isnan(torch.full((8,), guarded_alloc.GUARD_BYTE, dtype=torch.uint8).view(torch.float64)).any())
    for value in (0, 0xFF):
        with pytest.raises(GuardViolation):
            with guarded(device="cpu") as g:
                block = g.block_of(torch.empty(8, dtype=torch.float32))
                block.base[block.guard + 32] = value


REAL_EMPTY, REAL_EMPTY_LIKE = torch.empty, torch.empty_like


def _line_of(text):
    with open(__file__) as f:
        hits = [i + 1 for i, line in enumerate(f) if line.strip().startswith(text)]
    assert len(hits) == 1
    return hits[0]


def test_pass_through():
    with guarded(device="cpu") as g:
        out = torch.zeros(6)
        got = torch.empty(6, out=out)
        assert got is out and g.block_of(out) is None
        strided = torch.zeros(4, 6).t()
        like = torch.empty_like(strided)
        assert like.stride() == strided.stride() and g.block_of(like) is None
        cl = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last) and g.block_of(cl) is None
        leaf = torch.empty(3, requires_grad=True)
        assert leaf.requires_grad and g.block_of(leaf) is None
        flags = torch.empty(5, dtype=torch.bool)
        assert flags.dtype == torch.bool and g.block_of(flags) is None
        meta = torch.empty(5, device="meta")
        assert meta.device.type == "meta"
        # not touched at all: buffers the code fills on purpose stay filled
        assert bool((torch.zeros(5) == 0).all()) and bool((torch.full((5,), 2.0) == 2).all()) and bool((torch.ones(3).to(torch.float64) == 1).all())
        assert bool((torch.zeros_like(out) == 0).all())
        assert g.check() == 0
    # a context that selects another device leaves host allocations alone
    with guarded(device="cuda") as g:
        t = torch.empty(8)
        assert g.block_of(t) is None and g.check() == 0
    if torch.cuda.is_available():          # pinned host memory is not modelled either
        with guarded(device=["cpu", "cuda"]) as g:
            pinned = torch.empty(8, pin_memory=True)
            assert pinned.is_pinned() and g.block_of(pinned) is None


def test_nesting_and_exit_restore_the_originals():
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE and guarded_alloc.active() is None
    with guarded(device="cpu") as outer:
        outer_empty, outer_like = torch.empty, torch.empty_like
        assert outer_empty is not REAL_EMPTY and guarded_alloc.active() is outer
        with guarded(device="cpu", fill="zeros") as inner:
            assert torch.empty is not outer_empty and guarded_alloc.active() is inner
            t = torch.empty(3)
            assert bool((t == 0).all()) and inner.block_of(t) is not None
            # the inner context carves its block with the outer context's torch.empty: both see it, both check it
            assert len(outer.blocks) == 1 and outer.blocks[0].nbytes == 2 * inner.guard + 12
        assert torch.empty is outer_empty and torch.empty_like is outer_like and guarded_alloc.active() is outer
        assert bool(torch.isnan(torch.empty(2)).all())
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE and guarded_alloc.active() is None
    with pytest.raises(ZeroDivisionError):
        with guarded(device="cpu"):
            1 / 0
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE and guarded_alloc.active() is None


def test_autograd_function_site_is_the_caller_not_torch():
    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a):
            out = torch.empty_like(a)          # site: Twice
            out.copy_(2 * a)
            return out

        @staticmethod
        def backward(ctx, grad):
            return 2 * grad

    with guarded(device="cpu") as g:
        y = Twice.apply(torch.ones(3, requires_grad=True))
        assert bool((y == 2).all())
        (block,) = g.blocks
        assert block.site == "tests/test_guarded_alloc_host.py:%d" % _line_of("out = torch.empty_like(a)          # site: Twice")
