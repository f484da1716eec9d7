"""Poisoned engine buffers (test helper, GPU box).

An engine's `gradstate`, `workspace` and `workspace2` come from torch.empty: the library must give
the same results whatever they held before begin_epoch (include/flsim.h).  fill() writes
one 32-bit pattern over all of them, so a kernel that reads a float nothing wrote in the current
pass or epoch reads the pattern:

  ZERO   what a fresh process usually gets from the allocator (the baseline)
  QNAN   a quiet NaN with a payload: it survives every sum and product
  PI     finite and positive: it survives the `> 0` masks that turn a NaN (or a 0) into 0

The integer tensors of the workspace are then zeroed again for every pattern, so the pattern is
only ever read as a float value, never as a label or an index (nothing can index out of bounds
with it).  They are `y` and the max-pool argmax bytes: y i1 i2 i3 (PerformantNet1, WS in
csrc/pn1_net.hip) and y i1 i2 i4 i6 i8 (vgg11 / vgg11_bn, VWS in csrc/vgg_net.hip); every other
member of WS / VWS is a float tensor.  They are laid out one after another, so one range
[offset(y), offset(the tensor after the last i*)) covers them.  The gradstate's only integers are
the fused server step's tile counters, which begin_epoch clears: fill before begin_epoch.
"""
import ctypes

import torch

ZERO = 0x00000000
QNAN = 0x7FC12345        # the payload tests/test_gpu_optim.py uses
PI = 0x40490FDB
PATTERNS = {"zero": ZERO, "qnan": QNAN, "pi": PI}

# workspace ids (engine.WORKSPACE) of the integer tensors, first to last
INT_TENSORS = {"pn1": ("y", "i1", "i2", "i3"),
               "vgg11": ("y", "i1", "i2", "i4", "i6", "i8"),
               "vgg11_bn": ("y", "i1", "i2", "i4", "i6", "i8")}


def _offset(engine, which):
    off = ctypes.c_long()
    from flsim._lib import check
    check(engine._fn("workspace_offset")(int(which), engine.max_samples, ctypes.byref(off)))
    return int(off.value)


def int_range(engine):
    """[lo, hi) bytes of the workspace's integer tensors (with the alignment gaps between them)."""
    ids = [engine.WORKSPACE.index(n) for n in INT_TENSORS[engine.PREFIX]]
    assert ids == list(range(ids[0], ids[0] + len(ids))), ids       # consecutive in the layout
    lo = _offset(engine, ids[0])
    if engine.PREFIX == "vgg11":
        hi = int(engine.workspace.numel())       # the argmax bytes end vgg11's workspace
    else:
        hi = _offset(engine, ids[-1] + 1)        # the next tensor (pn1: a1l, vgg11_bn: z0)
    assert 0 <= lo < hi <= engine.workspace.numel(), (lo, hi)
    return lo, hi


def buffers(engine):
    """gradstate, workspace and (pipelined engines) workspace2, made as run_chunk_async does."""
    if engine.PIPELINE and getattr(engine, "workspace2", None) is None:
        engine.workspace2 = torch.empty_like(engine.workspace)
    out = [engine.gradstate, engine.workspace]
    if getattr(engine, "workspace2", None) is not None:
        out.append(engine.workspace2)
    return out


def fill(engine, pattern):
    """Write `pattern` (32 bits) over the whole of the engine's raw buffers, then zero the
    workspaces' integer tensors.  Call before begin_epoch."""
    pattern = int(pattern) & 0xFFFFFFFF
    signed = pattern - (1 << 32) if pattern >= 1 << 31 else pattern
    lo, hi = int_range(engine)
    for buf in buffers(engine):
        assert buf.numel() % 4 == 0
        buf.view(torch.int32).fill_(signed)
    for ws in buffers(engine)[1:]:
        ws[lo:hi].zero_()
    torch.cuda.synchronize()
    return engine
