"""Guarded inputs and outputs for the edge tests of the forward kernels (pure torch; imports no GPU code).

A kernel with a partial last tile either stages rows that do not exist, or clamps, or zero-fills, or masks; an output comparison
sees none of it while the memory behind a tensor is whatever the allocator left (finite, usually).  These helpers put a tensor in
the middle of an ARENA the test owns:

    guarded_input   the tensor's values, and `poison` (zeros, quiet NaN or +Inf) in every other element of the arena: a pad row that
                    reaches the result through `0 * x` or a row maximum shows as a changed bit or a NaN;
    guarded_output  the same layout filled with a sentinel bit pattern; `assert_contained` then demands that every word outside the
                    view still holds it and that every word inside was written.

The arena is flat: `lead` elements of guard (rows_before rows, rounded up so that the view starts on a 16-byte boundary), the rows of
the tensor `row stride = width + col_pad` elements apart (the pad columns belong to the guard), `rows_after` rows of guard.  A band
is given in ROWS of the tensor: the case tables choose it at least as large as the largest tile, in rows, of the kernel under
test, so that a reach of one tile past either end lands in memory of the test's own.

An output that the ABI ACCUMULATES into (dgamma / dbeta, `out` with `accumulate != 0`, a running amax) cannot start as sentinel: `Guard.out(...,
init=...)` initialises the view as the ABI demands and leaves the sentinel around it; of such an output only the outside of the view is checked.

Used by test_edge_guard_host.py (CPU), test_gpu_edge_guards.py, test_gpu_edge_guards_fused.py and test_gpu_edge_guards_training.py.
"""
import math

import torch

POISONS = ("zeros", "nan", "inf")
_POISON_VALUE = {"zeros": 0.0, "nan": float("nan"), "inf": float("inf")}

# the sentinels of test_gpu_attn_backward.py; one byte of the same pattern for byte outputs (e4m3: 0x5A = 104.0, finite)
SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A), torch.uint8: (torch.uint8, 0x5A)}


def poison_value(poison, dtype):
    """The fill of an input arena: 0, quiet NaN or +Inf; integer arenas (key masks: nonzero = attend) get 0 resp. all ones."""
    assert poison in POISONS, poison
    if dtype.is_floating_point:
        return _POISON_VALUE[poison]
    return 0 if poison == "zeros" else torch.iinfo(dtype).max


def _layout(shape, itemsize, rows_before, rows_after, col_pad):
    """(arena elements, offset of the view, strides of the view).  The last dim is the row; the leading dims are dense over rows."""
    assert len(shape) >= 1 and rows_before >= 0 and rows_after >= 0
    assert col_pad >= 0 and col_pad % 8 == 0, "col_pad: a multiple of 8 elements (the kernels' stride rule)"
    width = int(shape[-1])
    rows = int(math.prod(shape[:-1]))
    stride = width + col_pad
    per16 = 16 // itemsize
    lead = -(-(rows_before * stride) // per16) * per16                      # 16-byte aligned start of the view
    total = lead + rows * stride + rows_after * stride
    strides, s = [1], stride
    for d in reversed(shape[1:-1]):
        strides.insert(0, s)
        s *= int(d)
    if len(shape) > 1:
        strides.insert(0, s)
    return total, lead, tuple(strides)


def guarded_input(values, poison, rows_before, rows_after, col_pad=0, device=None):
    """`(arena, view)`: `view` holds exactly `values` (its dtype, its bits), starts 16-byte aligned and has a dense last dim with
    rows `values.shape[-1] + col_pad` elements apart; every other element of the flat `arena` holds the poison."""
    device = values.device if device is None else device
    total, lead, strides = _layout(tuple(values.shape), values.element_size(), rows_before, rows_after, col_pad)
    arena = torch.full((total,), poison_value(poison, values.dtype), dtype=values.dtype, device=device)
    view = arena.as_strided(tuple(values.shape), strides, lead)
    view.copy_(values)
    assert view.data_ptr() % 16 == 0
    return arena, view


def _bits(t):
    return t.view(SENTINEL[t.dtype][0])


def guarded_output(shape, dtype, rows_before, rows_after, col_pad=0, device="cpu"):
    """`(arena, view)` in the layout of `guarded_input`, every word of the arena holding the sentinel of `dtype` (bf16: 0x5A5A,
    fp32 -- outputs, LSE, statistics partials, workspaces --: 0x5A5A5A5A, uint8 -- e4m3 bytes --: 0x5A)."""
    total, lead, strides = _layout(tuple(shape), torch.empty((), dtype=dtype).element_size(), rows_before, rows_after, col_pad)
    arena = torch.empty((total,), dtype=dtype, device=device)
    _bits(arena).fill_(SENTINEL[dtype][1])
    view = arena.as_strided(tuple(shape), strides, lead)
    assert view.data_ptr() % 16 == 0
    return arena, view


def owned_mask(arena, view):
    """bool `[arena.numel()]`: the elements of the flat arena that belong to the view."""
    assert view.dtype == arena.dtype and view.device == arena.device
    first = (view.data_ptr() - arena.data_ptr()) // arena.element_size()
    if view.is_contiguous():                                              # (large workspaces: no index tensor)
        own = torch.zeros(arena.numel(), dtype=torch.bool, device=arena.device)
        own[first:first + view.numel()] = True
        return own
    index = torch.arange(arena.numel(), device=arena.device).as_strided(tuple(view.shape), tuple(view.stride()), first)
    own = torch.zeros(arena.numel(), dtype=torch.bool, device=arena.device)
    own[index.reshape(-1)] = True
    return own


class OutsideTouched(AssertionError):
    """A word of the guard band no longer holds the sentinel: the kernel wrote outside its output."""


class InsideUnwritten(AssertionError):
    """A word of the view still holds the sentinel: the kernel left part of its output unwritten."""


def assert_contained(arena, view, what="", written=True):
    """Every word outside the view keeps the sentinel (`OutsideTouched` otherwise), and every word inside was written
    (`InsideUnwritten`).  `written=False`: scratch the kernel may use in part (a workspace sized 'at least')."""
    own = owned_mask(arena, view)
    is_sent = _bits(arena) == SENTINEL[arena.dtype][1]
    touched = ~own & ~is_sent
    if bool(touched.any()):
        at = int(touched.nonzero()[0])
        first = (view.data_ptr() - arena.data_ptr()) // arena.element_size()
        raise OutsideTouched(f"{what}: {int(touched.sum())} words outside the view were written, the first at arena element {at} "
                             f"(the view starts at {first}, the arena has {arena.numel()})")
    if written:
        unwritten = own & is_sent
        if bool(unwritten.any()):
            raise InsideUnwritten(f"{what}: {int(unwritten.sum())} of {int(own.sum())} words of the view were never written, the first at "
                                  f"arena element {int(unwritten.nonzero()[0])}")


def assert_poison_intact(arena, view, poison, what=""):
    """The guard of an INPUT still holds the poison everywhere: a forward kernel writes no operand, and a stray store of another
    output that lands in an input's arena shows here (`OutsideTouched`)."""
    outside = arena[~owned_mask(arena, view)]
    fill = poison_value(poison, arena.dtype)
    ok = torch.isnan(outside) if poison == "nan" and arena.dtype.is_floating_point else outside == fill
    if not bool(ok.all()):
        raise OutsideTouched(f"{what}: {int((~ok).sum())} guard elements of an input no longer hold the poison")


class SurroundingsMoved(AssertionError):
    """The output differs between two surroundings, or is not finite: something outside the extents reached the result."""


def assert_same_bits(results, what=""):
    """`results`: {poison: {name: tensor}} of one case under the three surroundings.  Every output is finite and bit-identical
    across them (`torch.equal`; no tolerance)."""
    base = results[POISONS[0]]
    for name, t in base.items():
        if not bool(torch.isfinite(t.float()).all()):
            raise SurroundingsMoved(f"{what} {name}: not finite under {POISONS[0]}")
    for poison in POISONS[1:]:
        for name, t in results[poison].items():
            if not bool(torch.isfinite(t.float()).all()):
                raise SurroundingsMoved(f"{what} {name}: {int((~torch.isfinite(t.float())).sum())} non-finite elements with {poison} around the inputs")
            if not torch.equal(t, base[name]):
                diff = (_bits(t.contiguous()) != _bits(base[name].contiguous()))
                raise SurroundingsMoved(f"{what} {name}: {int(diff.sum())} elements differ between {POISONS[0]} and {poison} around the inputs")


class Guard:
    """The arenas of one run of a case under one poison: `inp` / `out` hand out views, `check` runs `assert_contained` on every
    output.  `bands` records (name, rows before, rows after, col_pad) for the record."""

    def __init__(self, poison, device="cpu"):
        self.poison, self.device = poison, device
        self.inputs, self.outputs, self.bands = [], [], []

    def inp(self, values, band, col_pad=0, name="in"):
        before, after = band if isinstance(band, tuple) else (band, band)
        arena, view = guarded_input(values, self.poison, before, after, col_pad, self.device)
        self.inputs.append((name, arena, view))
        self.bands.append((name, before, after, col_pad))
        return view

    def out(self, shape, dtype, band, col_pad=0, name="out", written=True, init=None):
        """`init` (a number or a tensor of the view's shape): an output the ABI accumulates into.  The view starts as `init`, the sentinel
        stays around it, and only the outside of the view is checked (what is inside is for the reference to judge)."""
        before, after = band if isinstance(band, tuple) else (band, band)
        arena, view = guarded_output(shape, dtype, before, after, col_pad, self.device)
        if init is not None:
            view.copy_(init) if torch.is_tensor(init) else view.fill_(init)
            written = False
        self.outputs.append((name, arena, view, written))
        self.bands.append((name, before, after, col_pad))
        return view

    def check(self, what=""):
        for name, arena, view, written in self.outputs:
            assert_contained(arena, view, f"{what} {name} [{self.poison}]", written)
        for name, arena, view in self.inputs:
            assert_poison_intact(arena, view, self.poison, f"{what} {name} [{self.poison}]")


def run_surroundings(fn, device="cpu", what="", sync=None):
    """Run `fn(guard) -> {name: output view}` under zeros, NaN and +Inf; `assert_contained` on every output of every run, then
    `assert_same_bits`.  Returns the outputs of the zeros run (clones)."""
    results = {}
    for poison in POISONS:
        g = Guard(poison, device)
        outs = fn(g)
        if sync is not None:
            sync()
        g.check(what)
        results[poison] = {k: v.clone() for k, v in outs.items()}
    assert_same_bits(results, what)
    return results[POISONS[0]]
