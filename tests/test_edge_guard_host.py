"""The helpers of tests/edge_guard_common.py do what they say, and each assertion catches the fault it is written for (CPU).

The "kernels" here are plain-torch stand-ins that reach into the arena the way a HIP kernel with a partial last tile does: through
`as_strided` past the end of the view they were given.  Nine of them are wrong, each in one way, and each must fail exactly its own one of

    bits       `assert_same_bits`: finite and bit-identical under zeros, NaN and +Inf around the inputs
    outside    `assert_contained`: a word outside the output view was written
    unwritten  `assert_contained`: a word of the output view was not written
    gate       the comparison with the float64 reference (under zeros around the inputs: what the suite had before)

and none of the reads and stray writes fails the gate: that is the gap the GPU file closes.  (The unwritten row does, but only because the
sentinel stands in it.)"""
import pytest
import torch

from tests import edge_guard_common as EG

DTYPES = [torch.bfloat16, torch.float32]
TAG = {torch.bfloat16: "bf16", torch.float32: "fp32"}
TILE = 8                                     # the stand-ins' tile: rows staged or stored at a time


def _rnd(shape, seed, dtype):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# ---- the helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("poison", EG.POISONS)
@pytest.mark.parametrize("shape,before,after,col_pad", [((5, 24), 3, 2, 0), ((2, 7, 40), 8, 8, 16), ((13,), 1, 1, 0), ((3, 2, 5, 8), 0, 4, 8)])
def test_guarded_input_layout(dtype, poison, shape, before, after, col_pad):
    values = _rnd(shape, 1, dtype)
    arena, view = EG.guarded_input(values, poison, before, after, col_pad)
    assert view.dtype == dtype and view.shape == values.shape and view.data_ptr() % 16 == 0
    assert torch.equal(view.view(EG.SENTINEL[dtype][0]), values.view(EG.SENTINEL[dtype][0]))           # the bits
    width, stride = shape[-1], shape[-1] + col_pad
    assert view.stride(-1) == 1
    if len(shape) > 1:
        assert view.stride(-2) == stride
        for d in range(len(shape) - 2):
            assert view.stride(d) == view.stride(d + 1) * shape[d + 1]                                  # leading dims dense over rows
    first = (view.data_ptr() - arena.data_ptr()) // arena.element_size()
    rows = values.numel() // width
    assert first >= before * stride and arena.numel() - first - rows * stride == after * stride         # the bands, in rows
    own = EG.owned_mask(arena, view)
    assert int(own.sum()) == values.numel()
    outside = arena[~own]
    assert outside.numel() == arena.numel() - values.numel()
    if poison == "zeros":
        assert bool((outside == 0).all())
    elif poison == "nan":
        assert bool(torch.isnan(outside).all())
    else:
        assert bool((outside == float("inf")).all())
    if col_pad:                                                                                       # the pad columns are guard
        pad = arena.as_strided((rows, col_pad), (stride, 1), first + width)
        assert not bool(torch.isfinite(pad).any()) if poison != "zeros" else bool((pad == 0).all())


def test_guarded_input_integer_mask():
    keep = torch.tensor([[1, 0, 1], [1, 1, 0]], dtype=torch.uint8)
    for poison, fill in (("zeros", 0), ("nan", 255), ("inf", 255)):
        arena, view = EG.guarded_input(keep, poison, 4, 4)
        assert torch.equal(view, keep) and view.data_ptr() % 16 == 0
        assert bool((arena[~EG.owned_mask(arena, view)] == fill).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_guarded_output_and_assert_contained(dtype):
    itype, sent = EG.SENTINEL[dtype]
    arena, view = EG.guarded_output((2, 5, 16), dtype, 3, 3, col_pad=8)
    assert view.data_ptr() % 16 == 0 and view.stride() == (5 * 24, 24, 1)
    assert bool((arena.view(itype) == sent).all())
    with pytest.raises(EG.InsideUnwritten):
        EG.assert_contained(arena, view)                               # nothing written yet
    EG.assert_contained(arena, view, written=False)
    view.copy_(_rnd((2, 5, 16), 2, dtype))
    EG.assert_contained(arena, view)
    view[1, 4, 15] = torch.zeros((), dtype=dtype).view(itype).fill_(sent).view(dtype)      # one word back to the sentinel
    with pytest.raises(EG.InsideUnwritten):
        EG.assert_contained(arena, view)
    view[1, 4, 15] = 1.0
    arena[0] = 1.0                                                     # the first guard word
    with pytest.raises(EG.OutsideTouched):
        EG.assert_contained(arena, view)
    arena.view(itype)[0] = sent
    arena[-1] = 0.0                                                    # the last one
    with pytest.raises(EG.OutsideTouched):
        EG.assert_contained(arena, view)


@pytest.mark.parametrize("poison", EG.POISONS)
def test_a_store_into_an_inputs_guard_is_seen(poison):
    g = EG.Guard(poison)
    x = g.inp(_rnd((4, 8), 3, torch.float32), 2)
    g.check()
    x[0, 0] = 7.0                                                       # the operand itself is the kernel's to read, not checked here
    g.check()
    g.inputs[0][1][0] = 1.0                                             # ... its guard is
    with pytest.raises(EG.OutsideTouched):
        g.check()


def test_assert_same_bits():
    a = torch.tensor([1.0, 2.0, 3.0])
    same = {p: {"y": a.clone()} for p in EG.POISONS}
    EG.assert_same_bits(same)
    moved = {p: {"y": a.clone()} for p in EG.POISONS}
    moved["inf"]["y"][1] = torch.nextafter(a[1], a[2])                 # one ulp
    with pytest.raises(EG.SurroundingsMoved):
        EG.assert_same_bits(moved)
    nan = {p: {"y": a.clone()} for p in EG.POISONS}
    nan["nan"]["y"][0] = float("nan")
    with pytest.raises(EG.SurroundingsMoved):
        EG.assert_same_bits(nan)


def test_byte_sentinel_and_byte_output():
    """e4m3 outputs are bytes: a one-byte sentinel, the same containment rules."""
    itype, sent = EG.SENTINEL[torch.uint8]
    assert itype == torch.uint8 and sent == 0x5A
    arena, view = EG.guarded_output((5, 48), torch.uint8, 2, 2, col_pad=16)
    assert view.data_ptr() % 16 == 0 and view.stride() == (64, 1) and bool((arena == sent).all())
    with pytest.raises(EG.InsideUnwritten):
        EG.assert_contained(arena, view)
    view.fill_(3)
    EG.assert_contained(arena, view)
    arena[-1] = 0
    with pytest.raises(EG.OutsideTouched):
        EG.assert_contained(arena, view)
    same = {p: {"y": view.clone()} for p in EG.POISONS}
    EG.assert_same_bits(same)
    same["nan"]["y"][0, 0] = 4
    with pytest.raises(EG.SurroundingsMoved):
        EG.assert_same_bits(same)


@pytest.mark.parametrize("init", [0.0, "tensor"])
def test_initialised_view_checks_outside_only(init):
    """`Guard.out(init=...)`: the view starts as the ABI demands (also when that happens to be the sentinel's value), is not asked to have been
    written, and the words around it still are checked."""
    g = EG.Guard("zeros")
    start = _rnd((3, 8), 5, torch.float32) if init == "tensor" else init
    acc = g.out((3, 8), torch.float32, 2, 8, "acc", init=start)
    assert torch.equal(acc, start if init == "tensor" else torch.zeros(3, 8))
    name, arena, view, written = g.outputs[0]
    assert written is False and bool((arena[~EG.owned_mask(arena, view)].view(torch.int32) == EG.SENTINEL[torch.float32][1]).all())
    g.check()                                                           # nothing written: fine for an accumulator
    acc[0, 0] = torch.zeros((), dtype=torch.int32).fill_(EG.SENTINEL[torch.float32][1]).view(torch.float32)
    g.check()                                                           # ... and a sum that equals the sentinel is no finding
    arena[arena.numel() - 1] = 1.0
    with pytest.raises(EG.OutsideTouched):
        g.check()


# ---- stand-in kernels ---------------------------------------------------------------------------------------------------------
def _past(view, extra_rows=0, extra_cols=0):
    """The view with more rows / columns than it has: what a kernel's address arithmetic reaches past a partial tile."""
    shape = list(view.shape)
    shape[-2] += extra_rows
    shape[-1] += extra_cols
    return view.as_strided(shape, view.stride(), view.storage_offset())


def attn_standin(fault):
    """softmax(q k^T) v for one head; keys are staged a tile of 8 at a time, 13 of them exist."""
    Sq, Skv, D = 5, 13, 16
    q, k, v = _rnd((Sq, D), 10, torch.float32).abs(), _rnd((Skv, D), 11, torch.float32), _rnd((Skv, D), 12, torch.float32)
    # (q >= 0: the score of a +Inf pad key is +Inf, not the NaN of Inf - Inf, which the maximum would drop like any NaN)
    ref = torch.softmax(q.double() @ k.double().t(), -1) @ v.double()

    def run(g):
        qv, kv, vv = g.inp(q, TILE), g.inp(k, TILE), g.inp(v, TILE)
        o = g.out((Sq, D), torch.float32, TILE)
        tiles = -(-Skv // TILE) * TILE
        if fault == "zero_prob":                                       # pad keys staged; their probability is 0 by multiplication
            vt = _past(vv, tiles - Skv)
            valid = (torch.arange(tiles) < Skv).float()
            s = qv @ kv.t()
            p = torch.softmax(s, -1)
            p = torch.cat([p, torch.ones(Sq, tiles - Skv)], 1) * valid
            o.copy_(p @ vt)
        elif fault == "pad_max":                                       # the row maximum runs over the pad scores too (a hardware max drops NaN)
            kt = _past(kv, tiles - Skv)
            s_all = qv @ kt.t()
            m = s_all[:, 0]
            for j in range(1, tiles):
                m = torch.fmax(m, s_all[:, j])
            e = torch.exp(s_all[:, :Skv] - m[:, None])
            o.copy_((e @ vv) / e.sum(-1, keepdim=True))
        else:
            o.copy_(torch.softmax(qv @ kv.t(), -1) @ vv)
        return {"o": o}

    return run, {"o": ref}, 1e-5


def groupnorm_standin(fault):
    """GroupNorm statistics + apply over [HW, C] with one group; rows are summed a tile at a time, 11 of them exist."""
    HW, C = 11, 16
    x = _rnd((HW, C), 20, torch.float32)
    xd = x.double()
    ref = (xd - xd.mean()) / torch.sqrt(xd.var(unbiased=False) + 1e-5)

    def run(g):
        xv = g.inp(x, TILE)
        y = g.out((HW, C), torch.float32, TILE)
        xs = _past(xv, 1) if fault == "pad_stat" else xv                # the sum takes one row too many (and divides by the right count)
        n = HW * C
        mean = xs.double().sum() / n
        var = (xs.double() ** 2).sum() / n - mean ** 2
        y.copy_(((xv.double() - mean) / torch.sqrt(var + 1e-5)).float())
        return {"y": y}

    return run, {"y": ref}, 1e-5


def copy_standin(fault, col_pad=8):
    """y = 2 x on [R, W] rows of a wider buffer; stores go a tile of rows at a time."""
    R, W = 11, 24
    x = _rnd((R, W), 30, torch.bfloat16)
    ref = 2 * x.double()

    def run(g):
        xv = g.inp(x, TILE, col_pad)
        y = g.out((R, W), torch.bfloat16, TILE, col_pad)
        if fault == "row_past":                                        # the store guard is one row too generous
            _past(y, 1)[:R + 1] = torch.cat([2 * xv, torch.zeros(1, W, dtype=x.dtype)])
        elif fault == "col_past":                                      # ... or one column
            _past(y, 0, 1)[:, :W + 1] = torch.cat([2 * xv, torch.zeros(R, 1, dtype=x.dtype)], 1)
        elif fault == "last_row":                                      # ... or one row too tight
            y[:R - 1] = 2 * xv[:R - 1]
        else:
            y.copy_(2 * xv)
        return {"y": y}

    return run, {"y": ref}, 2.0 ** -8


def column_sum_standin(fault):
    """out = sum over the 11 rows of x [11, 16], rows summed a tile of 8 at a time: the training side's reductions."""
    M, N = 11, 16
    x = _rnd((M, N), 40, torch.float32)
    ref = x.double().sum(0)

    def run(g):
        xv = g.inp(x, TILE)
        out = g.out((N,), torch.float32, 2)
        xs = _past(xv, 1) if fault == "pad_row" else xv                 # the last tile's row guard is one row too generous
        out.copy_(xs.double().sum(0).float())
        return {"out": out}

    return run, {"out": ref}, 1e-5


def accumulate_standin(fault):
    """out += x.sum(rows) into an accumulator the ABI wants initialised (here: to `base`); stores go four words at a time."""
    M, N = 11, 12
    x, base = _rnd((M, N), 41, torch.float32), _rnd((N,), 42, torch.float32)
    ref = base.double() + x.double().sum(0)

    def run(g):
        xv = g.inp(x, TILE)
        out = g.out((N,), torch.float32, 2, name="out", init=base)
        add = xv.double().sum(0).float()
        if fault == "spill":                                           # one word past the view gets the "accumulated" 0 + old value
            wide = out.as_strided((N + 1,), (1,), out.storage_offset())
            wide += torch.cat([add, torch.zeros(1)])
            wide[N] = 0.0
        else:
            out += add
        return {"out": out}

    return run, {"out": ref}, 1e-5


def byte_standin(fault):
    """y = byte(x) on [R, W] rows of bytes, rows `W + 16` apart: an fp8 epilogue's output."""
    R, W = 11, 32
    x = torch.randint(1, 0x5A, (R, W), generator=torch.Generator().manual_seed(43), dtype=torch.uint8)      # (below the sentinel: a byte has no spare pattern,
                                                                                                          # so a case keeps its values off 0x5A)
    ref = x.double()

    def run(g):
        xv = g.inp(x, TILE, 16)
        y = g.out((R, W), torch.uint8, TILE, 16)
        if fault == "row_past":                                        # one row too many
            _past(y, 1)[:R + 1] = torch.cat([xv, torch.zeros(1, W, dtype=torch.uint8)])
        else:
            y.copy_(xv)
        return {"y": y}

    return run, {"y": ref}, 2.0 ** -8


def verdicts(run, refs, tol):
    """Which of the three guard assertions a stand-in fails, and "gate" when it misses the reference under zeros."""
    failed, results = set(), {}
    for poison in EG.POISONS:
        g = EG.Guard(poison)
        outs = run(g)
        for name, arena, view, written in g.outputs:
            try:
                EG.assert_contained(arena, view, name, written)
            except EG.OutsideTouched:
                failed.add("outside")
            except EG.InsideUnwritten:
                failed.add("unwritten")
        results[poison] = {k: v.clone() for k, v in outs.items()}
    try:
        EG.assert_same_bits(results)
    except EG.SurroundingsMoved:
        failed.add("bits")
    for name, ref in refs.items():
        got = results["zeros"][name].double()
        if not float((got - ref).abs().max() / ref.abs().max()) < tol:
            failed.add("gate")
    return failed


WRONG = [
    ("pad key with probability 0 by multiplication", lambda: attn_standin("zero_prob"), {"bits"}),
    ("row maximum over pad scores", lambda: attn_standin("pad_max"), {"bits"}),
    ("GroupNorm statistic summed over a pad row", lambda: groupnorm_standin("pad_stat"), {"bits"}),
    ("one row written past the end", lambda: copy_standin("row_past"), {"outside"}),
    ("one column written past a strided row", lambda: copy_standin("col_past"), {"outside"}),
    ("last row left unwritten", lambda: copy_standin("last_row"), {"unwritten", "gate"}),       # (the gate too: the row holds the sentinel here; in a
                                                                                                # fresh allocation it would hold the previous call's right result)
    ("reduction over one pad row", lambda: column_sum_standin("pad_row"), {"bits"}),
    ("accumulate-output spills one word past its view", lambda: accumulate_standin("spill"), {"outside"}),
    ("byte output one row too long", lambda: byte_standin("row_past"), {"outside"}),
]


@pytest.mark.parametrize("what,make,expected", WRONG, ids=[w[0].replace(" ", "_") for w in WRONG])
def test_wrong_standin_fails_exactly_its_assertion(what, make, expected):
    run, refs, tol = make()
    got = verdicts(run, refs, tol)
    assert got == expected, f"{what}: failed {sorted(got)}, expected {sorted(expected)}"


@pytest.mark.parametrize("make", [lambda: attn_standin(None), lambda: groupnorm_standin(None), lambda: copy_standin(None), lambda: copy_standin(None, 0),
                                  lambda: column_sum_standin(None), lambda: accumulate_standin(None), lambda: byte_standin(None)],
                         ids=["attention", "groupnorm", "strided_copy", "dense_copy", "column_sum", "accumulate", "byte_copy"])
def test_correct_standin_passes_under_all_surroundings(make):
    run, refs, tol = make()
    assert verdicts(run, refs, tol) == set()
    out = EG.run_surroundings(run, what="stand-in")                    # the driver the GPU file uses
    for name, ref in refs.items():
        assert float((out[name].double() - ref).abs().max() / ref.abs().max()) < tol
