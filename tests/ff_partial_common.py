"""Shared by tests/test_ff_partial_host.py (CPU) and tests/test_gpu_ff_partial.py: the feed-forward chain with a partly filled last tile.

Pure torch, imports no GPU code.  What is here:

  * the case tables of the GPU file (remainders of the last tile, tile totals of the persistent GEMM) and `placement`, which says from the restated tile
    order (`g160p_tile_of`, `g160p_group_m`: restatements of csrc/gemm_conv.hip kept here, next to their only users) where the ragged tile of such a
    launch runs;
  * the tile-major layout `[ceil(M / 160)][K / 32][160][32]` as index arithmetic of its own (`blocked_index`: written with divmod per element, not
    through the kernels' own formula, which the host file checks it against);
  * `FFGuard`: the arenas of tests/edge_guard_common.py plus tile-major operands -- an INPUT whose pad rows (the rows of the last tile past M) hold the
    poison like everything around it, and an OUTPUT whose pad rows belong to the sentinel-filled outside;
  * `run_surroundings`: a case under zeros, quiet NaN and +Inf.  These are THE assertions of the GPU file: every sentinel word outside the output views
    intact (`OutsideTouched`), every word inside written (`InsideUnwritten`), outputs finite and bit-identical across the three fills
    (`SurroundingsMoved`); `assert_valid_rows_equal` is the bit comparison with the whole-tile result.  The host file runs wrong stand-ins through
    exactly these functions.
"""
import math

import torch

from tests import edge_guard_common as EG

ROWS = 160                                        # rows of a tile of the tile-major layout and of the persistent GEMM

# remainders (valid rows of the last tile) per kernel: one row, around the 16-row MFMA block, around the 80-row pass / wave row, one short of whole
PIPE80_REMAINDERS = (1, 15, 16, 17, 79)
PIPE160_REMAINDERS = (1, 79, 80, 81, 159)
GEMM_REMAINDERS = (1, 17, 79, 80, 81, 159)
PIPE_CFF = (128, 256, 384)                        # one, two, three chunks of 128 gated columns: the odd and the even tail of the chunk loop
GEMM_EXTRA_TILES = (0, 1, 8)                      # total tiles = CUs + this


def tiles(M, rows=ROWS):
    return -(-M // rows)


def blocked_index(M, K):
    """int64 `[M, K]`: element offset of (row m, column k) inside the tile-major storage, by the definition of the layout."""
    m = torch.arange(M, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    tile, row = m // ROWS, m % ROWS
    blk, col = k // 32, k % 32
    return ((tile * (K // 32) + blk) * ROWS + row) * 32 + col


def to_blocked(x, fill):
    """`[M, K]` -> flat tile-major storage of `tiles(M) * 160 * K` elements, the pad rows of the last tile holding `fill`."""
    M, K = x.shape
    flat = torch.full((tiles(M) * ROWS * K,), fill, dtype=x.dtype, device=x.device)
    flat[blocked_index(M, K).to(x.device).reshape(-1)] = x.reshape(-1)
    return flat


def from_blocked(flat, M, K):
    return flat[blocked_index(M, K).to(flat.device).reshape(-1)].view(M, K)


def last_tile_rows(M, rows=ROWS):
    """Valid rows of the last tile, 1 .. rows."""
    return M - (tiles(M, rows) - 1) * rows


# ---- the persistent GEMM's tile order, restated from csrc/gemm_conv.hip (`xcd_group_m`, `tile_of` + `lin_to_tile` of gemm160p_kernel) ----
def g160p_group_m(tiles_m, tiles_n, N, K):
    """`xcd_group_m` for a token projection on 160 x 320 tiles (no FMC_GEMM_GM override): m-tiles per group of the tile order."""
    if N * K * 2 <= 5 << 19:
        return 1
    c = min(32.0, tiles_m * tiles_n / 8.0)
    gm = int(math.floor(math.sqrt(c * 320 / 160) + 0.5))
    return gm if gm > 1 and tiles_n * 2 > 3 * (c / gm) else 1


def g160p_tile_of(tile_id, tiles_m, tiles_n, group_m=1):
    """Launch-order id -> (m-tile, n-tile).  XCD `id & 7` owns a contiguous range of the linear order; inside a group of `group_m` m-tiles the order is
    n-outer / m-inner.  Workgroup b of a grid of G runs ids b, b + G, ..."""
    total = tiles_m * tiles_n
    q, r, x = total >> 3, total & 7, tile_id & 7
    lin = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (tile_id >> 3)
    gsz = group_m * tiles_n
    g, rr = divmod(lin, gsz)
    first = g * group_m
    gm = min(group_m, tiles_m - first)
    tn = rr // gm
    return first + (rr - tn * gm), tn


def ragged_placements(tiles_m, tiles_n, group_m, cus):
    """Every tile of the LAST row tile: [(n-tile, workgroup, position in that workgroup's sequence, tiles that workgroup runs)]."""
    total = tiles_m * tiles_n
    out = []
    for tid in range(total):
        tm, tn = g160p_tile_of(tid, tiles_m, tiles_n, group_m)
        if tm == tiles_m - 1:
            out.append((tn, tid % cus, tid // cus, len(range(tid % cus, total, cus))))
    assert len(out) == tiles_n
    return sorted(out)


def placement(total, cus):
    """One n-tile, group_m = 1 (the N = 320 cases): (workgroup, position, tiles of that workgroup, the most tiles any workgroup runs) of the last row tile."""
    (_, wg, at, n), = ragged_placements(total, 1, 1, cus)
    return wg, at, n, max(len(range(b, total, cus)) for b in range(cus))


# a shape whose ragged row tile is the FIRST tile of a workgroup that runs a second one (another tile's first phase, with its `vmcnt(S_EPI + NE)`, follows
# the ragged tile's epilogue): it needs a grouped tile order, i.e. a weight beyond 2.5 MiB and several column tiles
WIDE_N, WIDE_K = 2560, 640


def wide_tiles_m(cus):
    """The smallest row-tile count at N = 2560, K = 640 for which some tile of the last row tile is a workgroup's first of two (None if there is none)."""
    tiles_n = WIDE_N // 320
    for tiles_m in range(-(-cus // tiles_n), 2 * cus // tiles_n + 1):
        gm = g160p_group_m(tiles_m, tiles_n, WIDE_N, WIDE_K)
        if any(at == 0 and n >= 2 for _, _, at, n in ragged_placements(tiles_m, tiles_n, gm, cus)):
            return tiles_m
    return None


class FFGuard(EG.Guard):
    """`EG.Guard` + tile-major operands.  Band = elements of guard on each side of the storage (a multiple of 8: 16-byte alignment)."""

    def __init__(self, poison, device="cpu"):
        super().__init__(poison, device)
        self.blocked_outputs = []

    def blocked_inp(self, values, band=4096, name="x_blocked"):
        """The tile-major storage of `values [M, K]` (a flat view, 16-byte aligned); pad rows and surroundings hold the poison."""
        M, Kd = values.shape
        n = tiles(M) * ROWS * Kd
        arena = torch.full((band + n + band,), EG.poison_value(self.poison, values.dtype), dtype=values.dtype, device=self.device)
        arena[band + blocked_index(M, Kd).to(self.device).reshape(-1)] = values.reshape(-1).to(self.device)
        view = arena[band:band + n]
        assert view.data_ptr() % 16 == 0
        self.inputs.append((name, arena, view))
        return view

    def blocked_out(self, M, Kd, dtype, band=4096, name="out_blocked"):
        """Sentinel-filled storage for a tile-major output of M valid rows; returns the flat view of the PADDED storage the kernel is handed."""
        n = tiles(M) * ROWS * Kd
        arena = torch.empty((band + n + band,), dtype=dtype, device=self.device)
        EG._bits(arena).fill_(EG.SENTINEL[dtype][1])
        view = arena[band:band + n]
        assert view.data_ptr() % 16 == 0
        self.blocked_outputs.append((name, arena, band, M, Kd))
        return view

    def check(self, what=""):
        super().check(what)
        for name, arena, band, M, Kd in self.blocked_outputs:
            own = torch.zeros(arena.numel(), dtype=torch.bool, device=arena.device)
            own[band + blocked_index(M, Kd).to(arena.device).reshape(-1)] = True       # the pad rows of the last tile are OUTSIDE
            is_sent = EG._bits(arena) == EG.SENTINEL[arena.dtype][1]
            touched = ~own & ~is_sent
            if bool(touched.any()):
                at = int(touched.nonzero()[0]) - band
                raise EG.OutsideTouched(f"{what} {name} [{self.poison}]: {int(touched.sum())} words outside the valid rows were written, the first at storage "
                                        f"element {at} (tile-major storage of {tiles(M)} tiles, {M} valid rows)")
            unwritten = own & is_sent
            if bool(unwritten.any()):
                raise EG.InsideUnwritten(f"{what} {name} [{self.poison}]: {int(unwritten.sum())} of {int(own.sum())} words of the valid rows were never written")


def run_surroundings(fn, device="cpu", what="", sync=None):
    """`EG.run_surroundings` on an `FFGuard`: `fn(guard) -> {name: output}` under zeros, NaN and +Inf around every input and in the pad rows of the
    tile-major operands.  `fn` returns a tile-major output as its valid rows (`from_blocked`); the pad rows are the containment check's business.
    Returns the outputs of the zeros run (clones)."""
    results = {}
    for poison in EG.POISONS:
        g = FFGuard(poison, device)
        outs = fn(g)
        if sync is not None:
            sync()
        g.check(what)
        results[poison] = {k: v.clone() for k, v in outs.items()}
    EG.assert_same_bits(results, what)
    return results[EG.POISONS[0]]


def assert_valid_rows_equal(got, want, what=""):
    """Bit identity of the valid rows with the whole-tile result (`want`: that result cut to the same rows)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(got, want):
        diff = (EG._bits(got.contiguous()) != EG._bits(want.contiguous()))
        rows = diff.reshape(got.shape[0], -1).any(-1).nonzero().reshape(-1)
        raise AssertionError(f"{what}: {int(diff.sum())} elements in {rows.numel()} rows differ from the whole-tile result, the first row {int(rows[0])}, "
                             f"the last {int(rows[-1])} of {got.shape[0]}")
