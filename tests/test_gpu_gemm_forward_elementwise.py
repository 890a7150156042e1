"""The forward token GEMMs, every output element: each launch form of tests/gemm_fwd_common.py's table under both instruments -- an EXACT run (dense
integer operands: the output must equal the float64 reference bit for bit, whatever the tile, ring depth, split, segment boundary or summation order)
and a ROUNDING run (Gaussian data: `2^-8 |ref| + 1e-5 sum|terms|` per element, plus the addends derived per form).  Side outputs (gn_partials per slot,
ln_out, ln_stats, the fold's w_out / bias_out, amax) are held the same way.

One launch per assertion.  A is a column slice of a wider NaN-filled matrix, residuals and out have row strides above N, every output and side output is
pre-filled with NaN (e4m3 bytes: 0x5A), so an unwritten element shows.  `fmc_linear_bf16` goes through `hip_ops.linear_bf16` where the wrapper passes
everything on (plain grid and persistent forms, `out=` a strided view); the split forms (the wrapper owns their workspace), tile 18 with a strided out
and the tile-16-only entry points (the wrappers allocate their outputs and pick the form themselves) go through the raw C ABI.  A case whose purpose is
a particular arm is asserted to reach it (`expected_kernel`); the split forms also assert that workspace slots were written and that the stream-K
flag words come back zero.  profiles/gemm_forward_bounds.md records one run (the largest err / bound per form)."""
import pytest
import torch

from tests import gemm_fwd_common as G

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _call(K, name, *args):
    K._lib.check(getattr(K._lib.load(), name)(*args), name)


def _p(t):
    return None if t is None else t.data_ptr()


_LIVE = []                                # every device operand of the running case: a temporary freed before the launch would be handed to the next allocation


def _dev(t):
    if t is None:
        return None
    _LIVE.append(t.cuda().contiguous())
    return _LIVE[-1]


def _slice(t, pad):
    """`t` on the device as the leading columns of a NaN-filled matrix `pad` columns wider (a row stride above the row length)."""
    if t is None:
        return None
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=t.dtype, device="cuda")
    _LIVE.append(buf)
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def _out(rows, cols, pad=8, dtype=BF16):
    return torch.full((rows, cols + pad), NAN, dtype=dtype, device="cuda")[:, :cols]


def _arm(K, tile):
    """C-ABI tile -> the arm id `hip_ops.linear_bf16` decodes back to it."""
    return {16: K.ARM_160, 17: K.ARM_256}.get(tile, K.ARM_SMALLM + tile - 19 if tile >= 19 else tile)


def _linear_bf16(K, c, d, cus):
    M, N, Kd = c.shape
    w, b = d["w"], d["b"]
    if c.geglu:
        w, b = G.interleave(w, b, G.geglu_block(c, cus))
    n_out = N // 2 if c.geglu else N
    xd, x2d = _slice(d["x"], 64), _slice(d["x2"], 64)
    rd, r2d = _slice(d["r"], 8), _slice(d["r2"], 8)
    out = _out(M, n_out)
    if c.split_k == 1 and c.tile != 18:
        K.linear_bf16(xd, _dev(w), _dev(b), rd, d["alpha"], c.geglu, _arm(K, c.tile), 1, x2d, r2d, out)
        return {"out": out}
    wd = _dev(G.tilemajor(w) if c.tile == 18 else w)
    bd = _dev(b)
    ws, nbytes = None, G.workspace_bytes(c, cus)
    if c.split_k != 1:
        ws = torch.full((nbytes // 4,), NAN, dtype=F32, device="cuda")
        if c.split_k < 0:
            ws[:1024].zero_()                                                    # the flag words: zero on entry, handed back zero
    _call(K, "fmc_linear_bf16", xd.data_ptr(), wd.data_ptr(), _p(bd), _p(rd), out.data_ptr(), M, N, Kd, xd.stride(0), rd.stride(0) if rd is not None else 0,
          out.stride(0), d["alpha"], int(c.geglu), c.tile, c.split_k, _p(ws), nbytes, _p(x2d), x2d.stride(0) if x2d is not None else 0, c.k_split, _p(r2d),
          K._stream())
    torch.cuda.synchronize()
    if c.split_k != 1:
        slots = ws[1024:] if c.split_k < 0 else ws
        assert int((~torch.isnan(slots)).sum()) > 0, f"{c.name}: no workspace slot was written -- the launch fell back to the plain grid"
        if c.split_k < 0:
            assert int(ws[:1024].view(torch.int32).abs().sum()) == 0, f"{c.name}: the stream-K flag words did not come back zero"
    return {"out": out}


def _tile16_entry(K, c, d, cus):
    """The tile-16-only entry points through the raw C ABI (argument order: include/fmc_hip.h)."""
    M, N, Kd = c.shape
    tm = int("w_tilemajor" in c.form)
    n_out = N // 2 if c.geglu else N
    w, b = d.get("w"), d.get("b")
    if c.geglu and "lnc" not in c.form:
        w, b = G.interleave(w, b, 8)
    pack = (lambda t: _dev(G.tilemajor(t) if tm else t))
    st = K._stream()
    if c.entry == "linear_bf16_gn":
        xd, rd, r2d, out = _slice(d["x"], 64), _slice(d["r"], 8), _slice(d["r2"], 8), _out(M, N)
        hw = G.gn_hw(c)
        part = torch.full((M // hw, hw // 160, 32, 2), NAN, dtype=F32, device="cuda")
        _call(K, "fmc_linear_bf16_gn", xd.data_ptr(), pack(w).data_ptr(), _p(_dev(b)), _p(rd), out.data_ptr(), M, N, Kd, xd.stride(0), rd.stride(0), out.stride(0),
              d["alpha"], _p(r2d), part.data_ptr(), hw, tm, st)
        return {"out": out, "gn_partials": part}
    if c.entry == "linear_bf16_ln":
        xd, rd, r2d, out = _slice(d["x"], 64), _slice(d["r"], 8), _slice(d["r2"], 8), _out(M, N)
        with_out = "ln_out" in c.form
        ln_out = torch.full((M, N), NAN, dtype=BF16, device="cuda") if with_out else None
        stats = None if with_out else torch.full((M, 2), NAN, dtype=F32, device="cuda")
        gd, btd, ped = _dev(d["gamma"]), _dev(d["beta"]), _dev(d["pe"]) if with_out else None
        _call(K, "fmc_linear_bf16_ln", xd.data_ptr(), pack(w).data_ptr(), _p(_dev(b)), _p(rd), out.data_ptr(), M, N, Kd, xd.stride(0), rd.stride(0), out.stride(0),
              d["alpha"], _p(r2d), _p(ln_out), gd.data_ptr(), btd.data_ptr(), G.LN_EPS, _p(ped), d["pe_inner"] if with_out else 1,
              d["pe_frames"] if with_out else 1, _p(stats), tm, st)
        return {"out": out, "ln_out": ln_out} if with_out else {"out": out, "ln_stats": stats}
    lnc = "lnc" in c.form
    if lnc:                                                                      # ln_c / ln_bias follow the weight's row order
        w, _ = G.interleave(d["w"], None, 8) if c.geglu else (d["w"], None)
        lc, lb = (G.interleave(d["ln_c"][:, None], d["ln_bias"], 8) if c.geglu else (d["ln_c"][:, None], d["ln_bias"]))
        sd, cd, lbd = _dev(d["ln_stats"]), _dev(lc[:, 0]), _dev(lb)
    if c.entry == "linear_bf16_lnc":
        xd, out = _slice(d["x"], 64), _out(M, n_out)
        _call(K, "fmc_linear_bf16_lnc", xd.data_ptr(), pack(w).data_ptr(), out.data_ptr(), M, N, Kd, xd.stride(0), out.stride(0), int(c.geglu), sd.data_ptr(),
              cd.data_ptr(), lbd.data_ptr(), tm, st)
        return {"out": out}
    if c.entry == "linear_bf16_ffblk":
        x_blocked, out_blocked = int("x_blocked" in c.form), int("out_blocked" in c.form)
        xd = _dev(G.blocked(d["x"]) if x_blocked else d["x"])
        rd = _slice(d["r"], 8)
        out = torch.full((M, n_out), NAN, dtype=BF16, device="cuda")
        _call(K, "fmc_linear_bf16_ffblk", xd.data_ptr(), pack(w).data_ptr(), None if lnc else _p(_dev(b)), _p(rd), out.data_ptr(), M, N, Kd,
              rd.stride(0) if rd is not None else 0, d["alpha"], int(c.geglu), x_blocked, out_blocked, sd.data_ptr() if lnc else None, cd.data_ptr() if lnc else None,
              lbd.data_ptr() if lnc else None, tm, st)
        torch.cuda.synchronize()
        return {"out": G.unblocked(out) if out_blocked else out}
    if c.entry == "linear_bf16_ffblk_partial":
        xd, rd = _dev(G.blocked(d["x"])), _slice(d["r"], 8)                      # (the pad rows of the last tile hold NaN: they reach no valid row)
        out = torch.full((M, N), NAN, dtype=BF16, device="cuda")
        _call(K, "fmc_linear_bf16_ffblk_partial", xd.data_ptr(), pack(w).data_ptr(), _p(_dev(b)), _p(rd), out.data_ptr(), M, N, Kd, rd.stride(0), d["alpha"], tm, st)
        return {"out": out}
    if c.entry in ("linear_bf16_fftail", "linear_bf16_fftail_partial"):
        xd, hd, rd = _dev(G.blocked(d["x"])), _slice(d["x2"], 64), _slice(d["r"], 8)
        out = torch.full((M, N), NAN, dtype=BF16, device="cuda")
        gn = "gn_partials" in c.form
        part = torch.full((M // 160, 1, 32, 2), NAN, dtype=F32, device="cuda") if gn else None
        _call(K, "fmc_" + c.entry, xd.data_ptr(), hd.data_ptr(), pack(w).data_ptr(), _p(_dev(b)), _p(rd), out.data_ptr(), M, N, Kd, c.k_split, hd.stride(0),
              rd.stride(0), _p(part), G.gn_hw(c) if gn else 0, tm, st)
        return {"out": out, "gn_partials": part} if gn else {"out": out}
    raise AssertionError(c.entry)


def _imgw(K, c, d, instrument, what):
    """`fmc_groupnorm_fold_linear` -> `fmc_linear_bf16_imgw`.  Rounding: the fold runs, its outputs are held against float64 and are then the projection's
    operands; exact: integer weights and fp32 bias rows of the test's own (the fold is not part of an exact run: its rstd is no power of two)."""
    M, N, Kd = c.shape
    tm = int("w_tilemajor" in c.form)
    n_img, hw = d["n_img"], d["img_rows"]
    st = K._stream()
    if instrument == "rounding":
        w_img = torch.full((n_img, N, Kd), NAN, dtype=BF16, device="cuda")
        b_img = torch.full((n_img, N), NAN, dtype=F32, device="cuda")
        ops = [_dev(d[k]) for k in ("partials", "gamma", "beta", "w", "b")]
        _call(K, "fmc_groupnorm_fold_linear", ops[0].data_ptr(), d["splits"], ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr(), ops[4].data_ptr(),
              w_img.data_ptr(), b_img.data_ptr(), n_img, hw, Kd, d["G"], N, d["eps"], tm, st)
        torch.cuda.synchronize()
        rowmajor = w_img.view(n_img, N // 320, Kd // 32, 320, 32).transpose(2, 3).reshape(n_img, N, Kd) if tm else w_img
        shares = G.check_fold(rowmajor, b_img, d, N, Kd, what)
        print(f"   {what}: fold w_out {shares[0]:.3f}, bias_out {shares[1]:.3f} of their bounds")
        d = G.with_fold(d, rowmajor, b_img)
    else:
        w_img, b_img = _dev(G.tilemajor(d["w_img"]) if tm else d["w_img"]), _dev(d["bias_img"])
    xd, out = _slice(d["x"], 64), _out(M, N)
    stats = torch.full((M, 2), NAN, dtype=F32, device="cuda") if "ln_stats" in c.form else None
    _call(K, "fmc_linear_bf16_imgw", xd.data_ptr(), w_img.data_ptr(), b_img.data_ptr(), out.data_ptr(), M, N, Kd, xd.stride(0), out.stride(0), hw, _p(stats),
          G.LN_EPS if stats is not None else 0.0, tm, st)
    return d, ({"out": out, "ln_stats": stats} if stats is not None else {"out": out})


def _launch(K, c, d, cus, instrument, what):
    M, N, Kd = c.shape
    st = K._stream()
    if c.entry == "linear_bf16":
        return d, _linear_bf16(K, c, d, cus)
    if c.entry == "linear_bf16_imgw":
        return _imgw(K, c, d, instrument, what)
    if c.entry == "linear4_bf16":
        xd, rd, r2d, out = _slice(d["x"], 64), _slice(d["r"], 8), _slice(d["r2"], 8), _out(M, N)
        assert K._lib.load().fmc_linear4_supported(M, N, Kd, xd.stride(0))
        _call(K, "fmc_linear4_bf16", xd.data_ptr(), _dev(d["w"]).data_ptr(), _p(_dev(d["b"])), _p(rd), _p(r2d), out.data_ptr(), M, N, Kd, xd.stride(0),
              rd.stride(0) if rd is not None else 0, out.stride(0), d["alpha"], st)
        return d, {"out": out}
    if c.entry == "linear_x3_f32":
        x3, w3 = K.split_bf16x3(d["x"].cuda(), 0), K.split_bf16x3(d["w"].cuda(), 1)
        xd = _slice(x3, 64)
        bd, rd, r2d, out = _dev(d["b"]), _slice(d["r"], 8), _slice(d["r2"], 8), _out(M, N, 8, F32)
        nbytes = c.split_k * M * N * 4 if c.split_k > 1 else 0
        ws = torch.full((nbytes // 4,), NAN, dtype=F32, device="cuda") if nbytes else None
        _call(K, "fmc_linear_x3_f32", xd.data_ptr(), w3.data_ptr(), bd.data_ptr(), rd.data_ptr(), out.data_ptr(), M, N, 3 * Kd, xd.stride(0), rd.stride(0),
              out.stride(0), d["alpha"], 0, c.tile, c.split_k, _p(ws), nbytes, r2d.data_ptr(), st)
        torch.cuda.synchronize()
        assert ws is None or int((~torch.isnan(ws)).sum()) > 0, f"{c.name}: no split-K partial was written"
        return d, {"out": out}
    if c.entry == "linear_fp8_qkv":
        xd = _slice(d["x"], 64)
        out = torch.full((M, N), 0x5A, dtype=U8, device="cuda")                  # 0x5A = 20.0: no byte of this run (|value| <= 16)
        amax = torch.zeros(3, dtype=F32, device="cuda")                          # accumulated into (atomicMax of float bit patterns): starts at zero
        _call(K, "fmc_linear_fp8_qkv", xd.data_ptr(), _dev(d["w"]).data_ptr(), out.data_ptr(), M, N, Kd, xd.stride(0), _dev(d["inv_scales"]).data_ptr(),
              amax.data_ptr(), st)
        return d, {"out": out, "amax": amax}
    return d, _tile16_entry(K, c, d, cus)


PARAMS = [pytest.param(n, i, id=f"{n}-{i}") for n in G.NAMES for i in ("exact", "rounding") if not (n == "fp8-qkv" and i == "rounding")]


@pytest.mark.parametrize("name,instrument", PARAMS)
def test_gemm_forward_every_element(K, name, instrument):
    cus = K._cus(torch.device("cuda", torch.cuda.current_device()))
    c = G.case(name, cus)
    kernel, form = G.expected_kernel(c, cus)
    if c.want is not None:
        assert (kernel, form) == tuple(c.want), f"{name}: the dispatch restatement sends this case to {kernel} ({form}), not to the arm it exists for"
    what = f"{name} [{instrument}] {c.entry} tile {c.tile} split_k {c.split_k} {c.shape} -> {kernel}, {form}"
    d = G.inputs(c, instrument)
    _LIVE.clear()
    try:
        d, got = _launch(K, c, d, cus, instrument, what)
        torch.cuda.synchronize()
    except RuntimeError as e:                                                    # a launch or device error: nothing more is started on this GPU
        pytest.exit(f"gemm-forward {what}: {e}", returncode=3)
    for k, v in got.items():                                                     # the pad columns behind a strided output keep their NaN
        if v.dim() == 2 and v.stride(0) > v.shape[1] and v.dtype.is_floating_point:
            pad = torch.as_strided(v, (v.shape[0], v.stride(0) - v.shape[1]), v.stride(), v.storage_offset() + v.shape[1])
            assert bool(torch.isnan(pad).all()), f"{what}: {k} wrote behind its rows"
    shares = G.check(c, d, {k: v.cpu() for k, v in got.items()}, instrument, what)
    _LIVE.clear()
    print(f"gemm-forward {what}: " + ("bit-equal" if instrument == "exact" and not shares else "") +
          ", ".join(f"{k} {v:.3f} of its bound" for k, v in shares.items()))
