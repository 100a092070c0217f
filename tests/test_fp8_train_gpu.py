"""The fp8 training Linear on the GPU: the fused amax and quantise kernels
(native/kernels/fp8_train.hip) against torch, bit for bit where the result is
exact; the three e4m3 products built from the raw ops, ``linear_fp8`` against
that composition and against its torch model; the decoder with ``linear="fp8"``."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
SHAPES = [(16, 16), (48, 272), (272, 48), (512, 768)]
POISON_BYTE = 0xAB


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, device=DEV, generator=g)).bfloat16()


def _bits(t):
    return t.view(torch.int32)


def _matrix(rows, cols, seed, strided=False):
    """A bf16 test matrix with an all-zero row and an all-zero column; with
    ``strided`` a view (ld = cols + 24) into a buffer whose padding is NaN."""
    x = _randn(_gen(seed), rows, cols, scale=3.0)
    x[2] = 0
    x[:, 5] = 0
    if strided:
        buf = torch.full((rows, cols + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
        buf[:, :cols] = x
        x = buf[:, :cols]
        assert x.stride(0) == cols + 24
    return x


def _torch_amax(x):
    a = x.float().abs()
    return a.amax(dim=1), a.amax(dim=0), a.amax().reshape(1)


# ----------------------------------------------------------------------------
# amax

# (2064, 8208): 17 x 33 = 561 tiles, past the 512 workgroups the grid is capped at when the tensor amax is
# asked for, so workgroups loop over tiles there (and do not when it is not asked for)
@pytest.mark.parametrize("rows,cols,strided", [(*s, False) for s in SHAPES] + [(48, 272, True), (2064, 8208, False)])
def test_amax_is_bit_equal_to_torch(rows, cols, strided):
    from kgs.ops import fp8_amax

    x = _matrix(rows, cols, rows + cols, strided)
    want = _torch_amax(x)
    got = fp8_amax(x, rows=True, cols=True, tensor=True)
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and torch.equal(_bits(g), _bits(w))
    assert got[0][2] == 0 and got[1][5] == 0
    # a null output leaves the others as they are; two runs are bit-identical
    for sel in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1)):
        part = fp8_amax(x, rows=bool(sel[0]), cols=bool(sel[1]), tensor=bool(sel[2]))
        for on, p, w in zip(sel, part, want):
            assert (p is None) == (not on)
            if on:
                assert torch.equal(_bits(p), _bits(w))


@pytest.mark.parametrize("rows,cols", SHAPES + [(2064, 8208)])
def test_amax_keeps_nan_and_inf_visible(rows, cols):
    from kgs.ops import fp8_amax

    x = _matrix(rows, cols, 7 * rows + cols)
    rn, cn, ri, ci = rows - 3, 1, 4, cols - 2
    for val, hit in ((float("nan"), torch.isnan), (float("inf"), torch.isinf)):
        y = x.clone()
        r, c = (rn, cn) if val != val else (ri, ci)
        y[r, c] = val
        ra, ca, ta = fp8_amax(y, rows=True, cols=True, tensor=True)
        assert hit(ta).all()
        assert hit(ra).nonzero().flatten().tolist() == [r] and hit(ca).nonzero().flatten().tolist() == [c]
        assert torch.isfinite(ra).sum() == rows - 1 and torch.isfinite(ca).sum() == cols - 1
    y = x.clone()
    y[rn, cn], y[ri, ci], y[rn, ci] = float("nan"), float("inf"), float("-inf")
    ra, ca, ta = fp8_amax(y, rows=True, cols=True, tensor=True)
    assert torch.isnan(ta).all() and torch.isnan(ra[rn]) and torch.isnan(ca[cn])  # NaN beats Inf
    assert torch.isinf(ra[ri]) and torch.isinf(ca[ci])
    for g, w in zip((ra, ca, ta), _torch_amax(y)):
        torch.testing.assert_close(g, w, rtol=0, atol=0, equal_nan=True)


# ----------------------------------------------------------------------------
# quantise

def _scale(amax):
    return amax.clamp(min=1e-12) / 448


def _check_image(x, q, s, per, what):
    """``q`` ([rows, cols], already un-transposed) against x with the unfolded
    scales ``s`` (``per``: 0 per row, 1 per column, None per tensor)."""
    xf = x.float()
    want = _scale(_torch_amax(x)[2 if per is None else per])
    torch.testing.assert_close(s, want, rtol=1e-6, atol=0, msg=lambda m: f"{what} scale: {m}")
    sb = s.reshape(1, 1) if per is None else (s[:, None] if per == 0 else s[None, :])
    deq = q.float() * sb
    assert not torch.isnan(deq).any(), what
    assert torch.all((deq - xf).abs() <= 2.0 ** -4 * xf.abs() + 2 * sb * 2.0 ** -9), what
    codes = q.contiguous().view(torch.uint8)
    assert (codes[2] == 0).all() and (codes[:, 5] == 0).all(), what


@pytest.mark.parametrize("rows,cols,strided", [(*s, False) for s in SHAPES] + [(48, 272, True)])
def test_quantise_every_output_combination(rows, cols, strided):
    from kgs.ops import fp8_amax, fp8_quantize

    x = _matrix(rows, cols, 3 * rows + cols, strided)
    ra, ca, ta = fp8_amax(x, rows=True, cols=True, tensor=True)
    fy, ft = torch.tensor([0.37], device=DEV), torch.tensor([5.5], device=DEV)

    # each image alone, per tensor and per row / column
    y_t, ys_t, none1, none2 = fp8_quantize(x, tensor_amax=ta)
    assert none1 is None and none2 is None and ys_t.shape == (1,)
    _check_image(x, y_t, ys_t, None, "y per tensor")
    y_r, ys_r, _, _ = fp8_quantize(x, row_amax=ra)
    assert ys_r.shape == (rows,)
    _check_image(x, y_r, ys_r, 0, "y per row")
    _, _, t_t, ts_t = fp8_quantize(x, tensor_amax=ta, y=False, yt=True)
    assert t_t.shape == (cols, rows) and ts_t.shape == (1,)
    _check_image(x, t_t.T, ts_t, None, "yt per tensor")
    _, _, t_c, ts_c = fp8_quantize(x, col_amax=ca, y=False, yt=True)
    assert ts_c.shape == (cols,)
    _check_image(x, t_c.T, ts_c, 1, "yt per column")

    # both per tensor: yt is y transposed bit for bit, and each is what it was alone
    y2, ys2, t2, ts2 = fp8_quantize(x, tensor_amax=ta, y=True, yt=True)
    assert torch.equal(t2.view(torch.uint8), y2.view(torch.uint8).T)
    assert torch.equal(y2.view(torch.uint8), y_t.view(torch.uint8))
    assert torch.equal(t2.view(torch.uint8), t_t.view(torch.uint8))
    assert torch.equal(ys2, ys_t) and torch.equal(ts2, ts_t)

    # y per row with yt per column (dy), and y per row with yt per tensor (x): each image as alone
    y3, ys3, t3, ts3 = fp8_quantize(x, row_amax=ra, col_amax=ca, y=True, yt=True)
    assert torch.equal(y3.view(torch.uint8), y_r.view(torch.uint8)) and torch.equal(ys3, ys_r)
    assert torch.equal(t3.view(torch.uint8), t_c.view(torch.uint8)) and torch.equal(ts3, ts_c)
    y4, ys4, t4, ts4 = fp8_quantize(x, row_amax=ra, tensor_amax=ta, y=True, yt=True)
    assert torch.equal(y4.view(torch.uint8), y_r.view(torch.uint8)) and torch.equal(ys4, ys_r)
    assert torch.equal(t4.view(torch.uint8), t_t.view(torch.uint8)) and torch.equal(ts4, ts_t)

    # folds: the same codes, the stored scales times the fold
    for kw, (by, bys, bt, bts) in (({"tensor_amax": ta}, (y2, ys2, t2, ts2)),
                                   ({"row_amax": ra, "col_amax": ca}, (y3, ys3, t3, ts3)),
                                   ({"row_amax": ra, "tensor_amax": ta}, (y4, ys4, t4, ts4))):
        y5, ys5, t5, ts5 = fp8_quantize(x, y=True, yt=True, y_fold=fy, yt_fold=ft, **kw)
        assert torch.equal(y5.view(torch.uint8), by.view(torch.uint8))
        assert torch.equal(t5.view(torch.uint8), bt.view(torch.uint8))
        torch.testing.assert_close(ys5, bys * fy, rtol=1e-6, atol=0)
        torch.testing.assert_close(ts5, bts * ft, rtol=1e-6, atol=0)
        y6, ys6, t6, ts6 = fp8_quantize(x, y=True, yt=True, y_fold=fy, **kw)  # one fold only
        torch.testing.assert_close(ys6, bys * fy, rtol=1e-6, atol=0)
        assert torch.equal(ts6, bts)

    # into wider, taller poisoned buffers: nothing outside the image is written
    ybuf = torch.full((rows + 16, cols + 32), POISON_BYTE, dtype=torch.uint8, device=DEV)
    tbuf = torch.full((cols + 16, rows + 48), POISON_BYTE, dtype=torch.uint8, device=DEV)
    yv, tv = ybuf.view(FP8)[:rows, :cols], tbuf.view(FP8)[:cols, :rows]
    y7, _, t7, _ = fp8_quantize(x, row_amax=ra, col_amax=ca, y=yv, yt=tv)
    assert y7 is yv and t7 is tv
    assert torch.equal(ybuf[:rows, :cols], y3.view(torch.uint8))
    assert torch.equal(tbuf[:cols, :rows], t3.view(torch.uint8))
    assert (ybuf[rows:] == POISON_BYTE).all() and (ybuf[:, cols:] == POISON_BYTE).all()
    assert (tbuf[cols:] == POISON_BYTE).all() and (tbuf[:, rows:] == POISON_BYTE).all()


def test_quantise_scales_turn_non_finite_with_their_amax():
    from kgs.ops import fp8_amax, fp8_quantize

    x = _matrix(48, 272, 5)
    x[7, 9], x[11, 20] = float("nan"), float("inf")
    ra, ca, ta = fp8_amax(x, rows=True, cols=True, tensor=True)
    _, ys, _, ts = fp8_quantize(x, row_amax=ra, col_amax=ca, y=True, yt=True)
    assert torch.isnan(ys[7]) and torch.isinf(ys[11]) and torch.isfinite(ys).sum() == 46
    assert torch.isnan(ts[9]) and torch.isinf(ts[20]) and torch.isfinite(ts).sum() == 270
    assert torch.isnan(fp8_quantize(x, tensor_amax=ta)[1]).all()


def test_bad_arguments_return_error_codes_and_launch_nothing():
    from kgs.ops import _lib

    lib, st = _lib.lib(), _lib.stream_handle(torch.device(DEV))
    rows, cols = 32, 48
    x = _randn(_gen(1), rows, cols + 8)
    ld = x.stride(0)
    P = 1234.0
    ra, ca, ta = (torch.full((n,), P, device=DEV) for n in (rows, cols, 1))
    y = torch.full((rows, cols), POISON_BYTE, dtype=torch.uint8, device=DEV)
    yt = torch.full((cols, rows), POISON_BYTE, dtype=torch.uint8, device=DEV)
    ys, yts = torch.full((rows,), P, device=DEV), torch.full((cols,), P, device=DEV)
    vp = ctypes.c_void_p

    def amax(r=rows, c=cols, ldx=ld, off=0, outs=True, out_off=0):
        o = [vp(t.data_ptr() + out_off) for t in (ra, ca, ta)] if outs else [None] * 3
        return lib.kgs_fp8_amax_bf16(x.data_ptr() + off, r, c, ldx, *o, st)

    def quant(r=rows, c=cols, ldx=ld, off=0, y_on=True, yt_on=True, ldy=cols, ldyt=rows, yoff=0, amaxes=True):
        am = [vp(t.data_ptr()) for t in (ra, ca, ta)] if amaxes else [None] * 3
        return lib.kgs_fp8_quant_bf16(x.data_ptr() + off, r, c, ldx, *am, vp(y.data_ptr() + yoff) if y_on else None, ldy,
                                      vp(ys.data_ptr()), vp(yt.data_ptr()) if yt_on else None, ldyt,
                                      vp(yts.data_ptr()), None, None, st)

    assert amax(r=24) == -1 and amax(c=40) == -1 and amax(c=64) == -1  # % 16; ld < cols
    assert amax(r=0) == -1
    assert amax(off=2) == -2 and amax(ldx=ld + 4) == -2 and amax(out_off=2) == -2
    assert amax(outs=False) == -3
    assert quant(r=24) == -1 and quant(c=40) == -1 and quant(c=64) == -1
    assert quant(ldy=32) == -1 and quant(ldyt=16) == -1
    assert quant(off=2) == -2 and quant(yoff=8) == -2 and quant(ldy=cols + 8) == -2 and quant(ldyt=rows + 8) == -2
    assert quant(y_on=False, yt_on=False) == -3 and quant(amaxes=False) == -3
    torch.cuda.synchronize()
    for t in (ra, ca, ta, ys, yts):
        assert (t == P).all()
    assert (y == POISON_BYTE).all() and (yt == POISON_BYTE).all()
    assert amax() == 0 and quant() == 0  # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert not (y == POISON_BYTE).all()


# ----------------------------------------------------------------------------
# linear

LINEAR_SHAPES = [(256, 256, 256), (48, 272, 80), (512, 768, 1024)]  # aligned GEMM, bounded GEMM, several tiles


def _operands(T, K, N, seed=0):
    g = _gen(seed)
    return (_randn(g, T, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, T, N), _randn(g, N, scale=0.5))


def _compose(x, w, dy, bias):
    """The recipe from the raw ops: returns the three products and, for each, the
    fp32 product of the kernels' own dequantised operands."""
    from kgs.ops import fp8_amax, fp8_quantize, gemm_fp8_rows

    w_amax = fp8_amax(w, tensor=True)[2]
    w8, sw, _, _ = fp8_quantize(w, tensor_amax=w_amax)
    x_row, _, x_ten = fp8_amax(x, rows=True, tensor=True)
    x8, xs, x8t, sx = fp8_quantize(x, row_amax=x_row, tensor_amax=x_ten, y=True, yt=True, y_fold=sw)
    y = gemm_fp8_rows(x8, xs, w8, 1.0, bias=bias)
    d_row, d_col, _ = fp8_amax(dy, rows=True, cols=True)
    dy8, dys, dy8t, dyts = fp8_quantize(dy, row_amax=d_row, col_amax=d_col, y=True, yt=True, y_fold=sw, yt_fold=sx)
    w8t = fp8_quantize(w, tensor_amax=w_amax, y=False, yt=True)[2]
    assert torch.equal(w8t.view(torch.uint8), w8.view(torch.uint8).T)
    dx = gemm_fp8_rows(dy8, dys, w8t, 1.0)
    dw = gemm_fp8_rows(dy8t, dyts, x8t, 1.0)
    # the stored row scales carry B's scale (the fold), so A's dequantised rows times B's codes is the product
    refs = {"y": (x8.float() * xs[:, None]) @ w8.float().T + (0 if bias is None else bias.float()),
            "dx": (dy8.float() * dys[:, None]) @ w8t.float().T,
            "dw": (dy8t.float() * dyts[:, None]) @ x8t.float().T}
    return {"y": y, "dx": dx, "dw": dw}, refs


def _fro(got, ref):
    return ((got.float() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("T,K,N", LINEAR_SHAPES)
def test_linear_fp8_products_composition_and_model(T, K, N):
    from kgs.ops import linear_fp8, ref_linear_fp8

    x, w, dy, bias = _operands(T, K, N, seed=T + N)
    got, refs = _compose(x, w, dy, bias)
    for k in ("y", "dx", "dw"):
        rel = ((got[k].float() - refs[k]).abs().max() / refs[k].abs().max()).item()
        print(f"{k} [{T},{K},{N}]: rel to the dequantised product {rel:.5f}")
        assert rel < 1e-2, (k, rel)

    # the autograd function is that composition, bit for bit
    xi, wi, bi = (t.clone().requires_grad_(True) for t in (x, w, bias))
    y = linear_fp8(xi, wi, bi)
    y.backward(dy)
    assert torch.equal(y, got["y"]) and torch.equal(xi.grad, got["dx"]) and torch.equal(wi.grad, got["dw"])
    assert torch.equal(bi.grad, dy.float().sum(0).bfloat16())

    # needs_input_grad: a product that is not wanted is not made, the others keep their bits
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    linear_fp8(xo, w).backward(dy)
    linear_fp8(x, wo).backward(dy)
    assert torch.equal(xo.grad, got["dx"]) and torch.equal(wo.grad, got["dw"])
    with torch.no_grad():
        assert torch.equal(linear_fp8(x, w, bias), got["y"])

    # against the torch model on the same device: errors against fp32 within 2 x the model's
    xm, wm, bm = (t.clone().requires_grad_(True) for t in (x, w, bias))
    ym = ref_linear_fp8(xm, wm, bm)
    ym.backward(dy)
    xf, wf, df = x.float(), w.float(), dy.float()
    f32 = {"y": xf @ wf.T + bias.float(), "dx": df @ wf, "dw": df.T @ xf}
    model = {"y": ym.detach(), "dx": xm.grad, "dw": wm.grad}
    for k in ("y", "dx", "dw"):
        e_kgs, e_model = _fro(got[k], f32[k]), _fro(model[k], f32[k])
        print(f"{k} [{T},{K},{N}]: against fp32, kgs {e_kgs:.4f} model {e_model:.4f}")
        assert e_kgs <= 2 * e_model, (k, e_kgs, e_model)


def test_linear_fp8_keeps_nan_and_inf_visible():
    from kgs.ops import linear_fp8

    T, K, N = 48, 272, 80
    x, w, dy, _ = _operands(T, K, N, seed=9)
    xi = x.clone()
    xi[5, 100] = float("inf")
    y = linear_fp8(xi, w)
    assert not torch.isfinite(y[5]).any() and torch.isfinite(y[:5]).all() and torch.isfinite(y[6:]).all()
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    d = dy.clone()
    d[7, 33] = float("nan")
    linear_fp8(xg, wg).backward(d)
    assert not torch.isfinite(xg.grad[7]).any() and not torch.isfinite(wg.grad[33]).any()
    keep_r, keep_c = torch.arange(T, device=DEV) != 7, torch.arange(N, device=DEV) != 33
    assert torch.isfinite(xg.grad[keep_r]).all() and torch.isfinite(wg.grad[keep_c]).all()


def test_linear_fp8_forward_and_backward_in_a_graph():
    from kgs.ops import linear_fp8

    T, K, N = 256, 256, 256
    x, w, dy, bias = _operands(T, K, N, seed=21)
    sx, sw, sb = (torch.zeros_like(t).requires_grad_(True) for t in (x, w, bias))
    sdy = torch.zeros_like(dy)

    def run():
        y = linear_fp8(sx, sw, sb)
        return (y, *torch.autograd.grad(y, (sx, sw, sb), sdy))

    run()  # warm up: the library and every allocation path, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    with torch.no_grad():
        for s, t in ((sx, x), (sw, w), (sb, bias), (sdy, dy)):
            s.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    xi, wi, bi = (t.clone().requires_grad_(True) for t in (x, w, bias))
    y = linear_fp8(xi, wi, bi)
    y.backward(dy)
    for got, want in zip(outs, (y, xi.grad, wi.grad, bi.grad)):
        assert torch.equal(got, want)
    del graph


# ----------------------------------------------------------------------------
# models

def _copy_rounded(dst, src):
    with torch.no_grad():
        for (n, p), (m, q) in zip(dst.named_parameters(), src.named_parameters()):
            assert n == m
            p.copy_(q.to(p.dtype))


def test_decoder_layer_fp8_gradients_against_an_fp32_copy():
    """test_decoder_layer_gradients_against_an_fp32_copy's rule with the fp8
    Linears: for both input gradients and every parameter gradient, the kgs
    layer's max error against an fp32 copy of the same rounded weights, over the
    reference's max, is at most 2x that of the torch model of the same recipe."""
    from kgs.models.decoder import DecoderLayer
    from kgs.ops import LinearFp8

    dim, nh, nkv, inter, b, s = 512, 4, 1, 1536, 2, 256
    g = _gen(3)
    x, d, dy1, dy2 = (_randn(g, b, s, dim) for _ in range(4))
    layers = {"kgs": DecoderLayer(dim, nh, nkv, inter, backend="kgs", device=DEV, linear="fp8"),
              "torch": DecoderLayer(dim, nh, nkv, inter, backend="torch", device=DEV, linear="fp8"),
              "fp32": DecoderLayer(dim, nh, nkv, inter, backend="torch", device=DEV, dtype=torch.float32)}
    assert all(isinstance(m, LinearFp8) for m in (layers["kgs"].qkv, layers["kgs"].o, layers["kgs"].gate_up,
                                                  layers["kgs"].down))
    with torch.no_grad():
        layers["kgs"].attn_norm.copy_(1 + 0.1 * torch.randn(dim, device=DEV, generator=g))
        layers["kgs"].mlp_norm.copy_(1 + 0.1 * torch.randn(dim, device=DEV, generator=g))
    _copy_rounded(layers["torch"], layers["kgs"])
    _copy_rounded(layers["fp32"], layers["kgs"])
    grads = {}
    for name, layer in layers.items():
        cast = (lambda t: t.float()) if name == "fp32" else (lambda t: t)
        xi, di = cast(x).clone().requires_grad_(True), cast(d).clone().requires_grad_(True)
        res, out = layer(xi, di)
        torch.autograd.backward([res, out], [cast(dy1), cast(dy2)])
        grads[name] = {"x": xi.grad.float(), "delta": di.grad.float(),
                       **{n: p.grad.float() for n, p in layer.named_parameters()}}
    assert len(grads["fp32"]) == 8
    for n, ref in grads["fp32"].items():
        mag = ref.abs().max().item()
        e_kgs = (grads["kgs"][n] - ref).abs().max().item() / mag
        e_model = (grads["torch"][n] - ref).abs().max().item() / mag
        print(f"{n}: kgs fp8 {e_kgs:.4f} torch fp8 {e_model:.4f}")
        assert e_kgs <= 2 * e_model, (n, e_kgs, e_model)


def test_decoder_lm_fp8_trains_with_adamw():
    """Eight steps of kgs.optim.AdamW on one fixed batch, the four projections of
    both layers in fp8: the loss stays finite and ends below where it started."""
    from kgs.models.decoder import DecoderLM
    from kgs.optim import AdamW, decay_groups

    vocab, dim, nl, nh, nkv, inter, b, s = 1024, 512, 2, 4, 1, 1536, 2, 128
    g = _gen(11)
    tokens = torch.randint(0, vocab, (b, s), device=DEV, generator=g)
    targets = tokens.roll(-1, 1).clone()
    targets[:, -1] = -100
    lm = DecoderLM(vocab, dim, nl, nh, nkv, inter, backend="kgs", device=DEV, linear="fp8")
    opt = AdamW(decay_groups(lm, 0.1), lr=1e-3, max_grad_norm=1.0, backend="kgs")
    losses = []
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        loss = lm.loss(tokens, targets)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("loss", [f"{v:.4f}" for v in losses])
    assert all(torch.isfinite(torch.tensor(losses)))
    assert opt.skipped_steps == 0 and opt.step_count == 8
    assert losses[-1] < losses[0]
