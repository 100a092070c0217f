"""GPU tests of the training glue (native/kernels/train_ops.hip): the backward
kernels of the norm and of SwiGLU, RoPE's backward on the forward kernel, the
softmax cross-entropy, the autograd ops over them, DecoderLayer and DecoderLM.

Every kernel evaluates its formula once in fp32 and rounds once to bf16, so every
element is held to ``|out - ref64| <= 2^-7 |ref64| + atol`` against the float64
reference on the same bf16 inputs, with the atol of each quantity stated at its
test. A column sum (the norm's dw) adds the textbook bound of an fp32 sum of n
terms in any order, ``n 2^-24 sum |term|``, computed here in float64."""
import ctypes
import functools

import pytest
import torch

# the criterion and the poisoned buffers are shared with the forward kernels' tests
from forward_refs import POISON, poison_intact as _poison_intact, wide as _wide, within as _within

pytestmark = pytest.mark.gpu

DEV = "cuda"
LP_TOL = 1e-4  # tests/test_logit_ops_gpu.py: an fp32 exp-sum's logprob, valid for |reference| <= 64


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, device=DEV, generator=g)).bfloat16()


def _zero_bits(t):
    return int(t.view(torch.int16).count_nonzero()) == 0


# ----------------------------------------------------------------------------
# rmsnorm_backward

NORM_COLS = (512, 1536, 4096, 8192)
NORM_ROWS = (1, 5, 2053)  # 2053: more rows than the stage-1 grid has waves (2048), so some waves own two


@functools.lru_cache(maxsize=None)
def _norm_case(rows, cols, with_dres):
    """Inputs, the kernel's outputs and the float64 reference of one case, computed
    once and shared by the tests (nothing below modifies them)."""
    from kgs.ops.transformer import ref_rmsnorm_backward, rmsnorm_backward

    g = _gen(rows * 31 + cols + with_dres)
    x, dy = _randn(g, rows, cols), _randn(g, rows, cols)
    w = (1 + 0.1 * torch.randn(cols, device=DEV, generator=g)).bfloat16()
    dres = _randn(g, rows, cols) if with_dres else None
    dx, dw = rmsnorm_backward(x, w, dy, dres)
    rdx, rdw = ref_rmsnorm_backward(x, w, dy, dres)
    xf = x.double()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)
    dw_atol = rows * 2.0 ** -24 * (dy.double() * xf * r).abs().sum(0)
    torch.cuda.synchronize()
    return {"x": x, "w": w, "dy": dy, "dres": dres, "dx": dx, "dw": dw, "rdx": rdx, "rdw": rdw, "dw_atol": dw_atol}


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("rows", NORM_ROWS)
@pytest.mark.parametrize("cols", NORM_COLS)
def test_rmsnorm_backward_against_float64(cols, rows, with_dres):
    """dx: atol 1e-4 at unit-scale inputs. dw[j]: rows 2^-24 sum_rows |dy x r|."""
    c = _norm_case(rows, cols, with_dres)
    assert c["dx"].shape == (rows, cols) and c["dw"].shape == (cols,)
    assert c["dx"].dtype == torch.bfloat16 and c["dw"].dtype == torch.bfloat16
    _within(c["dx"], c["rdx"], 1e-4, "dx")
    _within(c["dw"], c["rdw"], c["dw_atol"], "dw")


def _raw_norm_bwd(x, w, dy, dres, dx, dw, ws_ptr, rows=None, cols=None, eps=1e-5, x_off=0):
    from kgs.ops import _lib

    return _lib.lib().kgs_rmsnorm_bwd_bf16(
        x.data_ptr() + x_off, w.data_ptr(), dy.data_ptr(), ctypes.c_void_p(0 if dres is None else dres.data_ptr()),
        dx.data_ptr(), dw.data_ptr(), ctypes.c_void_p(ws_ptr), x.shape[0] if rows is None else rows,
        x.shape[1] if cols is None else cols, x.stride(0), dy.stride(0), 0 if dres is None else dres.stride(0),
        dx.stride(0), eps, _lib.stream_handle(x.device))


def _norm_ws(rows, cols):
    from kgs.ops import _lib

    nbytes = _lib.lib().kgs_rmsnorm_bwd_workspace(rows, cols)
    assert nbytes >= 16
    return torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("rows,cols,with_dres", [(5, 1536, True), (2053, 512, False)])
def test_rmsnorm_backward_strided_rows_and_poison_around_dx(rows, cols, with_dres):
    """Row strides wider than cols for x, dy, dres and dx: the contiguous call's bits,
    and nothing written outside dx's [rows, cols]."""
    c = _norm_case(rows, cols, with_dres)
    x, _ = _wide(c["x"], pad=64)
    dy, _ = _wide(c["dy"], pad=128)
    dres = _wide(c["dres"], pad=192)[0] if with_dres else None
    dx, buf = _wide(torch.zeros_like(c["dx"]), pad=72)
    dw = torch.full((cols + 16,), POISON, dtype=torch.bfloat16, device=DEV)
    assert _raw_norm_bwd(x, c["w"], dy, dres, dx, dw[8:8 + cols], _norm_ws(rows, cols).data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, c["dx"]) and torch.equal(dw[8:8 + cols], c["dw"])
    assert _poison_intact(buf, rows, cols)
    assert (dw[:8] == POISON).all() and (dw[8 + cols:] == POISON).all()


@pytest.mark.parametrize("rows,cols", [(5, 1536), (2053, 4096)])
def test_rmsnorm_backward_zero_dy_passes_the_residual_gradient_through(rows, cols):
    from kgs.ops.transformer import rmsnorm_backward

    c = _norm_case(rows, cols, True)
    dx, dw = rmsnorm_backward(c["x"], c["w"], torch.zeros_like(c["dy"]), c["dres"])
    assert torch.equal(dx.view(torch.int16), c["dres"].view(torch.int16))
    assert _zero_bits(dw)


# ----------------------------------------------------------------------------
# silu_mul_backward

SILU_SHAPES = ((1, 8), (5, 1536), (1027, 1536), (5, 14336))


@functools.lru_cache(maxsize=None)
def _silu_case(rows, inter):
    from kgs.ops.transformer import ref_silu_mul_backward, silu_mul_backward

    g = _gen(rows + inter)
    gu = torch.cat((_randn(g, rows, inter, scale=2.0), _randn(g, rows, inter)), dim=1)  # gates at scale 2: both tails
    dh = _randn(g, rows, inter)
    dgu = silu_mul_backward(gu, dh)
    ref = ref_silu_mul_backward(gu, dh)
    torch.cuda.synchronize()
    return {"gu": gu, "dh": dh, "dgu": dgu, "ref": ref}


@pytest.mark.parametrize("rows,inter", SILU_SHAPES)
def test_silu_mul_backward_against_float64(rows, inter):
    c = _silu_case(rows, inter)
    assert c["dgu"].shape == (rows, 2 * inter) and c["dgu"].dtype == torch.bfloat16
    _within(c["dgu"], c["ref"], 1e-5, "dgu")


@pytest.mark.parametrize("rows,inter", SILU_SHAPES)
def test_silu_mul_backward_strided_and_poisoned(rows, inter):
    from kgs.ops.transformer import silu_mul_backward

    c = _silu_case(rows, inter)
    gu, _ = _wide(c["gu"], pad=64)
    dh, _ = _wide(c["dh"], pad=128)
    out, buf = _wide(torch.zeros_like(c["dgu"]), pad=72)
    got = silu_mul_backward(gu, dh, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, c["dgu"])
    assert _poison_intact(buf, rows, 2 * inter)


def test_silu_mul_backward_zero_dh_gives_zero_bits():
    from kgs.ops.transformer import silu_mul_backward

    c = _silu_case(1027, 1536)
    assert _zero_bits(silu_mul_backward(c["gu"], torch.zeros_like(c["dh"])))


# ----------------------------------------------------------------------------
# rope_qkv

ROPE = dict(seq=384, nh=4, nkv=1, hd=128, batch=2)


@functools.lru_cache(maxsize=None)
def _rope_case():
    from kgs.ops.transformer import rope_tables

    s, nh, nkv, hd, b = (ROPE[k] for k in ("seq", "nh", "nkv", "hd", "batch"))
    g = _gen(17)
    qkv = _randn(g, b * s, (nh + 2 * nkv) * hd)
    dout = _randn(g, b * s, (nh + 2 * nkv) * hd)
    cos, sin = rope_tables(s, hd, 10000.0, DEV)
    return {"qkv": qkv, "dout": dout, "cos": cos, "sin": sin, "rot": nh + nkv, "hd": hd, "seq": s}


@pytest.mark.parametrize("leaf", [True, False])
def test_rope_qkv_forward_and_gradient_are_the_inference_kernels_bits(leaf):
    from kgs.ops.transformer import ref_rope_qkv_backward, rope_qkv, rope_qkv_

    c = _rope_case()
    cos, sin, rot, hd, seq = c["cos"], c["sin"], c["rot"], c["hd"], c["seq"]
    want = rope_qkv_(c["qkv"].clone(), cos, sin, rot, hd, seq)
    src = c["qkv"].clone().requires_grad_(True)
    inp = src if leaf else src * 1  # a leaf is rotated on a copy, a non-leaf in place
    out = rope_qkv(inp, cos, sin, rot, hd, seq)
    assert torch.equal(out, want)
    assert torch.equal(src, c["qkv"])  # the leaf itself is never touched
    assert (out.data_ptr() == inp.data_ptr()) == (not leaf)
    dout = c["dout"].clone()
    out.backward(dout)
    assert torch.equal(dout, c["dout"])  # the incoming gradient is not rotated in place
    grad = src.grad
    assert torch.equal(grad, rope_qkv_(c["dout"].clone(), cos, -sin, rot, hd, seq))
    assert torch.equal(grad[:, rot * hd:], c["dout"][:, rot * hd:])  # pass-through columns
    _within(grad, ref_rope_qkv_backward(c["dout"], cos, sin, rot, hd, seq), 1e-5, "rope grad")


def test_rope_qkv_without_a_gradient_is_the_inference_op():
    from kgs.ops.transformer import rope_qkv, rope_qkv_

    c = _rope_case()
    a, b = c["qkv"].clone(), c["qkv"].clone()
    out = rope_qkv(a, c["cos"], c["sin"], c["rot"], c["hd"], c["seq"])
    assert out.grad_fn is None and not out.requires_grad and out.data_ptr() == a.data_ptr()
    assert torch.equal(out, rope_qkv_(b, c["cos"], c["sin"], c["rot"], c["hd"], c["seq"]))


# ----------------------------------------------------------------------------
# cross-entropy

XENT = {(1, 8): ("zero",),
        (5, 520): ("zero", "last", "ignored", "peaky", "scale8"),
        (3, 4104): ("last", "ignored", "peaky"),
        (4, 128256): ("zero", "peaky", "scale8", "ignored")}


@functools.lru_cache(maxsize=None)
def _xent_case(rows, cols):
    """Rows by kind: N(0, 1) with target 0 / cols - 1; an ignored row (-100); a
    peaky row (target logit 60, the rest N(0, 1)); a row at scale 8 (target cols - 1).
    ld > cols: the logits are a view into a wider buffer."""
    from kgs.ops.transformer import (cross_entropy_rows, cross_entropy_rows_backward, ref_cross_entropy_rows,
                                     ref_cross_entropy_rows_backward)

    g = _gen(rows + cols)
    x = torch.randn(rows, cols, device=DEV, generator=g)
    tg = []
    for i, kind in enumerate(XENT[(rows, cols)]):
        tg.append({"zero": 0, "last": cols - 1, "ignored": -100, "peaky": cols // 2 + 1, "scale8": cols - 1}[kind])
        if kind == "peaky":
            x[i, tg[-1]] = 60.0
        if kind == "scale8":
            x[i] *= 8
    logits, _ = _wide(x.bfloat16(), pad=64)
    target = torch.tensor(tg, dtype=torch.int64, device=DEV)
    grow = torch.randn(rows, device=DEV, generator=g) / rows
    loss, lse = cross_entropy_rows(logits, target)
    dl = cross_entropy_rows_backward(logits, target, lse, grow)
    rloss, rlse = ref_cross_entropy_rows(logits, target)
    rdl = ref_cross_entropy_rows_backward(logits, target, rlse, grow)
    torch.cuda.synchronize()
    return {"logits": logits, "target": target, "grow": grow, "loss": loss, "lse": lse, "dl": dl, "rloss": rloss,
            "rlse": rlse, "rdl": rdl, "kinds": XENT[(rows, cols)]}


@pytest.mark.parametrize("rows,cols", list(XENT))
def test_cross_entropy_rows_against_float64(rows, cols):
    c = _xent_case(rows, cols)
    assert c["loss"].dtype == torch.float32 and c["lse"].dtype == torch.float32
    assert c["rlse"].abs().max() <= 64 and c["rloss"].abs().max() <= 64  # where LP_TOL is derived
    e_loss = (c["loss"].double() - c["rloss"]).abs().max().item()
    e_lse = (c["lse"].double() - c["rlse"]).abs().max().item()
    print(f"loss err {e_loss:.3e}, lse err {e_lse:.3e}")
    assert e_loss <= LP_TOL and e_lse <= LP_TOL, (e_loss, e_lse)
    for i, kind in enumerate(c["kinds"]):
        if kind == "ignored":
            assert c["loss"][i].item() == 0.0 and torch.isfinite(c["lse"][i])


@pytest.mark.parametrize("rows,cols", list(XENT))
def test_cross_entropy_rows_backward_against_float64(rows, cols):
    """atol 1e-4 |grow[row]|; every gradient row sums to 0 within cols 2^-9 max|row|."""
    c = _xent_case(rows, cols)
    dl = c["dl"]
    assert dl.shape == (rows, cols) and dl.dtype == torch.bfloat16
    _within(dl, c["rdl"], 1e-4 * c["grow"].double().abs()[:, None], "dlogits")
    sums, peak = dl.double().sum(1).abs(), dl.double().abs().max(1).values
    print("row sums", sums.tolist(), "bounds", (cols * 2.0 ** -9 * peak).tolist())
    assert (sums <= cols * 2.0 ** -9 * peak).all()
    for i, kind in enumerate(c["kinds"]):
        if kind == "ignored":
            assert _zero_bits(dl[i].contiguous())
        else:
            assert dl[i, c["target"][i]].item() <= 0 or c["grow"][i].item() <= 0  # p - 1 <= 0 at the target


@pytest.mark.parametrize("rows,cols", [(5, 520), (4, 128256)])
def test_cross_entropy_rows_backward_into_a_wider_poisoned_buffer(rows, cols):
    from kgs.ops.transformer import cross_entropy_rows_backward

    c = _xent_case(rows, cols)
    out, buf = _wide(torch.zeros_like(c["dl"]), pad=72)
    got = cross_entropy_rows_backward(c["logits"], c["target"], c["lse"], c["grow"], out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, c["dl"])
    assert _poison_intact(buf, rows, cols)


# ----------------------------------------------------------------------------
# repeatability, graph capture

def _replays(capture, want):
    """Capture ``capture()`` in one graph, replay it twice over zeroed outputs, compare bits."""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = capture()
    for _ in range(2):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, exp in zip(outs, want):
            assert torch.equal(got, exp)


@pytest.mark.parametrize("rows,cols,with_dres", [(2053, 4096, True), (5, 8192, False)])
def test_rmsnorm_repeatable_and_graph_capturable(rows, cols, with_dres):
    from kgs.ops.transformer import add_rmsnorm, rmsnorm_backward

    c = _norm_case(rows, cols, with_dres)
    dx, dw = rmsnorm_backward(c["x"], c["w"], c["dy"], c["dres"])
    assert torch.equal(dx, c["dx"]) and torch.equal(dw, c["dw"])
    y = add_rmsnorm(c["x"], None, c["w"])

    def capture():
        return (add_rmsnorm(c["x"], None, c["w"]), *rmsnorm_backward(c["x"], c["w"], c["dy"], c["dres"]))

    _replays(capture, (y, c["dx"], c["dw"]))


def test_silu_mul_repeatable_and_graph_capturable():
    from kgs.ops.transformer import silu_mul, silu_mul_backward

    c = _silu_case(1027, 1536)
    assert torch.equal(silu_mul_backward(c["gu"], c["dh"]), c["dgu"])
    h = silu_mul(c["gu"])
    _replays(lambda: (silu_mul(c["gu"]), silu_mul_backward(c["gu"], c["dh"])), (h, c["dgu"]))


def test_rope_repeatable_and_graph_capturable():
    from kgs.ops.transformer import rope_qkv_

    c = _rope_case()
    cos, sin, rot, hd, seq = c["cos"], c["sin"], c["rot"], c["hd"], c["seq"]
    nsin = -sin
    fwd = rope_qkv_(c["qkv"].clone(), cos, sin, rot, hd, seq)
    bwd = rope_qkv_(c["dout"].clone(), cos, nsin, rot, hd, seq)
    assert torch.equal(bwd, rope_qkv_(c["dout"].clone(), cos, nsin, rot, hd, seq))

    def capture():
        return (rope_qkv_(c["qkv"].clone(), cos, sin, rot, hd, seq),
                rope_qkv_(c["dout"].clone(), cos, nsin, rot, hd, seq))

    _replays(capture, (fwd, bwd))


@pytest.mark.parametrize("rows,cols", [(5, 520), (4, 128256)])
def test_cross_entropy_repeatable_and_graph_capturable(rows, cols):
    from kgs.ops.transformer import cross_entropy_rows, cross_entropy_rows_backward

    c = _xent_case(rows, cols)
    assert torch.equal(cross_entropy_rows_backward(c["logits"], c["target"], c["lse"], c["grow"]), c["dl"])

    def capture():
        loss, lse = cross_entropy_rows(c["logits"], c["target"])
        return loss, lse, cross_entropy_rows_backward(c["logits"], c["target"], lse, c["grow"])

    _replays(capture, (c["loss"], c["lse"], c["dl"]))


# ----------------------------------------------------------------------------
# autograd ops

@pytest.mark.parametrize("with_d", [False, True])
def test_rmsnorm_residual_backward_is_the_raw_ops_bits(with_d):
    from kgs.ops.transformer import add_rmsnorm, rmsnorm_backward, rmsnorm_residual

    c = _norm_case(5, 1536, True)
    x = c["x"].clone().requires_grad_(True)
    d = c["dy"].clone().requires_grad_(True) if with_d else None  # any [rows, cols] tensor serves as the delta
    w = c["w"].clone().requires_grad_(True)
    res, y = rmsnorm_residual(x, d, w)
    assert torch.equal(x, c["x"])  # out of place
    stream = c["x"].clone()
    want_y = add_rmsnorm(stream, None if d is None else d.detach(), c["w"])  # the in-place inference op
    assert torch.equal(res, stream) and torch.equal(y, want_y)
    assert with_d or res.data_ptr() == x.data_ptr()  # no delta: res is x itself
    dres, dy = c["dres"], c["dx"]  # any two gradients
    torch.autograd.backward([res, y], [dres, dy])
    dx, dw = rmsnorm_backward(stream, c["w"], dy, dres)
    assert torch.equal(x.grad, dx) and torch.equal(w.grad, dw)
    if with_d:
        assert torch.equal(d.grad, dx)
    # no gradient wanted: the inference kernel, nothing saved
    res0, y0 = rmsnorm_residual(c["x"], None if d is None else d.detach(), c["w"])
    assert y0.grad_fn is None and res0.grad_fn is None and torch.equal(y0, y) and torch.equal(res0, stream)


def test_swiglu_backward_is_the_raw_ops_bits():
    from kgs.ops.transformer import silu_mul, swiglu

    c = _silu_case(5, 1536)
    gu = c["gu"].clone().requires_grad_(True)
    h = swiglu(gu)
    assert torch.equal(h, silu_mul(c["gu"]))
    h.backward(c["dh"])
    assert torch.equal(gu.grad, c["dgu"])
    h0 = swiglu(c["gu"])
    assert h0.grad_fn is None and not h0.requires_grad and torch.equal(h0, h)


def test_softmax_cross_entropy_backward_is_the_raw_ops_bits():
    from kgs.ops.transformer import softmax_cross_entropy

    c = _xent_case(5, 520)
    logits = c["logits"].clone().requires_grad_(True)  # a contiguous copy: the bits must not depend on ld
    loss = softmax_cross_entropy(logits, c["target"])
    assert torch.equal(loss, c["loss"])
    loss.backward(c["grow"])
    assert torch.equal(logits.grad, c["dl"])
    # the usual reduction: the mean over the rows that are not ignored, taken in torch
    logits.grad = None
    live = (c["target"] >= 0).sum()
    (softmax_cross_entropy(logits, c["target"]).sum() / live).backward()
    assert _zero_bits(logits.grad[2].contiguous()) and logits.grad.abs().sum() > 0
    l0 = softmax_cross_entropy(c["logits"], c["target"])
    assert l0.grad_fn is None and not l0.requires_grad and torch.equal(l0, c["loss"])


# ----------------------------------------------------------------------------
# raw entries

def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    from kgs.ops import _lib

    lib = _lib.lib()
    c = _norm_case(5, 1536, True)
    rows, cols = 5, 1536
    dx, dw = torch.full_like(c["x"], POISON), torch.full_like(c["w"], POISON)
    ws = torch.full((rows * cols,), POISON, device=DEV)
    args = (c["x"], c["w"], c["dy"], c["dres"], dx, dw)
    assert _raw_norm_bwd(*args, ws.data_ptr(), cols=1000) == -1    # KGS_ERR_SHAPE: cols % 512
    assert _raw_norm_bwd(*args, ws.data_ptr(), cols=8704) == -1    # cols > 8192
    assert _raw_norm_bwd(*args, ws.data_ptr(), x_off=2) == -2      # KGS_ERR_ALIGN: pointer not 16-byte aligned
    assert _raw_norm_bwd(*args, 0) == -2                           # null workspace
    assert lib.kgs_rmsnorm_bwd_workspace(5, 1000) == -1
    assert lib.kgs_rmsnorm_bwd_workspace(5, 1536) == 2 * 1536 * 4  # ceil(5 / 4) partial rows
    assert lib.kgs_rmsnorm_bwd_workspace(1 << 20, 512) == 512 * 512 * 4  # the grid's cap

    s = _silu_case(5, 1536)
    dgu = torch.full_like(s["gu"], POISON)
    st = _lib.stream_handle(dgu.device)

    def silu(inter=1536, off=0, ld=3072):
        return lib.kgs_silu_mul_bwd_bf16(s["gu"].data_ptr() + off, s["dh"].data_ptr(), dgu.data_ptr(), 5, inter, ld,
                                         1536, 3072, st)

    assert silu(inter=1532) == -1 and silu(inter=2048) == -1  # I % 8; ld < 2 I
    assert silu(off=2) == -2 and silu(ld=3076) == -2          # misaligned pointer; stride % 8

    x = _xent_case(5, 520)
    loss, lse = torch.full((5,), POISON, device=DEV), torch.full((5,), POISON, device=DEV)
    dl = torch.full((5, 520), POISON, dtype=torch.bfloat16, device=DEV)
    ld = x["logits"].stride(0)

    def fwd(cols=520, off=0, lse_ptr=None):
        return lib.kgs_xent_fwd_bf16(x["logits"].data_ptr() + off, x["target"].data_ptr(), loss.data_ptr(),
                                     ctypes.c_void_p(lse.data_ptr() if lse_ptr is None else lse_ptr), 5, cols, ld, st)

    def bwd(cols=520, off=0, ldd=520):
        return lib.kgs_xent_bwd_bf16(x["logits"].data_ptr() + off, x["target"].data_ptr(), x["lse"].data_ptr(),
                                     x["grow"].data_ptr(), dl.data_ptr(), 5, cols, ld, ldd, st)

    assert fwd(cols=516) == -1 and fwd(cols=1024) == -1  # cols % 8; ld < cols
    assert fwd(off=2) == -2 and fwd(lse_ptr=0) == -2
    assert bwd(cols=516) == -1 and bwd(ldd=512) == -1
    assert bwd(off=2) == -2 and bwd(ldd=524) == -2
    torch.cuda.synchronize()
    for t in (dx, dw, ws, dgu, loss, lse, dl):
        assert (t == POISON).all()


# ----------------------------------------------------------------------------
# models

def _copy_rounded(dst, src):
    with torch.no_grad():
        for (n, p), (m, q) in zip(dst.named_parameters(), src.named_parameters()):
            assert n == m
            p.copy_(q.to(p.dtype))


def test_decoder_layer_gradients_against_an_fp32_copy():
    """The rule of test_attention_block_gradients_against_an_fp32_copy: for both input
    gradients and every parameter gradient, the kgs backend's max error against
    an fp32 copy holding the same rounded weights, over the reference's max, is at
    most 2x the torch bf16 backend's, which itself must be under 2e-2."""
    from kgs.models.decoder import DecoderLayer

    dim, nh, nkv, inter, b, s = 512, 4, 1, 1536, 2, 256
    g = _gen(3)
    x, d, dy1, dy2 = (_randn(g, b, s, dim) for _ in range(4))
    layers = {"kgs": DecoderLayer(dim, nh, nkv, inter, backend="kgs", device=DEV),
              "torch": DecoderLayer(dim, nh, nkv, inter, backend="torch", device=DEV),
              "fp32": DecoderLayer(dim, nh, nkv, inter, backend="torch", device=DEV, dtype=torch.float32)}
    with torch.no_grad():  # norm weights off 1, so that their gradients and the w factor are exercised
        layers["kgs"].attn_norm.copy_(1 + 0.1 * torch.randn(dim, device=DEV, generator=g))
        layers["kgs"].mlp_norm.copy_(1 + 0.1 * torch.randn(dim, device=DEV, generator=g))
    _copy_rounded(layers["torch"], layers["kgs"])
    _copy_rounded(layers["fp32"], layers["kgs"])
    assert torch.equal(layers["kgs"].qkv.weight, layers["torch"].qkv.weight)
    grads = {}
    for name, layer in layers.items():
        cast = (lambda t: t.float()) if name == "fp32" else (lambda t: t)
        xi, di = cast(x).clone().requires_grad_(True), cast(d).clone().requires_grad_(True)
        res, out = layer(xi, di)
        assert res.shape == (b, s, dim) and out.shape == (b, s, dim)
        torch.autograd.backward([res, out], [cast(dy1), cast(dy2)])
        grads[name] = {"x": xi.grad.float(), "delta": di.grad.float(),
                       **{n: p.grad.float() for n, p in layer.named_parameters()}}
    assert len(grads["fp32"]) == 8
    for n, ref in grads["fp32"].items():
        mag = ref.abs().max().item()
        e_kgs = (grads["kgs"][n] - ref).abs().max().item() / mag
        e_base = (grads["torch"][n] - ref).abs().max().item() / mag
        print(f"{n}: kgs {e_kgs:.4f} torch {e_base:.4f}")
        assert e_base < 2e-2, (n, e_base)
        assert e_kgs <= 2 * e_base, (n, e_kgs, e_base)


def test_decoder_lm_sgd_steps_track_the_fp32_copy():
    """Eight SGD steps on one fixed seeded batch for kgs, torch bf16 and an fp32 copy
    of the same rounded initial weights: the kgs loss falls, and at every step
    |loss_kgs - loss_fp32| <= 2 |loss_torch - loss_fp32| + 1e-4."""
    from kgs.models.decoder import DecoderLM

    vocab, dim, nl, nh, nkv, inter, b, s, lr = 1024, 512, 2, 4, 1, 1536, 2, 128, 0.1
    g = _gen(11)
    tokens = torch.randint(0, vocab, (b, s), device=DEV, generator=g)
    targets = tokens.roll(-1, 1).clone()
    targets[:, -1] = -100  # the last position has no next token
    models = {"kgs": DecoderLM(vocab, dim, nl, nh, nkv, inter, backend="kgs", device=DEV),
              "torch": DecoderLM(vocab, dim, nl, nh, nkv, inter, backend="torch", device=DEV),
              "fp32": DecoderLM(vocab, dim, nl, nh, nkv, inter, backend="torch", device=DEV, dtype=torch.float32)}
    assert all(torch.equal(p, q) for p, q in zip(models["kgs"].parameters(), models["torch"].parameters()))
    _copy_rounded(models["fp32"], models["kgs"])
    losses = {}
    for name, lm in models.items():
        losses[name] = []
        for _ in range(8):
            lm.zero_grad(set_to_none=True)
            loss = lm.loss(tokens, targets)
            loss.backward()
            with torch.no_grad():
                for p in lm.parameters():
                    p.add_(p.grad, alpha=-lr)
            losses[name].append(loss.item())
        print(name, [f"{v:.4f}" for v in losses[name]])
    assert all(torch.isfinite(torch.tensor(v)).all() for v in losses.values())
    assert losses["kgs"][7] < losses["kgs"][0]
    for i in range(8):
        e_kgs = abs(losses["kgs"][i] - losses["fp32"][i])
        e_base = abs(losses["torch"][i] - losses["fp32"][i])
        assert e_kgs <= 2 * e_base + 1e-4, (i, e_kgs, e_base)
