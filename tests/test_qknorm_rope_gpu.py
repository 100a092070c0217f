"""GPU tests of QK-norm fused with RoPE (native/kernels/qknorm_rope.hip). The per-element
criteria against float64 are the ones tests/test_qknorm_rope.py derives and shows to
admit an fp32 evaluation."""
import ctypes
import functools

import pytest
import torch

from forward_refs import POISON, poison_intact, wide
from test_qknorm_rope import EPS, SEQ, check_backward, check_forward

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (T, H, HKV). (5, 4, 1): 5 head rows per token, so a wave's eight slots straddle tokens and
# both regions end mid-wave. 6571: 1643 32-row trips of q rows and 411 of k rows against the
# 1638 + 409 (forward) and 722 + 180 (backward) workgroups the default grid caps give the
# two regions at 4 q heads per k head, so some waves make two trips in both kernels.
SHAPES = ((1, 1, 1), (5, 4, 1), (6571, 8, 2))
CASES = [(*s, e) for s in SHAPES for e in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(t, h, hkv, explicit):
    """Inputs and the kernels' outputs of one case, computed once and shared by the
    tests (nothing below modifies them)."""
    from kgs.ops.qknorm_rope import qknorm_rope_, qknorm_rope_backward
    from kgs.ops.transformer import rope_tables

    g = torch.Generator(device=DEV).manual_seed(17 * t + h + explicit)
    nqk, width = (h + hkv) * 128, (h + 2 * hkv) * 128
    c = {"t": t, "h": h, "hkv": hkv, "nqk": nqk}
    c["qkv"] = torch.randn(t, width, device=DEV, generator=g).bfloat16()
    c["dy"] = torch.randn(t, width, device=DEV, generator=g).bfloat16()
    c["wq"], c["wk"] = ((1 + 0.1 * torch.randn(128, device=DEV, generator=g)).bfloat16() for _ in range(2))
    c["cos"], c["sin"] = rope_tables(SEQ, 128, 10000.0, DEV)
    c["pos"] = torch.randint(0, SEQ, (t,), device=DEV, generator=g).int() if explicit else None
    c["p"] = c["pos"] if explicit else (torch.arange(t, device=DEV) % SEQ).int()
    c["args"] = (c["wq"], c["wk"], c["cos"], c["sin"], h, hkv, SEQ, c["pos"], EPS)
    c["out"], c["save"], dy = c["qkv"].clone(), torch.empty(t, nqk, dtype=torch.bfloat16, device=DEV), c["dy"].clone()
    qknorm_rope_(c["out"], *c["args"], save=c["save"])
    c["dx"], c["dwq"], c["dwk"] = qknorm_rope_backward(dy, c["save"], *c["args"])
    assert torch.equal(dy, c["dy"])  # dy is only read
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("t,h,hkv,explicit", CASES)
def test_forward_against_float64(t, h, hkv, explicit):
    """q, k: atol 2^-20 (|n1 c| + |n2 s|). v: untouched. save: the input's q and k bits."""
    c = _case(t, h, hkv, explicit)
    check_forward(c["out"], c["save"], c["qkv"], *c["args"][:4], h, hkv, c["p"])


@pytest.mark.parametrize("t,h,hkv,explicit", CASES)
def test_backward_against_float64(t, h, hkv, explicit):
    """dx: DX_ATOL; its v columns: dy's bits. dwq, dwk: n 2^-24 sum |g nh| over the n summed rows."""
    c = _case(t, h, hkv, explicit)
    check_backward(c["dx"], c["dwq"], c["dwk"], c["dy"], c["qkv"], *c["args"][:4], h, hkv, c["p"])


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t if isinstance(t, int) else t.data_ptr())


def _raw_fwd(c, qkv, save, wq=None, hd=128, seq=SEQ, pos="case", off=0):
    from kgs.ops import _lib

    return _lib.lib().kgs_qknorm_rope_fwd_bf16(
        _ptr(qkv.data_ptr() + off), _ptr(save), _ptr(c["wq"] if wq is None else wq), _ptr(c["wk"]), _ptr(c["cos"]),
        _ptr(c["sin"]), _ptr(c["pos"] if pos == "case" else pos), c["t"], c["h"], c["hkv"], hd, qkv.stride(0),
        0 if save is None else save.stride(0), seq, SEQ, EPS, 0, _lib.stream_handle(qkv.device))


def _raw_bwd(c, dy, save, dx, dwq, dwk, ws, wq=None, hd=128, seq=SEQ, pos="case", off=0):
    from kgs.ops import _lib

    return _lib.lib().kgs_qknorm_rope_bwd_bf16(
        _ptr(dy.data_ptr() + off), _ptr(save), _ptr(c["wq"] if wq is None else wq), _ptr(c["wk"]), _ptr(c["cos"]),
        _ptr(c["sin"]), _ptr(c["pos"] if pos == "case" else pos), _ptr(dx), _ptr(dwq), _ptr(dwk), _ptr(ws), c["t"],
        c["h"], c["hkv"], hd, dy.stride(0), save.stride(0), dx.stride(0), seq, SEQ, EPS, 0,
        _lib.stream_handle(dy.device))


def _ws(c):
    from kgs.ops import _lib

    return torch.empty(_lib.lib().kgs_qknorm_rope_bwd_workspace(c["t"], c["h"], c["hkv"]) // 4, device=DEV)


@pytest.mark.parametrize("t,h,hkv,explicit", [(5, 4, 1, True), (6571, 8, 2, False)])
def test_strided_rows_and_poison_around_every_output(t, h, hkv, explicit):
    c = _case(t, h, hkv, explicit)
    nqk, width = c["nqk"], c["dy"].shape[1]
    qkv, qbuf = wide(c["qkv"], pad=64)
    save, sbuf = wide(torch.zeros_like(c["save"]), pad=72)
    dy, ybuf = wide(c["dy"], pad=128)
    dx, xbuf = wide(torch.zeros_like(c["dx"]), pad=192)
    dw = torch.full((2 * 128 + 24,), POISON, dtype=torch.bfloat16, device=DEV)
    dwq, dwk = dw[8:136], dw[144:272]
    assert _raw_fwd(c, qkv, save) == 0
    assert _raw_bwd(c, dy, save, dx, dwq, dwk, _ws(c)) == 0
    torch.cuda.synchronize()
    assert torch.equal(qkv, c["out"]) and torch.equal(save, c["save"]) and torch.equal(dy, c["dy"])
    assert torch.equal(dx, c["dx"]) and torch.equal(dwq, c["dwq"]) and torch.equal(dwk, c["dwk"])
    assert all(poison_intact(b, t, n) for b, n in ((qbuf, width), (sbuf, nqk), (xbuf, width), (ybuf, width)))
    assert (dw[:8] == POISON).all() and (dw[136:144] == POISON).all() and (dw[272:] == POISON).all()


@pytest.mark.parametrize("t,h,hkv,explicit", [(5, 4, 1, False), (6571, 8, 2, True)])
def test_repeatable_and_capturable(t, h, hkv, explicit):
    from kgs.ops.qknorm_rope import qknorm_rope_, qknorm_rope_backward

    c = _case(t, h, hkv, explicit)
    again = qknorm_rope_backward(c["dy"], c["save"], *c["args"])
    assert all(torch.equal(a, b) for a, b in zip(again, (c["dx"], c["dwq"], c["dwk"])))
    buf, save = torch.empty_like(c["qkv"]), torch.empty_like(c["save"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.copy_(c["qkv"])
        qknorm_rope_(buf, *c["args"], save=save)
        got = qknorm_rope_backward(c["dy"], save, *c["args"])
    for _ in range(3):
        for o in (buf, save, *got):
            o.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, c["out"]) and torch.equal(save, c["save"])
        assert all(torch.equal(a, b) for a, b in zip(got, (c["dx"], c["dwq"], c["dwk"])))


@pytest.mark.parametrize("leaf", [True, False])
def test_autograd_op_gives_the_raw_entries_bits(leaf):
    from kgs.ops import qknorm_rope

    c = _case(5, 4, 1, True)
    wq, wk = c["wq"].clone().requires_grad_(True), c["wk"].clone().requires_grad_(True)
    x = c["qkv"].clone().requires_grad_(True)
    inp = x if leaf else x * 1  # a non-leaf that is no view: normalised in place, marked dirty
    out = qknorm_rope(inp, wq, wk, *c["args"][2:])
    assert (out.data_ptr() == inp.data_ptr()) == (not leaf)
    out.backward(c["dy"])
    assert torch.equal(out, c["out"]) and torch.equal(x.detach(), c["qkv"])
    assert torch.equal(x.grad, c["dx"]) and torch.equal(wq.grad, c["dwq"]) and torch.equal(wk.grad, c["dwk"])
    plain = c["qkv"].clone()
    same = qknorm_rope(plain, *c["args"])  # no gradient wanted: the raw forward, in place, nothing saved
    assert same is plain and same.grad_fn is None and torch.equal(same, c["out"])


def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    c = _case(5, 4, 1, False)
    qkv, save, dx = (torch.full_like(c[k], POISON) for k in ("qkv", "save", "dx"))
    dwq, dwk, ws = torch.full_like(c["dwq"], POISON), torch.full_like(c["dwk"], POISON), torch.full_like(_ws(c), POISON)
    bad = (({"hd": 64}, -1), ({"off": 2}, -2), ({"wq": c["wq"].data_ptr() + 2}, -2),  # shape; misaligned pointers
           ({"wq": 0}, -2), ({"seq": 0, "pos": None}, -3))                             # a null weight; no positions
    for kw, rc in bad:
        assert _raw_fwd(c, qkv, save, **kw) == rc, kw
        assert _raw_bwd(c, c["dy"], c["save"], dx, dwq, dwk, ws, **kw) == rc, kw
    assert _raw_bwd(c, c["dy"], c["save"], dx, dwq, dwk, None) == -2  # a null workspace
    torch.cuda.synchronize()
    for o in (qkv, save, dx, dwq, dwk, ws):
        assert (o == POISON).all()


def test_decoder_layer_qk_norm_gradients_against_an_fp32_copy():
    """test_decoder_layer_gradients_against_an_fp32_copy's shape and rule with qk_norm on:
    every gradient, q_norm's and k_norm's included, within 2x the torch bf16 backend's
    error against an fp32 copy of the same rounded weights, itself under 2e-2."""
    from kgs.models.decoder import DecoderLayer

    dim, nh, nkv, inter, b, s = 512, 4, 1, 1536, 2, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    x, d, dy1, dy2 = (torch.randn(b, s, dim, device=DEV, generator=g).bfloat16() for _ in range(4))
    kw = {"device": DEV, "qk_norm": True}
    layers = {"kgs": DecoderLayer(dim, nh, nkv, inter, backend="kgs", **kw),
              "torch": DecoderLayer(dim, nh, nkv, inter, backend="torch", **kw),
              "fp32": DecoderLayer(dim, nh, nkv, inter, backend="torch", dtype=torch.float32, **kw)}
    with torch.no_grad():  # norm weights off 1, so that their gradients and the w factor are exercised
        for p in (layers["kgs"].attn_norm, layers["kgs"].mlp_norm, layers["kgs"].q_norm, layers["kgs"].k_norm):
            p.copy_(1 + 0.1 * torch.randn(p.shape, device=DEV, generator=g))
        for other in ("torch", "fp32"):
            for p, q in zip(layers[other].parameters(), layers["kgs"].parameters()):
                p.copy_(q.to(p.dtype))
    grads = {}
    for name, layer in layers.items():
        cast = (lambda z: z.float()) if name == "fp32" else (lambda z: z)
        xi, di = cast(x).clone().requires_grad_(True), cast(d).clone().requires_grad_(True)
        torch.autograd.backward(list(layer(xi, di)), [cast(dy1), cast(dy2)])
        grads[name] = {"x": xi.grad.float(), "delta": di.grad.float(),
                       **{n: p.grad.float() for n, p in layer.named_parameters()}}
    assert len(grads["fp32"]) == 10 and {"q_norm", "k_norm"} <= set(grads["kgs"])
    for n, ref in grads["fp32"].items():
        mag = ref.abs().max().item()
        e_kgs = (grads["kgs"][n] - ref).abs().max().item() / mag
        e_base = (grads["torch"][n] - ref).abs().max().item() / mag
        print(f"{n}: kgs {e_kgs:.4f} torch {e_base:.4f}")
        assert e_base < 2e-2, (n, e_base)
        assert e_kgs <= 2 * e_base, (n, e_kgs, e_base)
