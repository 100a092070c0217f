"""GPU tests of the sliding-window training attention kernels (native/kernels/attention_window.hip).

The reference is the masked attention math in float64 (query i sees keys max(0, i - W + 1) .. i). Accuracy
follows tests/test_attention_bwd_gpu.py: the baseline is the same math in plain torch bf16 ops on the same GPU;
the kernels' max error over the reference's max must be within 2x the baseline's, and the baseline itself
under 2e-2; lse within 1e-3 of the float64 logsumexp."""
import ctypes
import functools
import math

import pytest
import torch

from kgs.models.decoder import DecoderLM
from kgs.ops import _lib
from kgs.ops.transformer import attention_qkv, attention_qkv_backward, attention_qkv_lse, flash_attention_qkv

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 128

# W=1 self only; 33 both edges in a wave's diagonal tile; 64 / 65 the lower edge on a tile boundary and one past
# it (a wave's lowest tile wholly masked for some rows); 200 the edge crosses q-blocks
CASES = [(1, 256, 2, 2, w) for w in (1, 33, 64, 65, 128, 200)] + [(2, 384, 4, 1, w) for w in (65, 129, 192)] + \
        [(1, 1024, 4, 2, 256)]  # steady state, key blocks whose query sweep ends before S


def _groups(x, nh, nkv):
    return {"dq": x[:, :nh * HD], "dk": x[:, nh * HD:(nh + nkv) * HD], "dv": x[:, (nh + nkv) * HD:(nh + 2 * nkv) * HD]}


def _math(qkv, dout, b, s, nh, nkv, window, low):
    """({out, dq, dk, dv}, lse) by autograd: in float64, or (low) the bf16 baseline, which rounds P to bf16."""
    leaf = (qkv if low else qkv.double()).clone().requires_grad_(True)
    q = leaf[:, :nh * HD].reshape(b, s, nh, HD).transpose(1, 2)
    k = leaf[:, nh * HD:(nh + nkv) * HD].reshape(b, s, nkv, HD).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    v = leaf[:, (nh + nkv) * HD:].reshape(b, s, nkv, HD).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    sc = q @ k.transpose(-1, -2)
    sc = (sc.float() if low else sc) / math.sqrt(HD)
    d = torch.arange(s, device=DEV)[:, None] - torch.arange(s, device=DEV)[None, :]
    sc = sc.masked_fill((d < 0) | (d >= window), float("-inf"))
    o = (torch.softmax(sc, -1).to(leaf.dtype) @ v).transpose(1, 2).reshape(b * s, nh * HD)
    o.backward(dout.to(o.dtype))
    return {"out": o.detach(), **_groups(leaf.grad, nh, nkv)}, torch.logsumexp(sc.detach(), -1).reshape(b * nh, s)


@functools.lru_cache(maxsize=None)
def _case(b, s, nh, nkv, window, qscale=1.0):
    """A case's forward + backward, float64 reference and bf16 baseline, computed once and shared (never modified)."""
    g = torch.Generator(device=DEV).manual_seed(b + s + nh)
    qkv = torch.randn(b * s, (nh + 2 * nkv) * HD, device=DEV, generator=g)
    qkv[:, :nh * HD] *= qscale
    qkv, dout = qkv.bfloat16(), torch.randn(b * s, nh * HD, device=DEV, generator=g).bfloat16()
    out, lse = attention_qkv_lse(qkv, b, s, nh, nkv, window=window)
    dqkv = attention_qkv_backward(qkv, out, dout, lse, b, s, nh, nkv, window=window)
    torch.cuda.synchronize()
    return {"qkv": qkv, "dout": dout, "out": out, "lse": lse, "dqkv": dqkv,
            "ref": _math(qkv, dout, b, s, nh, nkv, window, False), "base": _math(qkv, dout, b, s, nh, nkv, window, True)}


@pytest.mark.parametrize("b,s,nh,nkv,window", CASES)
def test_forward_and_gradients_against_float64(b, s, nh, nkv, window):
    c = _case(b, s, nh, nkv, window)
    (ref, rl), (bas, _) = c["ref"], c["base"]
    assert torch.equal(c["out"], attention_qkv(c["qkv"], b, s, nh, nkv, window=window))
    assert c["lse"].dtype == torch.float32 and c["lse"].shape == (b * nh, s)
    for x in (c["out"], c["lse"], c["dqkv"]):
        assert torch.isfinite(x.float()).all()
    lse_err = (c["lse"].double() - rl).abs().max().item()
    got, errs = {"out": c["out"], **_groups(c["dqkv"], nh, nkv)}, {}
    for n, r in ref.items():
        mag = r.abs().max().item()
        if mag == 0:
            # W = 1: P is one-hot on the row's own key, so dS = P (dP - delta) and with it dq and dk are exactly
            # zero. The kernels' dP and delta are two fp32 sums of the same 128 exact products dO V, each within
            # 127 2^-24 sum |dO V| of the true sum; dS is their difference times the scale and multiplies one
            # element of K (dq) or Q (dk); 1.01 covers P's and the bf16 result's rounding
            sums = (c["dout"].float().abs() * c["qkv"][:, (nh + nkv) * HD:].float().abs()).reshape(-1, HD).sum(-1)
            bound = 1.01 * 2 * 127 * 2.0 ** -24 * sums.max().item() / math.sqrt(HD) * c["qkv"].float().abs().max().item()
            assert window == 1 and nh == nkv and n in ("dq", "dk") and got[n].float().abs().max().item() <= bound, (n, bound)
            continue
        errs[n] = ((got[n].double() - r).abs().max().item() / mag, (bas[n].double() - r).abs().max().item() / mag)
    print(f"lse err {lse_err:.3e}; err (kgs, baseline):", {n: (f"{e[0]:.4f}", f"{e[1]:.4f}") for n, e in errs.items()})
    assert lse_err < 1e-3, lse_err
    for n, (e_kgs, e_base) in errs.items():
        assert e_base < 2e-2 and e_kgs <= 2 * e_base, (n, e_kgs, e_base)  # a bad baseline cannot hide a failure


@pytest.mark.parametrize("window", [256, 263])
def test_a_window_that_covers_the_sequence_is_the_causal_op(window):
    b, s, nh, nkv = 1, 256, 2, 2
    c = _case(b, s, nh, nkv, 65)
    want_o, want_l = attention_qkv_lse(c["qkv"], b, s, nh, nkv)
    want_g = attention_qkv_backward(c["qkv"], want_o, c["dout"], want_l, b, s, nh, nkv)
    out, lse = attention_qkv_lse(c["qkv"], b, s, nh, nkv, window=window)
    dqkv = attention_qkv_backward(c["qkv"], out, c["dout"], lse, b, s, nh, nkv, window=window)
    assert torch.equal(out, want_o) and torch.equal(lse, want_l) and torch.equal(dqkv, want_g)


@pytest.mark.parametrize("row", [5, 200])
def test_one_row_of_dout_reaches_only_its_own_query_and_its_window_of_keys(row):
    b, s, nh, nkv, window = 1, 384, 2, 2, 65
    c = _case(b, s, nh, nkv, window)
    dout = torch.zeros_like(c["dout"])
    dout[row] = c["dout"][row]
    g = _groups(attention_qkv_backward(c["qkv"], c["out"], dout, c["lse"], b, s, nh, nkv, window=window)
                .view(torch.int16), nh, nkv)
    lo = max(0, row - 64)
    assert (g["dq"][:row] == 0).all() and (g["dq"][row + 1:] == 0).all() and g["dq"][row].count_nonzero() > 0
    for n in ("dk", "dv"):
        assert (g[n][:lo] == 0).all() and (g[n][row + 1:] == 0).all()
        assert (g[n][lo:row + 1].count_nonzero(dim=1) > 0).all()


def test_gradients_of_peaky_scores():
    """q x 8: P is near one-hot and the deferred maximum trails the true one."""
    b, s, nh, nkv = 2, 256, 4, 1
    c = _case(b, s, nh, nkv, 65, 8.0)
    got, ref = _groups(c["dqkv"].double(), nh, nkv), c["ref"][0]
    for x in (c["out"], c["lse"], c["dqkv"]):
        assert torch.isfinite(x.float()).all()
    for n in ("dq", "dk", "dv"):
        err, mag = (got[n] - ref[n]).abs().max().item(), ref[n].abs().max().item()
        print(f"{n}: err {err:.4f} mag {mag:.2f}")
        assert err < 4e-2 * max(1.0, mag), (n, err, mag)


@pytest.mark.parametrize("b,s,nh,nkv,window", [(2, 384, 4, 1, 65), (1, 256, 2, 2, 200)])
def test_repeatable_and_graph_capturable(b, s, nh, nkv, window):
    c = _case(b, s, nh, nkv, window)
    out, lse = attention_qkv_lse(c["qkv"], b, s, nh, nkv, window=window)
    again = attention_qkv_backward(c["qkv"], out, c["dout"], lse, b, s, nh, nkv, window=window)
    assert torch.equal(out, c["out"]) and torch.equal(lse, c["lse"]) and torch.equal(again, c["dqkv"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = attention_qkv_lse(c["qkv"], b, s, nh, nkv, window=window)
        dqkv = attention_qkv_backward(c["qkv"], out, c["dout"], lse, b, s, nh, nkv, window=window)
    for _ in range(2):
        for x in (out, lse, dqkv):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, c["out"]) and torch.equal(lse, c["lse"]) and torch.equal(dqkv, c["dqkv"])


def test_autograd_op_and_strided_operands():
    b, s, nh, nkv, window = 2, 384, 4, 1, 65
    c = _case(b, s, nh, nkv, window)
    leaf = c["qkv"].clone().requires_grad_(True)
    y = flash_attention_qkv(leaf, b, s, nh, nkv, window=window)
    y.backward(c["dout"])
    assert torch.equal(y, c["out"]) and torch.equal(leaf.grad, c["dqkv"])
    y0 = flash_attention_qkv(c["qkv"], b, s, nh, nkv, window=window)
    assert y0.grad_fn is None and not y0.requires_grad
    assert torch.equal(y0, attention_qkv(c["qkv"], b, s, nh, nkv, window=window))
    # a strided dout and a wider poisoned dqkv
    t, qc, w = b * s, nh * HD, (nh + 2 * nkv) * HD
    wide = torch.full((t, qc + 128), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, 64:64 + qc] = c["dout"]
    poison, buf = 1234.0, torch.full((t + 3, w + 256), 1234.0, dtype=torch.bfloat16, device=DEV)
    attention_qkv_backward(c["qkv"], c["out"], wide[:, 64:64 + qc], c["lse"], b, s, nh, nkv, window=window,
                           dqkv=buf[:, 128:128 + w + 64])
    assert torch.equal(buf[:t, 128:128 + w], c["dqkv"])
    assert (buf[:, :128] == poison).all() and (buf[:, 128 + w:] == poison).all() and (buf[t:] == poison).all()


def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    b, s, nh, nkv = 1, 256, 2, 1
    c = _case(2, 384, 4, 1, 65)  # any valid device buffers of at least this size
    qkv, out, dout, lse = c["qkv"], c["out"], c["dout"], c["lse"]
    poison = 1234.0
    dqkv, o2, ws = torch.full_like(qkv, poison), torch.full_like(out, poison), torch.full((b * nh * s,), poison, device=DEV)
    ld, st = qkv.stride(0), _lib.stream_handle(qkv.device)
    ko, vo = nh * HD * 2, (nh + nkv) * HD * 2
    qp, dp = qkv.data_ptr(), dqkv.data_ptr()

    def bwd(S=s, q_off=0, ws_ptr=ws.data_ptr(), window=65):
        return _lib.lib().kgs_attn_win_bwd_bf16(
            qp + q_off, qp + ko, qp + vo, out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dp, dp + ko, dp + vo,
            ctypes.c_void_p(ws_ptr), b, S, nh, nkv, HD, ld, ld, ld, out.stride(0), dout.stride(0), ld, ld, ld, 0.125,
            1, window, st)

    def fwd(S=s, q_off=0, window=65):
        return _lib.lib().kgs_attn_win_fwd_bf16(qp + q_off, qp + ko, qp + vo, o2.data_ptr(), None, b, S, nh, nkv, HD,
                                                ld, ld, ld, o2.stride(0), 0.125, 1, window, st)

    assert bwd(S=192) == -1 and fwd(S=192) == -1        # KGS_ERR_SHAPE: S % 128
    assert bwd(window=0) == -1 and fwd(window=0) == -1  # KGS_ERR_SHAPE: window < 1
    assert bwd(q_off=2) == -2 and fwd(q_off=2) == -2    # KGS_ERR_ALIGN: pointer not 16-byte aligned
    assert bwd(ws_ptr=0) == -2                          # KGS_ERR_ALIGN: null workspace
    torch.cuda.synchronize()
    assert (dqkv == poison).all() and (ws == poison).all() and (o2 == poison).all()


def test_decoder_lm_with_windowed_layers_against_an_fp32_copy():
    """Loss and gradients against an fp32 copy with the same rounded weights: within 2x the torch bf16 backend's."""
    vocab, b, s = 512, 2, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    tok, tgt = (torch.randint(0, vocab, (b, s), device=DEV, generator=g) for _ in range(2))
    kw = dict(vocab=vocab, dim=512, layers=2, heads=4, kv_heads=2, inter=1024, window=64, global_every=2, device=DEV)
    models = {"kgs": DecoderLM(backend="kgs", **kw), "torch": DecoderLM(backend="torch", **kw),
              "fp32": DecoderLM(backend="torch", dtype=torch.float32, **kw)}
    assert [m.window for m in models["kgs"].layers] == [64, None]
    res = {}
    for name, model in models.items():
        with torch.no_grad():
            for p, q in zip(model.parameters(), models["kgs"].parameters()):
                p.copy_(q.to(p.dtype))
        loss = model.loss(tok, tgt)
        loss.backward()
        res[name] = {"loss": loss.detach().float().reshape(1), **{n: p.grad.float() for n, p in model.named_parameters()}}
    for n, ref in res["fp32"].items():
        mag = ref.abs().max().item()
        e_kgs = (res["kgs"][n] - ref).abs().max().item() / mag
        e_base = (res["torch"][n] - ref).abs().max().item() / mag
        print(f"{n}: kgs {e_kgs:.4f} torch {e_base:.4f}")
        assert e_base < 2e-2 and e_kgs <= 2 * e_base, (n, e_kgs, e_base)
