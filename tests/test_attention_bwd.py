"""CPU tests of the differentiable attention op's reference and argument
checks (the kernels themselves: tests/test_attention_bwd_gpu.py)."""
import math

import pytest
import torch

from kgs.ops.transformer import (attention_qkv_backward, attention_qkv_lse, flash_attention_qkv,
                                 ref_attention_qkv_backward)


def _loss64(qkv, dout, b, s, nh, nkv, hd, causal):
    """sum(attention(qkv) * dout) in float64, written out (no SDPA): its
    finite differences are the gradients the reference must return."""
    q = qkv[:, :nh * hd].reshape(b, s, nh, hd).transpose(1, 2)
    k = qkv[:, nh * hd:(nh + nkv) * hd].reshape(b, s, nkv, hd).transpose(1, 2)
    v = qkv[:, (nh + nkv) * hd:].reshape(b, s, nkv, hd).transpose(1, 2)
    k, v = (t.repeat_interleave(nh // nkv, dim=1) for t in (k, v))
    sc = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if causal:
        sc = sc.masked_fill(torch.triu(torch.ones(s, s, dtype=torch.bool), 1), float("-inf"))
    o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(b * s, nh * hd)
    return (o * dout).sum()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s", [4, 7])
def test_reference_backward_matches_float64_finite_differences(s, causal):
    b, nh, nkv, hd = 1, 2, 1, 8
    g = torch.Generator().manual_seed(5 + s)
    qkv = torch.randn(b * s, (nh + 2 * nkv) * hd, generator=g, dtype=torch.float64)
    dout = torch.randn(b * s, nh * hd, generator=g, dtype=torch.float64)
    got = ref_attention_qkv_backward(qkv, dout, b, s, nh, nkv, head_dim=hd, causal=causal)
    assert got.dtype == torch.float32 and got.shape == qkv.shape
    # central differences of the float64 loss: error O(eps^2 f''') ~ 1e-8
    eps = 1e-4
    fd = torch.empty_like(qkv)
    flat, out = qkv.reshape(-1), fd.reshape(-1)
    for i in range(flat.numel()):
        x0 = flat[i].item()
        flat[i] = x0 + eps
        hi = _loss64(qkv, dout, b, s, nh, nkv, hd, causal)
        flat[i] = x0 - eps
        lo = _loss64(qkv, dout, b, s, nh, nkv, hd, causal)
        flat[i] = x0
        out[i] = (hi - lo) / (2 * eps)
    # the reference works in fp32: 2^-24 relative per operation over a few dozen operations
    assert (got.double() - fd).abs().max().item() < 1e-4 * max(1.0, fd.abs().max().item())


@pytest.mark.parametrize("causal", [True, False])
def test_reference_backward_sums_a_kv_heads_group(causal):
    """dk / dv of a KV head are the sums of the gradients its query heads would
    give it alone (each head with its own copy of that K / V)."""
    b, s, nh, nkv, hd = 2, 6, 4, 2, 8
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(b * s, (nh + 2 * nkv) * hd, generator=g)
    dout = torch.randn(b * s, nh * hd, generator=g)
    got = ref_attention_qkv_backward(qkv, dout, b, s, nh, nkv, head_dim=hd, causal=causal)
    rep = nh // nkv
    q, k, v = qkv[:, :nh * hd], qkv[:, nh * hd:(nh + nkv) * hd], qkv[:, (nh + nkv) * hd:]
    kx = k.reshape(-1, nkv, 1, hd).expand(-1, nkv, rep, hd).reshape(-1, nh * hd)
    vx = v.reshape(-1, nkv, 1, hd).expand(-1, nkv, rep, hd).reshape(-1, nh * hd)
    mha = ref_attention_qkv_backward(torch.cat((q, kx, vx), 1), dout, b, s, nh, nh, head_dim=hd, causal=causal)
    dq, dk, dv = mha[:, :nh * hd], mha[:, nh * hd:2 * nh * hd], mha[:, 2 * nh * hd:]
    torch.testing.assert_close(got[:, :nh * hd], dq, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got[:, nh * hd:(nh + nkv) * hd],
                               dk.reshape(-1, nkv, rep, hd).sum(2).reshape(-1, nkv * hd), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got[:, (nh + nkv) * hd:], dv.reshape(-1, nkv, rep, hd).sum(2).reshape(-1, nkv * hd),
                               rtol=1e-5, atol=1e-5)


def _args(b=1, s=128, nh=2, nkv=1, dtype=torch.bfloat16):
    qkv = torch.zeros(b * s, (nh + 2 * nkv) * 128, dtype=dtype)
    out = torch.zeros(b * s, nh * 128, dtype=dtype)
    lse = torch.zeros(b * nh, s)
    return qkv, out, lse


def test_ops_reject_cpu_tensors():
    qkv, out, lse = _args()
    with pytest.raises(ValueError, match="GPU"):
        flash_attention_qkv(qkv, 1, 128, 2, 1)
    with pytest.raises(ValueError, match="GPU"):
        flash_attention_qkv(qkv.requires_grad_(True), 1, 128, 2, 1)
    with pytest.raises(ValueError, match="GPU"):
        attention_qkv_lse(qkv, 1, 128, 2, 1)
    with pytest.raises(ValueError, match="GPU"):
        attention_qkv_backward(qkv, out, out, lse, 1, 128, 2, 1)


def test_ops_reject_wrong_dtypes():
    qkv, out, lse = _args()
    f32, _, _ = _args(dtype=torch.float32)
    for fn in (flash_attention_qkv, attention_qkv_lse):
        with pytest.raises(TypeError):
            fn(f32, 1, 128, 2, 1)
    with pytest.raises(TypeError):
        attention_qkv_backward(f32, out, out, lse, 1, 128, 2, 1)
    with pytest.raises(TypeError):
        attention_qkv_backward(qkv, out.float(), out, lse, 1, 128, 2, 1)
    with pytest.raises(TypeError):
        attention_qkv_backward(qkv, out, out.float(), lse, 1, 128, 2, 1)
    with pytest.raises(TypeError):
        attention_qkv_backward(qkv, out, out, lse.double(), 1, 128, 2, 1)
    with pytest.raises(TypeError):
        attention_qkv_backward(qkv, out, out, lse, 1, 128, 2, 1, dqkv=qkv.float())


def test_ops_reject_shape_mismatches():
    qkv, out, lse = _args()
    for fn in (flash_attention_qkv, attention_qkv_lse):
        with pytest.raises(ValueError, match="128"):
            fn(torch.zeros(192, 512, dtype=torch.bfloat16), 1, 192, 2, 1)  # seq % 128
        with pytest.raises(ValueError, match="kv_heads"):
            fn(qkv, 1, 128, 3, 2)
        with pytest.raises(ValueError, match="shape"):
            fn(qkv, 2, 128, 2, 1)  # rows
        with pytest.raises(ValueError, match="shape"):
            fn(qkv, 1, 128, 4, 1)  # columns
    with pytest.raises(ValueError, match="out shape"):
        attention_qkv_backward(qkv, out[:, :128], out, lse, 1, 128, 2, 1)
    with pytest.raises(ValueError, match="dout shape"):
        attention_qkv_backward(qkv, out, out[:64], lse, 1, 128, 2, 1)
    with pytest.raises(ValueError, match="lse"):
        attention_qkv_backward(qkv, out, out, lse[:1], 1, 128, 2, 1)
    with pytest.raises(ValueError, match="dqkv shape"):
        attention_qkv_backward(qkv, out, out, lse, 1, 128, 2, 1, dqkv=qkv[:, :384])
    with pytest.raises(ValueError, match="row-major"):
        attention_qkv_backward(qkv, out, out.t().contiguous().t(), lse, 1, 128, 2, 1)


def test_ops_are_exported_next_to_attention_qkv():
    import kgs.ops

    for name in ("attention_qkv", "attention_qkv_lse", "attention_qkv_backward", "flash_attention_qkv"):
        assert callable(getattr(kgs.ops, name))


def test_attention_block_torch_backend_trains_on_cpu():
    """The torch backend is the fp32 reference copy the GPU test measures
    against: it runs on the CPU, is causal, and gives every parameter a gradient."""
    from kgs.models.attn_block import AttentionBlock

    blk = AttentionBlock(64, 4, 2, backend="torch", dtype=torch.float32)
    x = torch.randn(2, 8, 64, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    y = blk(x)
    assert y.shape == x.shape
    y[:, 3].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in blk.parameters())
    assert x.grad[:, :4].abs().sum() > 0 and x.grad[:, 4:].abs().sum() == 0  # causal: later tokens unseen
    with pytest.raises(ValueError):
        AttentionBlock(64, 4, 2, backend="kgs")  # head_dim 16
