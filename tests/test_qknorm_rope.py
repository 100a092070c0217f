"""CPU tests of QK-norm fused with RoPE: the float64 statements of
kgs/ops/qknorm_rope.py against torch autograd, the per-element criteria the GPU
tests apply (tests/test_qknorm_rope_gpu.py imports them from here) shown to admit
the fp32 evaluation rounded once to bf16, and the models' ``qk_norm`` switch.

The criteria are forward_refs' ``|out - ref64| <= 2^-7 |ref64| + atol``. Forward:
atol = 2^-20 (|n1 c| + |n2 s|), the rotation's two products: at most 8 fp32
roundings on n (the sum of squares, the rsqrt, two products) on top of ref_rope's
2^-23 cancellation term. dwq / dwk: an fp32 sum of n terms in any order, n 2^-24
sum |g nh|.

dx was first held to atol = 2^-20 (|r gw| + |r nh mean(gw nh)|), 8 roundings on each of
its two terms. That bound does not admit an fp32 evaluation: at (6571, 8, 2) torch's
own fp32 ``ref_qknorm_rope_backward`` rounded to bf16 misses it (least margin -2.5e-9),
and its fp32 error is over 4x that atol on one element in 10^4 and up to 480x where the
rotation cancels. Two fp32 errors are missing from it, and DX_ATOL adds exactly these:

* g = dy1 c + dy2 s is a sum of two products, so its fp32 error is 2^-23 of their size
  P = |dy1 c| + |dy2 s| (ref_rope's term), not of |g|: where the products cancel, |g w|
  says nothing about the error. The first term carries |w| P in place of |g w|.
* mean(gw nh) is an fp32 sum of 128 terms that are each off by that much. In any order
  its error is at most 128 2^-24 mean(|w| P |nh|), the bound the dw columns use, and it
  reaches dx through the factor r nh.

The fp32 evaluation uses a third of DX_ATOL at every shape here and at (6571, 8, 2)."""
import pytest
import torch

from forward_refs import ref_rope, within

SEQ, EPS = 384, 1e-6


def _pieces(qkv, wq, wk, h, hkv, eps):
    """float64: the q and k head rows [T, h + hkv, 128], their r, and every head's weight."""
    x = qkv[:, :(h + hkv) * 128].double().reshape(qkv.shape[0], h + hkv, 128)
    w = torch.cat((wq.double().expand(h, 128), wk.double().expand(hkv, 128)))
    return x, torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps), w


def check_forward(out, save, qkv, wq, wk, cos, sin, h, hkv, p, eps=EPS):
    """``out``, ``save``: what the forward made of ``qkv`` at the positions ``p`` (int [T])."""
    t, nqk = qkv.shape[0], (h + hkv) * 128
    x, r, w = _pieces(qkv, wq, wk, h, hkv, eps)
    ref, atol = ref_rope((x * r * w).reshape(t, nqk), cos, sin, h + hkv, 128, p)
    within(out[:, :nqk], ref, 8 * atol, "qknorm_rope")
    assert torch.equal(out[:, nqk:], qkv[:, nqk:]), "v columns"
    assert torch.equal(save, qkv[:, :nqk]), "save"
    return ref


def check_backward(dx, dwq, dwk, dy, qkv, wq, wk, cos, sin, h, hkv, p, eps=EPS):
    from kgs.ops.qknorm_rope import ref_qknorm_rope_backward

    t, nqk = qkv.shape[0], (h + hkv) * 128
    rdx, rdwq, rdwk = ref_qknorm_rope_backward(dy, qkv, wq, wk, cos, sin, h, hkv, SEQ, p, eps)
    x, r, w = _pieces(qkv, wq, wk, h, hkv, eps)
    g, a23 = ref_rope(dy, cos, -sin, h + hkv, 128, p)  # the transposed rotation and 2^-23 P
    g, wp = g.reshape(t, h + hkv, 128), w.abs() * (2.0 ** 23 * a23).reshape(t, h + hkv, 128)
    nhat, gw = x * r, g * w
    atol = 2.0 ** -20 * r * (wp + (nhat * (gw * nhat).mean(-1, keepdim=True)).abs()) + \
        128 * 2.0 ** -24 * r * nhat.abs() * (wp * nhat.abs()).mean(-1, keepdim=True)  # DX_ATOL, see the module
    within(dx[:, :nqk], rdx[:, :nqk], atol.reshape(t, nqk), "dx")
    assert torch.equal(dx[:, nqk:], dy[:, nqk:]), "dv"
    mag = (g * nhat).abs()
    within(dwq, rdwq, t * h * 2.0 ** -24 * mag[:, :h].sum((0, 1)), "dwq")
    within(dwk, rdwk, t * hkv * 2.0 ** -24 * mag[:, h:].sum((0, 1)), "dwk")


def _inputs(t, h, hkv, explicit, dtype=torch.bfloat16):
    from kgs.ops.transformer import rope_tables

    g = torch.Generator().manual_seed(17 * t + h + explicit)
    qkv, dy = (torch.randn(t, (h + 2 * hkv) * 128, generator=g).to(dtype) for _ in range(2))
    wq, wk = ((1 + 0.1 * torch.randn(128, generator=g)).to(dtype) for _ in range(2))
    cos, sin = rope_tables(SEQ, 128, 10000.0, "cpu")
    pos = torch.randint(0, SEQ, (t,), generator=g).int() if explicit else None
    return qkv, dy, wq, wk, cos, sin, pos


@pytest.mark.parametrize("explicit", [False, True])
def test_reference_backward_is_autograd_through_the_reference_forward(explicit):
    from kgs.ops.qknorm_rope import ref_qknorm_rope, ref_qknorm_rope_backward

    t, h, hkv = 3, 2, 1
    qkv, dy, wq, wk, cos, sin, pos = _inputs(t, h, hkv, explicit, torch.float64)
    leaves = [z.clone().requires_grad_(True) for z in (qkv, wq, wk)]
    out = ref_qknorm_rope(*leaves, cos, sin, h, hkv, SEQ, pos, EPS)
    want = torch.autograd.grad(out, leaves, dy)
    got = ref_qknorm_rope_backward(dy, qkv, wq, wk, cos, sin, h, hkv, SEQ, pos, EPS)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("t,h,hkv", [(1, 1, 1), (5, 4, 1), (300, 8, 2)])
def test_criteria_admit_the_fp32_evaluation(t, h, hkv, explicit):
    from kgs.ops.qknorm_rope import ref_qknorm_rope, ref_qknorm_rope_backward

    qkv, dy, wq, wk, cos, sin, pos = _inputs(t, h, hkv, explicit)
    p = pos if explicit else (torch.arange(t) % SEQ).int()
    args = (wq, wk, cos, sin, h, hkv, SEQ, pos, EPS)
    out = ref_qknorm_rope(qkv, *args, dtype=torch.float32).to(torch.bfloat16)
    ref = check_forward(out, qkv[:, :(h + hkv) * 128], qkv, wq, wk, cos, sin, h, hkv, p)
    torch.testing.assert_close(ref_qknorm_rope(qkv, *args)[:, :(h + hkv) * 128], ref, rtol=1e-12, atol=1e-12)
    dx, dwq, dwk = (z.to(torch.bfloat16) for z in ref_qknorm_rope_backward(dy, qkv, *args, dtype=torch.float32))
    check_backward(dx, dwq, dwk, dy, qkv, wq, wk, cos, sin, h, hkv, p)


def test_qk_norm_off_leaves_the_parameters_as_they_were():
    from kgs.models.attn_block import AttentionBlock
    from kgs.models.decoder import DecoderLM

    layer_keys = ["attn_norm", "mlp_norm", "qkv.weight", "o.weight", "gate_up.weight", "down.weight"]
    lm = {on: DecoderLM(64, 256, 1, 2, 1, 64, backend="torch", qk_norm=on) for on in (False, True)}
    base = ["norm", "embed.weight", "head.weight"]
    assert sorted(lm[False].state_dict()) == sorted(base + [f"layers.0.{k}" for k in layer_keys])
    assert sorted(lm[True].state_dict()) == sorted(base + [f"layers.0.{k}" for k in layer_keys + ["q_norm", "k_norm"]])
    assert sorted(AttentionBlock(256, 2, 1, backend="torch").state_dict()) == ["o.weight", "qkv.weight"]
    blk = AttentionBlock(256, 2, 1, backend="torch", qk_norm=True)
    assert sorted(blk.state_dict()) == ["k_norm", "o.weight", "q_norm", "qkv.weight"]
    x = torch.randn(1, 8, 256).bfloat16()
    assert lm[True].layers[0].q_norm.shape == (128,) and blk(x).shape == x.shape
    assert torch.isfinite(lm[True](torch.randint(0, 64, (1, 8))).float()).all()
