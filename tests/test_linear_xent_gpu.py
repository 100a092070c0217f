"""GPU tests of the fused LM head + loss (native/kernels/linear_xent.hip) against the float64
reference of kgs/ops/linear_xent.py, per element.

``tol_row = 2 K 2^-23 mag_row + 1e-4`` with ``mag_row = max_j (|h| |w|^T)[row, j]``: the project's loose
fp32 accumulation term (test_moe_gemm_gpu), once for the maximum logit and once for the target logit, plus
``LP_TOL = 1e-4``, the project's bound for an fp32 lse through v_exp / v_log (test_logit_ops_gpu).

* loss, lse: ``|err| <= tol_row``; an ignored row's loss is exactly 0 and its lse is still within it.
* dlogits: ``|err| <= 2^-8 |ref| + |grow| p_ref tol_row + 2^-126``: one bf16 rounding, the error of
  ``z - lse`` carried through ``e^x``, and the smallest normal number of bf16 and fp32, below which a
  product underflows in either format (the row that reaches +-80 has p_ref down to e^-160). On the
  p = 1 row lse equals the target logit in fp32, so the stored target entry is 0 whatever the formula: the
  bound holds it to within ``|grow| tol_row`` of ``grow (p - 1)``, and no sharper statement is true of it.
* the autograd op's dh and dW: at most twice the error of ``kgs.ops.linear`` + ``softmax_cross_entropy``
  against the same float64 autograd (the chunked fp32 sum of bf16 partial products in dh). There the
  +-80 row and the p = 1 row are scaled down, since today's path rounds its logits to bf16 and its error
  on them would make the comparison empty; so the chunked backward is not run on the extreme rows, which
  the dlogits test covers.
"""
import functools

import pytest
import torch

from forward_refs import POISON
from kgs.ops import linear_xent as lx

pytestmark = pytest.mark.gpu

DEV, S = "cuda", 8  # S: STRIP of native/kernels/linear_xent.hip, the vocabulary tiles a forward workgroup walks
# T: one tile; T % 256 == 128 with several tile rows; two 256-row tiles. V: one tile; a strip boundary; a
# ragged last strip. K: fewer K-steps than stages; an odd number of them.
CASES = [(t, v, k) for t in (128, 384, 512) for v in (128, 128 * (S + 1), 128 * (2 * S + 3)) for k in (64, 192)]
SCALED, PEAKY = 6, 7  # the row whose logits reach +-80, the row whose target has p = 1 in fp32


def _wide(rows, cols, src=None):  # a column block of a wider, taller poisoned buffer: (view, buffer)
    buf = torch.full((rows + 2, cols + 64), POISON, dtype=torch.bfloat16, device=DEV)
    view = buf[:rows, 8:8 + cols]
    if src is not None:
        view.copy_(src)
    return view, buf


@functools.lru_cache(maxsize=None)
def _case(t, v, k):
    g = torch.Generator(device=DEV).manual_seed(t + v + k)
    w = (torch.randn(v, k, device=DEV, generator=g) * k ** -0.5).bfloat16().double()
    h = torch.randn(t, k, device=DEV, generator=g).bfloat16().double()
    tg = torch.randint(0, v, (t,), device=DEV, generator=g)
    tg[:6] = torch.tensor([0, 127, 128, v - 1, -100, v], device=DEV)  # 128 == V: ignored too
    h[SCALED] *= 80 / (h[SCALED] @ w.T).abs().max()
    h[PEAKY] = w[tg[PEAKY]] * 60 / w[tg[PEAKY]].square().sum()
    (h, _), (w, _) = _wide(t, k, h), _wide(v, k, w)
    grow = torch.randn(t, device=DEV, generator=g) / t
    z = h.double() @ w.double().T
    rloss, rlse = lx.ref_linear_cross_entropy(h, w, tg)
    live = (tg >= 0) & (tg < v)
    onehot = torch.arange(v, device=DEV)[None, :] == tg[:, None]
    p = (z - rlse[:, None]).exp()
    tol = 2 * k * 2.0 ** -23 * (h.double().abs() @ w.double().abs().T).max(1).values + 1e-4
    loss, lse = lx.linear_cross_entropy_rows(h, w, tg)
    out, buf = _wide(t, v)
    assert lx.linear_cross_entropy_dlogits(h, w, tg, lse, grow, out=out) is out
    return dict(h=h, w=w, tg=tg, grow=grow, live=live, z=z, rloss=rloss, rlse=rlse, p=p, tol=tol, loss=loss, lse=lse,
                rdl=grow.double()[:, None] * (p - onehot.double()) * live[:, None], dl=out, buf=buf)


@pytest.mark.parametrize("t,v,k", CASES)
def test_loss_and_lse_against_float64(t, v, k):
    c = _case(t, v, k)
    assert c["z"][SCALED].abs().max() > 79
    e_loss, e_lse = (c["loss"].double() - c["rloss"]).abs(), (c["lse"].double() - c["rlse"]).abs()
    print(f"loss err {e_loss.max().item():.3e}, lse err {e_lse.max().item():.3e}, least tol {c['tol'].min().item():.3e}")
    assert torch.isfinite(c["lse"]).all() and (e_loss <= c["tol"]).all() and (e_lse <= c["tol"]).all()
    assert (c["loss"][~c["live"]] == 0).all() and int((~c["live"]).sum()) >= 2
    for tile in (0, 1)[:1 + (t % 256 == 0)]:  # either tile shape: the same additions in the same order
        assert all(torch.equal(a, b) for a, b in zip(lx.linear_cross_entropy_rows(c["h"], c["w"], c["tg"], tile=tile),
                                                     (c["loss"], c["lse"])))


@pytest.mark.parametrize("t,v,k", CASES)
def test_dlogits_against_float64(t, v, k):
    c = _case(t, v, k)
    dl, ref, g = c["dl"], c["rdl"], c["grow"].double().abs()[:, None]
    bound = 2.0 ** -8 * ref.abs() + g * c["p"] * c["tol"][:, None] + 2.0 ** -126
    err = (dl.double() - ref).abs()
    print(f"dlogits: max err {err.max().item():.3e}, least margin {(bound - err).min().item():.3e}")
    assert (err <= bound).all()
    tp = c["tg"][PEAKY]
    assert c["p"][PEAKY, tp].float() == 1 and dl[PEAKY].float().sum().abs() <= bound[PEAKY, tp]
    assert (dl[~c["live"]] == 0).all()
    if v > 128:  # a column range: the same bits as those columns of the full range
        part = lx.linear_cross_entropy_dlogits(c["h"], c["w"], c["tg"], c["lse"], c["grow"], cols=(128, v))
        assert torch.equal(part, dl[:, 128:])
    rest = c["buf"].clone()
    rest[:t, 8:8 + v] = POISON
    assert (rest == POISON).all()  # the surroundings of the output kept their poison


def test_autograd_op_against_todays_path():
    from kgs.ops.gemm import linear
    from kgs.ops.transformer import softmax_cross_entropy

    t, v, k = 384, 128 * (S + 1), 192
    c = _case(t, v, k)
    h0, w0, tg = c["h"].contiguous(), c["w"].contiguous(), c["tg"]
    h0[SCALED] /= 16  # today's path rounds its logits to bf16: keep them where that is harmless
    h0[PEAKY] /= 4

    def grads(loss_rows, dtype=torch.bfloat16):
        h, w = h0.to(dtype, copy=True).requires_grad_(True), w0.to(dtype, copy=True).requires_grad_(True)
        loss_rows(h, w).sum().backward()
        return h.grad.double(), w.grad.double()

    ref = grads(lambda h, w: lx.ref_linear_cross_entropy(h, w, tg)[0], torch.float64)
    base = grads(lambda h, w: softmax_cross_entropy(linear(h, w), tg))
    for chunk in (128, v):
        got = grads(lambda h, w: lx.linear_cross_entropy(h, w, tg, chunk=chunk))
        for name, a, b, r in zip(("dh", "dW"), got, base, ref):
            e_new, e_old = (a - r).abs().max().item(), (b - r).abs().max().item()
            print(f"chunk {chunk} {name}: fused {e_new:.3e}, today's path {e_old:.3e}")
            assert e_new <= 2 * e_old, (chunk, name, e_new, e_old)
    with torch.no_grad():  # no gradient wanted: the raw forward, nothing saved
        assert lx.linear_cross_entropy(h0, w0, tg).grad_fn is None


@pytest.mark.parametrize("tie", [False, True])
def test_decoder_lm_fused_loss(tie):
    """The issue's model has dim 128, which the kgs glue's norm does not take (dim % 512 == 0): dim 512
    in 4 heads of 128 is the smallest model of that shape."""
    from kgs.models.decoder import DecoderLM

    kw = dict(vocab=256, dim=512, layers=1, heads=4, kv_heads=1, inter=256, device=DEV, tie_embeddings=tie, seed=3)
    fused, plain = DecoderLM(**kw, fused_loss=True), DecoderLM(**kw)
    g = torch.Generator().manual_seed(5)
    tokens, targets = (torch.randint(0, 256, (1, 128), generator=g).to(DEV) for _ in range(2))
    targets[0, :3] = -100
    got, want = fused.loss(tokens, targets), plain.loss(tokens, targets)
    with torch.no_grad():
        h, w = fused._hidden(tokens).double(), fused.head.weight.double()
    tol = 2 * 512 * 2.0 ** -23 * (h.abs() @ w.abs().T).max().item() + 1e-4 + 2.0 ** -8 * (h @ w.T).abs().max().item()
    print(f"fused {got.item():.6f}, unfused {want.item():.6f}, tol {tol:.3e}")
    assert abs(got.item() - want.item()) <= tol
    got.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in fused.parameters())
    assert fused.embed.weight.grad is not None and (not tie or fused.head.weight is fused.embed.weight)
