"""CPU tests of the training glue (the kernels themselves:
tests/test_train_ops_gpu.py): the float64 references, which state the backward
formulas directly, against torch autograd; the torch backend of DecoderLayer /
DecoderLM; and the argument checks of the new ops, which raise before the native
library is touched."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.ops.transformer import (cross_entropy_rows, cross_entropy_rows_backward, ref_cross_entropy_rows,
                                 ref_cross_entropy_rows_backward, ref_rmsnorm_backward, ref_rope_qkv,
                                 ref_rope_qkv_backward, ref_silu_mul_backward, rmsnorm_backward, rmsnorm_residual,
                                 rope_qkv, rope_tables, silu_mul_backward, softmax_cross_entropy, swiglu)

F64 = torch.float64
TOL = 1e-10


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b):
    assert a.dtype == F64 and a.shape == b.shape
    assert (a - b).abs().max().item() <= TOL, (a - b).abs().max().item()


@pytest.mark.parametrize("with_dres", [False, True])
def test_ref_rmsnorm_backward_is_autograds_gradient(with_dres):
    g = _gen(1)
    rows, cols, eps = 7, 24, 1e-5
    x = torch.randn(rows, cols, generator=g, dtype=F64).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(cols, generator=g, dtype=F64)).requires_grad_(True)
    dy = torch.randn(rows, cols, generator=g, dtype=F64)
    dres = torch.randn(rows, cols, generator=g, dtype=F64) if with_dres else None
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    # the residual branch hands x's value on unchanged: its gradient adds to the norm's
    obj = (y * dy).sum() + ((x * dres).sum() if with_dres else 0)
    gx, gw = torch.autograd.grad(obj, (x, w))
    dx, dw = ref_rmsnorm_backward(x.detach(), w.detach(), dy, dres, eps)
    _close(dx, gx)
    _close(dw, gw)


def test_ref_silu_mul_backward_is_autograds_gradient():
    g = _gen(2)
    gu = (2 * torch.randn(9, 32, generator=g, dtype=F64)).requires_grad_(True)
    dh = torch.randn(9, 16, generator=g, dtype=F64)
    h = torch.nn.functional.silu(gu[:, :16]) * gu[:, 16:]
    (ggu,) = torch.autograd.grad(h, gu, dh)
    _close(ref_silu_mul_backward(gu.detach(), dh), ggu)


def test_ref_rope_qkv_backward_is_autograds_gradient():
    g = _gen(3)
    seq, batch, heads, hd, extra = 6, 2, 3, 16, 24
    cos, sin = (t.double() for t in rope_tables(seq, hd, 10000.0, "cpu"))
    qkv = torch.randn(batch * seq, heads * hd + extra, generator=g, dtype=F64).requires_grad_(True)
    dout = torch.randn(batch * seq, heads * hd + extra, generator=g, dtype=F64)
    (gq,) = torch.autograd.grad(_rope_autograd(qkv, cos, sin, heads, hd, seq), qkv, dout)
    got = ref_rope_qkv_backward(dout, cos, sin, heads, hd, seq)
    _close(got, gq)
    assert torch.equal(got[:, heads * hd:], dout[:, heads * hd:])  # pass-through columns
    # the rotation differentiated above is the forward reference's (which works in fp32)
    torch.testing.assert_close(_rope_autograd(qkv, cos, sin, heads, hd, seq).detach(),
                               ref_rope_qkv(qkv.detach(), cos, sin, heads, hd, seq), rtol=0, atol=1e-5)


def _rope_autograd(qkv, cos, sin, heads, hd, seq):
    t = qkv.shape[0]
    x = qkv[:, :heads * hd].reshape(t, heads, hd)
    pos = torch.arange(t) % seq
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
    rot = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).reshape(t, heads * hd)
    return torch.cat((rot, qkv[:, heads * hd:]), dim=1)


def test_ref_cross_entropy_is_torchs_and_its_backward_autograds():
    g = _gen(4)
    rows, cols = 6, 40
    x = (3 * torch.randn(rows, cols, generator=g, dtype=F64)).requires_grad_(True)
    tg = torch.tensor([0, cols - 1, 5, -100, 17, cols + 3])
    grow = torch.randn(rows, generator=g, dtype=F64)
    loss, lse = ref_cross_entropy_rows(x.detach(), tg)
    want = torch.nn.functional.cross_entropy(x, torch.where((tg >= 0) & (tg < cols), tg, -100), reduction="none",
                                             ignore_index=-100)
    _close(loss, want.detach())
    _close(lse, torch.logsumexp(x.detach(), 1))
    assert loss[3] == 0 and loss[5] == 0
    (gx,) = torch.autograd.grad(want, x, grow)
    got = ref_cross_entropy_rows_backward(x.detach(), tg, lse, grow)
    _close(got, gx)
    assert got[3].abs().max() == 0 and got[5].abs().max() == 0  # ignored rows


# ----------------------------------------------------------------------------
# models, torch backend

DIM, NH, NKV, INTER = 64, 4, 2, 96


def _layer(**kw):
    from kgs.models.decoder import DecoderLayer

    return DecoderLayer(DIM, NH, NKV, INTER, backend="torch", dtype=torch.float32, **kw)


def test_decoder_layer_shapes_and_gradients_on_cpu():
    layer = _layer()
    x = torch.randn(2, 8, DIM, generator=_gen(5)).requires_grad_(True)
    res, delta = layer(x)
    assert res.shape == x.shape and delta.shape == x.shape
    (res + delta)[:, 3].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.parameters())
    assert x.grad[:, :4].abs().sum() > 0 and x.grad[:, 4:].abs().sum() == 0  # causal: later tokens unseen


def test_decoder_layer_chaining_equals_the_unchained_sum():
    """layer(x, delta) is layer(x + delta): the pair is only a deferred add, so two
    chained layers equal the same layers applied to the summed stream."""
    a, b = _layer(seed=1), _layer(seed=2)
    x = torch.randn(2, 8, DIM, generator=_gen(6))
    d = torch.randn(2, 8, DIM, generator=_gen(7))
    r1, d1 = a(x, d)
    r0, d0 = a(x + d)
    torch.testing.assert_close(r1, r0, rtol=0, atol=0)
    torch.testing.assert_close(d1, d0, rtol=0, atol=0)
    r2, d2 = b(r1, d1)
    r3, d3 = b(r1 + d1)
    torch.testing.assert_close(r2 + d2, r3 + d3, rtol=1e-6, atol=1e-6)


def test_decoder_layer_rejects_what_the_kgs_backend_cannot_run():
    from kgs.models.decoder import DecoderLayer

    with pytest.raises(ValueError):
        DecoderLayer(64, 4, 2, 96, backend="kgs")  # head_dim 16
    with pytest.raises(ValueError):
        DecoderLayer(64, 4, 2, 96, backend="torch", glue="kgs")
    with pytest.raises(ValueError):
        DecoderLayer(64, 4, 2, 96, backend="jax")


def _lm(**kw):
    from kgs.models.decoder import DecoderLM

    return DecoderLM(48, DIM, 2, NH, NKV, INTER, backend="torch", dtype=torch.float32, **kw)


def test_decoder_lm_shapes_and_seeded_init():
    lm, twin = _lm(), _lm()
    tokens = torch.randint(0, 48, (2, 8), generator=_gen(8))
    logits = lm(tokens)
    assert logits.shape == (16, 48)
    assert all(torch.equal(p, q) for p, q in zip(lm.parameters(), twin.parameters()))
    assert not torch.equal(lm.layers[0].qkv.weight, lm.layers[1].qkv.weight)
    loss = lm.loss(tokens, tokens.roll(-1, 1))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    want = torch.nn.functional.cross_entropy(logits, tokens.roll(-1, 1).reshape(-1))
    torch.testing.assert_close(loss, want, rtol=1e-6, atol=1e-6)


def test_decoder_lm_ignored_targets_contribute_no_gradient():
    lm = _lm()
    tokens = torch.randint(0, 48, (2, 8), generator=_gen(9))
    targets = tokens.roll(-1, 1).clone()
    targets[:, 5:] = -100
    lm.loss(tokens, targets).backward()
    masked = {n: p.grad.clone() for n, p in lm.named_parameters()}
    # what the ignored positions hold must not matter: the same loss and gradients as any other filler
    lm.zero_grad()
    other = targets.clone()
    other[:, 5:] = 48 + 7  # out of range: ignored as well
    loss = lm.loss(tokens, other)
    loss.backward()
    for n, p in lm.named_parameters():
        torch.testing.assert_close(p.grad, masked[n], rtol=0, atol=0)
    # and the mean is over the 10 live rows only
    live = torch.nn.functional.cross_entropy(lm(tokens).reshape(2, 8, 48)[:, :5].reshape(10, 48),
                                             targets[:, :5].reshape(-1))
    torch.testing.assert_close(loss, live, rtol=1e-6, atol=1e-6)
    # causal + ignored: positions >= 5 are neither seen by a live row nor scored themselves
    e = lm.embed.weight.grad
    unseen = [t for t in set(tokens[:, 5:].reshape(-1).tolist()) if t not in set(tokens[:, :5].reshape(-1).tolist())]
    assert unseen and all(e[t].abs().max() == 0 for t in unseen)


# ----------------------------------------------------------------------------
# argument checks: raised before the native library is loaded (there is no GPU here)

def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


@pytest.fixture
def no_native(monkeypatch):
    from kgs.ops import _lib

    def boom():
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(_lib, "lib", boom)


def test_rmsnorm_ops_check_their_arguments(no_native):
    x, w = _bf(4, 512), _bf(512)
    for fn in (lambda *a: rmsnorm_backward(a[0], a[1], a[2]), lambda *a: rmsnorm_residual(a[0], a[2], a[1])):
        with pytest.raises(TypeError):
            fn(x.float(), w, x)
        with pytest.raises(TypeError):
            fn(x, w.float(), x)
        with pytest.raises(TypeError):
            fn(x, w, x.float())
        with pytest.raises(ValueError, match="512"):
            fn(_bf(4, 520), _bf(520), _bf(4, 520))
        with pytest.raises(ValueError, match="512"):
            fn(_bf(4, 8704), _bf(8704), _bf(4, 8704))
        with pytest.raises(ValueError):
            fn(x, _bf(256), x)
        with pytest.raises(ValueError):
            fn(x, w, _bf(3, 512))
        with pytest.raises(ValueError, match="row-major"):
            fn(_bf(512, 4).t(), w, x)
        with pytest.raises(ValueError, match="GPU"):
            fn(x, w, x)
    with pytest.raises(TypeError):
        rmsnorm_backward(x, w, x, dres=x.float())
    with pytest.raises(ValueError):
        rmsnorm_backward(x, w, x, dres=_bf(4, 1024))
    with pytest.raises(ValueError, match="GPU"):
        rmsnorm_residual(x.requires_grad_(True), None, w)


def test_swiglu_ops_check_their_arguments(no_native):
    gu, dh = _bf(4, 32), _bf(4, 16)
    with pytest.raises(TypeError):
        silu_mul_backward(gu.float(), dh)
    with pytest.raises(TypeError):
        silu_mul_backward(gu, dh.float())
    with pytest.raises(TypeError):
        silu_mul_backward(gu, dh, out=gu.float())
    with pytest.raises(ValueError):
        silu_mul_backward(_bf(4, 24), _bf(4, 12))  # I % 8
    with pytest.raises(ValueError):
        silu_mul_backward(gu, _bf(4, 32))
    with pytest.raises(ValueError):
        silu_mul_backward(gu, dh, out=_bf(4, 16))
    with pytest.raises(ValueError, match="GPU"):
        silu_mul_backward(gu, dh)
    with pytest.raises(TypeError):
        swiglu(gu.float())
    with pytest.raises(ValueError):
        swiglu(_bf(4, 24))
    with pytest.raises(ValueError, match="GPU"):
        swiglu(gu)
    with pytest.raises(ValueError, match="GPU"):
        swiglu(gu.requires_grad_(True))


def test_rope_qkv_checks_its_arguments(no_native):
    qkv = _bf(8, 3 * 16)
    cos, sin = rope_tables(4, 16, 10000.0, "cpu")
    with pytest.raises(TypeError):
        rope_qkv(qkv.float(), cos, sin, 2, 16, 4)
    with pytest.raises(TypeError):
        rope_qkv(qkv, cos.double(), sin, 2, 16, 4)
    with pytest.raises(ValueError):
        rope_qkv(qkv, cos, sin, 4, 16, 4)  # more rotated heads than columns
    with pytest.raises(ValueError):
        rope_qkv(qkv, cos, sin, 2, 16, 8)  # tables shorter than seq
    with pytest.raises(ValueError):
        rope_qkv(qkv, cos[:, :4].contiguous(), sin, 2, 16, 4)
    with pytest.raises(ValueError, match="GPU"):
        rope_qkv(qkv, cos, sin, 2, 16, 4)
    with pytest.raises(TypeError):
        rope_qkv(qkv, cos, sin, 2, 16, 4, torch.zeros(8, dtype=torch.int32))  # positions: not supported


def test_cross_entropy_ops_check_their_arguments(no_native):
    x, tg, v = _bf(4, 16), torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    for fn in (cross_entropy_rows, softmax_cross_entropy, lambda a, b: cross_entropy_rows_backward(a, b, v, v)):
        with pytest.raises(TypeError):
            fn(x.float(), tg)
        with pytest.raises(TypeError):
            fn(x, tg.int())
        with pytest.raises(ValueError):
            fn(_bf(4, 12), tg)  # cols % 8
        with pytest.raises(ValueError):
            fn(x, tg[:3])
        with pytest.raises(ValueError, match="GPU"):
            fn(x, tg)
    with pytest.raises(TypeError):
        cross_entropy_rows_backward(x, tg, v.double(), v)
    with pytest.raises(TypeError):
        cross_entropy_rows_backward(x, tg, v, v.bfloat16())
    with pytest.raises(ValueError):
        cross_entropy_rows_backward(x, tg, v[:2], v)
    with pytest.raises(TypeError):
        cross_entropy_rows_backward(x, tg, v, v, out=x.float())
    with pytest.raises(ValueError):
        cross_entropy_rows_backward(x, tg, v, v, out=_bf(4, 24))


def test_ops_are_exported_from_kgs_ops():
    import kgs.ops

    for name in ("rmsnorm_backward", "silu_mul_backward", "cross_entropy_rows", "cross_entropy_rows_backward",
                 "rmsnorm_residual", "swiglu", "rope_qkv", "softmax_cross_entropy"):
        assert callable(getattr(kgs.ops, name))


# ----------------------------------------------------------------------------
# compile-time resources (hipcc cross-compiles gfx950 without a GPU)

@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_train_ops_kernels_use_no_scratch(tmp_path):
    """Every instantiation, rmsnorm_bwd<16> (8192 columns) included: no spilled VGPR,
    no scratch. The row kernel keeps its dw row in LDS and its operands packed;
    a regression here is a silent slowdown of every training step."""
    root = Path(__file__).resolve().parents[1]
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", str(root / "native/kernels"),
                          str(root / "native/kernels/train_ops.hip"), "-o", str(tmp_path / "train_ops.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600,
                         cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    norm = [n for n in res if "rmsnorm_bwdILi" in n]
    assert len(norm) == 16 and len(res) == 20, sorted(res)
    assert all("ScratchSize" in r and "VGPRs Spill" in r and "VGPRs" in r for r in res.values()), res
    bad = {n: r for n, r in res.items() if r["ScratchSize"] or r["VGPRs Spill"]}
    assert not bad, bad
    assert res[[n for n in norm if "ILi8E" in n][0]]["VGPRs"] <= 256  # 4096 columns: two waves per SIMD
