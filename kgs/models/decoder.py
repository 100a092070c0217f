"""A trainable pre-norm Llama decoder layer and a small language model over it:
with ``backend="kgs"`` and ``embedding="kgs"`` a whole training step, from the
token gather to the loss and back, runs on the HIP kernels.

``DecoderLayer``: ``rmsnorm -> QKV Linear -> RoPE -> flash attention -> o Linear``,
then ``rmsnorm -> gate|up Linear -> SwiGLU -> down Linear``. The residual stream
travels as a pair ``(x, delta)`` whose value is ``x + delta``: each norm is
:func:`kgs.ops.rmsnorm_residual`, which adds the pending delta, writes the new
stream value and normalises it in one kernel, and whose backward folds the
residual branch's gradient into the norm's ``dx`` in one kernel too. The layer's
attention output is added by its own second norm; its MLP output is returned as
``delta`` for the next layer's first norm (or the model's final norm).

``backend="kgs"``: :class:`kgs.ops.Linear` (forward, dX, dW on the HIP GEMM),
:func:`kgs.ops.flash_attention_qkv`, and the glue ops of
``native/kernels/train_ops.hip`` -- :func:`kgs.ops.rmsnorm_residual`,
:func:`kgs.ops.rope_qkv`, :func:`kgs.ops.swiglu`, :func:`kgs.ops.softmax_cross_entropy`.
``glue="torch"`` keeps the kgs GEMMs and attention but runs that glue as plain
torch autograd ops: the layer as it could be built before those kernels, kept for
the benchmark's comparison. ``backend="torch"`` is the same module on
``nn.Linear``, ``scaled_dot_product_attention`` and torch glue (CPU tests, the
fp32 reference copy, the PyTorch-ROCm comparison). Both backends start from the
same seeded weights. ``linear="fp8"`` swaps the four projections (qkv, o, gate|up,
down) for :class:`kgs.ops.LinearFp8` -- forward, dX and dW in e4m3 -- or, with
``backend="torch"``, for its torch model :class:`kgs.ops.RefLinearFp8`; the LM
head and the embedding stay as they are. ``embedding="kgs"`` (with the kgs backend)
swaps ``DecoderLM``'s ``nn.Embedding`` for :class:`kgs.ops.Embedding`: the gather
and the deterministic dense scatter-sum of ``native/kernels/embedding.hip``; the
default stays ``"torch"``. ``tie_embeddings=True`` makes the LM head's weight and
the embedding's one Parameter, as the small Llama-3.2 models have it. The
reference has no model code; nothing here is ported.
"""
from __future__ import annotations

import torch

from .attn_block import _rope


def _torch_rmsnorm(res: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    up = torch.promote_types(res.dtype, torch.float32)
    xf = res.to(up)
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.to(up)).to(res.dtype)


def _torch_swiglu(gu: torch.Tensor) -> torch.Tensor:
    up = torch.promote_types(gu.dtype, torch.float32)
    g, u = gu.to(up).chunk(2, dim=-1)
    return (torch.nn.functional.silu(g) * u).to(gu.dtype)


class DecoderLayer(torch.nn.Module):
    def __init__(self, dim: int, heads: int, kv_heads: int, inter: int, backend: str = "kgs", glue: str | None = None,
                 causal: bool = True, rope_theta: float = 10000.0, eps: float = 1e-5, device=None,
                 dtype=torch.bfloat16, seed: int = 0, linear: str = "bf16"):
        super().__init__()
        if backend not in ("kgs", "torch"):
            raise ValueError(f"backend must be 'kgs' or 'torch', not {backend!r}")
        if linear not in ("bf16", "fp8"):
            raise ValueError(f"linear must be 'bf16' or 'fp8', not {linear!r}")
        glue = backend if glue is None else glue
        if glue not in ("kgs", "torch") or (backend == "torch" and glue == "kgs"):
            raise ValueError("glue must be 'kgs' (with the kgs backend only) or 'torch'")
        if dim % heads or heads % kv_heads:
            raise ValueError("dim must divide by heads and heads by kv_heads")
        self.backend, self.glue, self.dim, self.inter, self.linear = backend, glue, dim, inter, linear
        self.heads, self.kv_heads = heads, kv_heads
        self.head_dim, self.causal, self.rope_theta, self.eps = dim // heads, causal, rope_theta, eps
        if backend == "kgs" and (self.head_dim != 128 or dtype != torch.bfloat16):
            raise ValueError("the kgs backend takes head_dim 128 and bf16")
        if glue == "kgs" and (dim % 512 or dim > 8192 or inter % 8):
            raise ValueError("the kgs glue takes dim a multiple of 512 up to 8192 and inter a multiple of 8")
        wqkv = (heads + 2 * kv_heads) * self.head_dim
        if linear == "fp8" and backend == "kgs":
            from kgs.ops.fp8_train import LinearFp8

            def lin(i, o):
                return LinearFp8(i, o, bias=False, device=device)
        elif linear == "fp8":
            from kgs.ops.fp8_train import RefLinearFp8

            def lin(i, o):
                return RefLinearFp8(i, o, bias=False, device=device, dtype=dtype)
        elif backend == "kgs":
            from kgs.ops.gemm import Linear

            def lin(i, o):
                return Linear(i, o, bias=False, device=device)
        else:
            def lin(i, o):
                return torch.nn.Linear(i, o, bias=False, device=device, dtype=dtype)
        self.attn_norm = torch.nn.Parameter(torch.ones(dim, device=device, dtype=dtype))
        self.qkv, self.o = lin(dim, wqkv), lin(dim, dim)
        self.mlp_norm = torch.nn.Parameter(torch.ones(dim, device=device, dtype=dtype))
        self.gate_up, self.down = lin(dim, 2 * inter), lin(inter, dim)
        g = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():  # identical init for both backends
            for m in (self.qkv, self.o, self.gate_up, self.down):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * m.weight.shape[1] ** -0.5)
        self._tables = {}

    def _rope_tables(self, seq: int, device):
        key = (seq, str(device))
        if key not in self._tables:
            from kgs.ops.transformer import rope_tables

            self._tables[key] = rope_tables(seq, self.head_dim, self.rope_theta, device)
        return self._tables[key]

    def forward(self, x: torch.Tensor, delta: torch.Tensor | None = None):
        """``x``, ``delta``: ``[batch, seq, dim]``, the stream value is ``x + delta``.
        Returns the pair for the next layer: the stream after this layer's
        attention, and this layer's MLP output still to be added to it."""
        b, s, _ = x.shape
        t, nh, nkv, hd = b * s, self.heads, self.kv_heads, self.head_dim
        x2 = x.reshape(t, self.dim)
        d2 = None if delta is None else delta.reshape(t, self.dim)
        if self.glue == "kgs":
            from kgs.ops.transformer import flash_attention_qkv, rmsnorm_residual, rope_qkv, swiglu

            res, h = rmsnorm_residual(x2, d2, self.attn_norm, self.eps)
            cos, sin = self._rope_tables(s, x.device)
            qkv = rope_qkv(self.qkv(h), cos, sin, nh + nkv, hd, s)
            att = self.o(flash_attention_qkv(qkv, b, s, nh, nkv, causal=self.causal))
            res, h = rmsnorm_residual(res, att, self.mlp_norm, self.eps)
            out = self.down(swiglu(self.gate_up(h)))
            return res.reshape(b, s, self.dim), out.reshape(b, s, self.dim)
        res = x2 if d2 is None else x2 + d2
        qkv = _rope(self.qkv(_torch_rmsnorm(res, self.attn_norm, self.eps)), b, s, nh + nkv, hd, self.rope_theta)
        if self.backend == "kgs":
            from kgs.ops.transformer import flash_attention_qkv

            a = flash_attention_qkv(qkv, b, s, nh, nkv, causal=self.causal)
        else:
            q = qkv[:, :nh * hd].reshape(b, s, nh, hd).transpose(1, 2)
            k = qkv[:, nh * hd:(nh + nkv) * hd].reshape(b, s, nkv, hd).transpose(1, 2)
            v = qkv[:, (nh + nkv) * hd:].reshape(b, s, nkv, hd).transpose(1, 2)
            k, v = (z.repeat_interleave(nh // nkv, dim=1) for z in (k, v))
            a = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
            a = a.transpose(1, 2).reshape(t, nh * hd)
        res = res + self.o(a)
        out = self.down(_torch_swiglu(self.gate_up(_torch_rmsnorm(res, self.mlp_norm, self.eps))))
        return res.reshape(b, s, self.dim), out.reshape(b, s, self.dim)


class DecoderLM(torch.nn.Module):
    """Token embedding, ``layers`` :class:`DecoderLayer`, a final norm and an LM
    head; :meth:`loss` is the mean cross-entropy over the targets that are not
    ignored (outside ``[0, vocab)``, e.g. -100).

    ``embedding``: ``"torch"`` (``nn.Embedding``, the default) or ``"kgs"``
    (:class:`kgs.ops.Embedding`; needs ``backend="kgs"`` and ``dim % 8 == 0``). The
    parameter is ``embed.weight`` with the same seeded init either way.
    ``tie_embeddings``: ``head.weight`` IS ``embed.weight``, one Parameter that
    ``parameters()`` yields once (under ``embed.weight``); it takes the head's
    init, ``randn * dim ** -0.5``, and its gradient is the sum of the two uses'."""

    def __init__(self, vocab: int, dim: int, layers: int, heads: int, kv_heads: int, inter: int, backend: str = "kgs",
                 glue: str | None = None, rope_theta: float = 10000.0, eps: float = 1e-5, device=None,
                 dtype=torch.bfloat16, seed: int = 0, linear: str = "bf16", embedding: str = "torch",
                 tie_embeddings: bool = False):
        super().__init__()
        if linear not in ("bf16", "fp8"):
            raise ValueError(f"linear must be 'bf16' or 'fp8', not {linear!r}")
        if embedding not in ("torch", "kgs"):
            raise ValueError(f"embedding must be 'torch' or 'kgs', not {embedding!r}")
        if embedding == "kgs" and (backend != "kgs" or dim % 8):
            raise ValueError("the kgs embedding takes the kgs backend and dim a multiple of 8")
        self.vocab, self.dim, self.eps, self.linear = vocab, dim, eps, linear
        self.embedding, self.tie_embeddings = embedding, bool(tie_embeddings)
        self.layers = torch.nn.ModuleList(
            DecoderLayer(dim, heads, kv_heads, inter, backend=backend, glue=glue, rope_theta=rope_theta, eps=eps,
                         device=device, dtype=dtype, seed=seed + 1 + i, linear=linear) for i in range(layers))
        self.backend, self.glue = backend, self.layers[0].glue if layers else (backend if glue is None else glue)
        if self.glue == "kgs" and vocab % 8:
            raise ValueError("the kgs loss takes a vocabulary that is a multiple of 8")
        if embedding == "kgs":
            from kgs.ops.embedding import Embedding

            self.embed = Embedding(vocab, dim, device=device)
        else:
            self.embed = torch.nn.Embedding(vocab, dim, device=device, dtype=dtype)
        self.norm = torch.nn.Parameter(torch.ones(dim, device=device, dtype=dtype))
        if backend == "kgs":
            from kgs.ops.gemm import Linear

            self.head = Linear(dim, vocab, bias=False, device=device)
        else:
            self.head = torch.nn.Linear(dim, vocab, bias=False, device=device, dtype=dtype)
        g = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():  # identical init for both backends
            self.embed.weight.copy_(torch.randn(vocab, dim, generator=g))
            self.head.weight.copy_(torch.randn(vocab, dim, generator=g) * dim ** -0.5)
            if tie_embeddings:  # the head's init, and the head's values of the untied model
                self.embed.weight.copy_(self.head.weight)
        if tie_embeddings:
            self.head.weight = self.embed.weight

    def forward(self, tokens: torch.Tensor) -> torch.Tensor:
        """``tokens``: int64 ``[batch, seq]`` -> logits ``[batch * seq, vocab]``."""
        b, s = tokens.shape
        x, delta = self.embed(tokens), None
        for layer in self.layers:
            x, delta = layer(x, delta)
        x2 = x.reshape(b * s, self.dim)
        d2 = None if delta is None else delta.reshape(b * s, self.dim)
        if self.glue == "kgs":
            from kgs.ops.transformer import rmsnorm_residual

            h = rmsnorm_residual(x2, d2, self.norm, self.eps)[1]
        else:
            h = _torch_rmsnorm(x2 if d2 is None else x2 + d2, self.norm, self.eps)
        return self.head(h)

    def loss(self, tokens: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """Mean cross-entropy (fp32 scalar) of ``targets`` ``[batch, seq]``."""
        logits, tg = self(tokens), targets.reshape(-1)
        live = (tg >= 0) & (tg < self.vocab)
        if self.glue == "kgs":
            from kgs.ops.transformer import softmax_cross_entropy

            rows = softmax_cross_entropy(logits, tg.contiguous())
        else:
            up = torch.promote_types(logits.dtype, torch.float32)
            rows = torch.nn.functional.cross_entropy(logits.to(up), torch.where(live, tg, torch.full_like(tg, -100)),
                                                     reduction="none", ignore_index=-100)
        return rows.sum() / live.sum().clamp(min=1)
