"""A self-attention block whose whole forward and backward run on the HIP
kernels: the first model-level user of :func:`kgs.ops.flash_attention_qkv`.

``QKV Linear -> rotate-half RoPE -> flash attention (causal, GQA) -> o Linear``.
With ``backend="kgs"`` both projections are :class:`kgs.ops.Linear` (forward,
dX and dW on the HIP GEMM) and the attention is the flash-attention forward with
log-sum-exp plus the dQ / dK / dV kernels (``native/kernels/attention_train.hip``);
the attention's fused ``dqkv`` gradient feeds the QKV projection's backward with
no ``cat``. RoPE is plain torch (autograd): memory bound, and out of scope for a
kernel here. ``backend="torch"`` is the same module on ``nn.Linear`` +
``scaled_dot_product_attention`` (CPU tests, the fp32 reference copy, and the
PyTorch-ROCm comparison on a GPU). The reference has no model code; nothing here
is ported.
"""
from __future__ import annotations

import torch


def _rope(qkv: torch.Tensor, batch: int, seq: int, rot_heads: int, head_dim: int, theta: float) -> torch.Tensor:
    """Rotate-half RoPE on the first ``rot_heads`` heads (q then k) of every
    token row, in fp32, rounded back to ``qkv``'s dtype."""
    from kgs.ops.transformer import rope_tables

    t = batch * seq
    cos, sin = rope_tables(seq, head_dim, theta, qkv.device)
    x = qkv[:, :rot_heads * head_dim].float().reshape(batch, seq, rot_heads, head_dim)
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    x1, x2 = x[..., :head_dim // 2], x[..., head_dim // 2:]
    rot = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).reshape(t, rot_heads * head_dim)
    return torch.cat((rot.to(qkv.dtype), qkv[:, rot_heads * head_dim:]), dim=1)


class AttentionBlock(torch.nn.Module):
    def __init__(self, dim: int, heads: int, kv_heads: int, backend: str = "kgs", causal: bool = True,
                 rope_theta: float = 10000.0, device=None, dtype=torch.bfloat16, seed: int = 0):
        super().__init__()
        if backend not in ("kgs", "torch"):
            raise ValueError(f"backend must be 'kgs' or 'torch', not {backend!r}")
        if dim % heads or heads % kv_heads:
            raise ValueError("dim must divide by heads and heads by kv_heads")
        self.backend, self.dim, self.heads, self.kv_heads = backend, dim, heads, kv_heads
        self.head_dim, self.causal, self.rope_theta = dim // heads, causal, rope_theta
        if backend == "kgs" and (self.head_dim != 128 or dtype != torch.bfloat16):
            raise ValueError("the kgs backend takes head_dim 128 and bf16")
        wqkv = (heads + 2 * kv_heads) * self.head_dim
        if backend == "kgs":
            from kgs.ops.gemm import Linear

            self.qkv = Linear(dim, wqkv, bias=False, device=device)
            self.o = Linear(dim, dim, bias=False, device=device)
        else:
            self.qkv = torch.nn.Linear(dim, wqkv, bias=False, device=device, dtype=dtype)
            self.o = torch.nn.Linear(dim, dim, bias=False, device=device, dtype=dtype)
        g = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():  # identical init for both backends
            self.qkv.weight.copy_(torch.randn(wqkv, dim, generator=g) * dim ** -0.5)
            self.o.weight.copy_(torch.randn(dim, dim, generator=g) * dim ** -0.5)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """``x``: ``[batch, seq, dim]`` -> ``[batch, seq, dim]``."""
        b, s, _ = x.shape
        nh, nkv, hd = self.heads, self.kv_heads, self.head_dim
        qkv = self.qkv(x.reshape(b * s, self.dim))
        qkv = _rope(qkv, b, s, nh + nkv, hd, self.rope_theta)
        if self.backend == "kgs":
            from kgs.ops.transformer import flash_attention_qkv

            a = flash_attention_qkv(qkv, b, s, nh, nkv, causal=self.causal)
        else:
            q = qkv[:, :nh * hd].reshape(b, s, nh, hd).transpose(1, 2)
            k = qkv[:, nh * hd:(nh + nkv) * hd].reshape(b, s, nkv, hd).transpose(1, 2)
            v = qkv[:, (nh + nkv) * hd:].reshape(b, s, nkv, hd).transpose(1, 2)
            k, v = (t.repeat_interleave(nh // nkv, dim=1) for t in (k, v))
            a = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
            a = a.transpose(1, 2).reshape(b * s, nh * hd)
        return self.o(a).reshape(b, s, self.dim)
