"""A trainable token embedding on the kernels of ``native/kernels/embedding.hip``:
a row gather forward and a deterministic, dense scatter-sum backward.

With ``w [vocab, cols]`` bf16, ``tok [rows]`` int64 and ``dy [rows, cols]`` bf16::

    out[t, :] = bf16(scale * w[tok[t], :])                     (embedding_rows)
    dw[v, :]  = bf16(scale * sum_{t: tok[t] == v} dy[t, :])    (embedding_rows_backward)

A token outside ``[0, vocab)`` gives a row of zeros forward and contributes
nothing backward (the convention :func:`kgs.ops.cross_entropy_rows` has for an
ignored target); all 64 bits of a token are compared. The backward sums in fp32
in ascending position and rounds once; it writes every element of ``dw``, rows
without a token as zeros, whatever ``dw`` held: no memset, no float atomics,
bitwise repeatable. The order of the tokens it walks is a stable
``torch.sort`` on the device: nothing synchronises with the host.

:func:`ref_embedding_rows` and :func:`ref_embedding_rows_backward` state the two
formulas in torch ops on any device (float64 by default): the model for the
tests.
"""
from __future__ import annotations

import sys
import types

import torch

from . import _lib


class _CallableModule(types.ModuleType):
    """``kgs.ops.embedding`` names both this module and the op :func:`embedding`
    (as ``torch.nn.functional.embedding`` does not have to: it has no module of
    its own). Python binds the submodule to that attribute of the package, so the
    module itself is callable as the op: ``kgs.ops.embedding(w, tok)``."""

    def __call__(self, *args, **kwargs):
        return embedding(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule


# ---------------------------------------------------------------------------
# argument checks: dtype and shape before the device, so a wrong call fails the
# same way everywhere, and all of them before the native library is touched
def _check_matrix(t, name: str, shape: tuple | None = None) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be a bf16 tensor")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be a row-major 2-D matrix")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    rows, cols = t.shape
    if cols == 0 or cols % 8:
        raise ValueError(f"{name}: cols must be a positive multiple of 8, got {cols}")
    if rows > 1 and (t.stride(0) < cols or t.stride(0) % 8):
        raise ValueError(f"{name}: the row stride must be a multiple of 8 elements, at least cols")


def _check_tokens(tok) -> torch.Tensor:
    if not isinstance(tok, torch.Tensor) or tok.dtype != torch.int64:
        raise TypeError("tok must be an int64 tensor")
    return tok.reshape(-1).contiguous()


def _check_scale(scale) -> float:
    if isinstance(scale, torch.Tensor) or not isinstance(scale, (int, float)):
        raise TypeError("scale must be a number")
    return float(scale)


def _check_padding(padding_idx, vocab: int) -> int:
    if padding_idx is None:
        return -1
    if isinstance(padding_idx, bool) or not isinstance(padding_idx, int):
        raise TypeError("padding_idx must be an int or None")
    if not 0 <= padding_idx < vocab:
        raise ValueError(f"padding_idx must be in [0, {vocab}), got {padding_idx}")
    return padding_idx


def _check_place(*named) -> None:
    dev = None
    for t, name in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{name} must be on a GPU")
        if dev is not None and t.device != dev:
            raise ValueError(f"{name} must be on the device of the other operands")
        dev = t.device
        if t.dtype == torch.bfloat16 and t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")


def _ld(t: torch.Tensor) -> int:
    # a view of at most one row may carry any row stride: the kernels never use it
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


# ---------------------------------------------------------------------------
# raw ops
def embedding_rows(w: torch.Tensor, tok: torch.Tensor, scale: float = 1.0,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[t, :] = bf16(scale * w[tok[t], :])``: bf16 ``[tok.numel(), cols]`` from
    the bf16 table ``w [vocab, cols]`` (``cols % 8 == 0``, any row stride that is a
    multiple of 8) and int64 tokens of any shape, which are flattened. With
    ``scale == 1`` a row is a bit copy. A token outside ``[0, vocab)`` gives a row
    of zeros. ``out``: a bf16 ``[rows, cols]`` view (any row stride); only its
    columns ``< cols`` are written."""
    _check_matrix(w, "w")
    vocab, cols = w.shape
    if vocab == 0:
        raise ValueError("w must have at least one row")
    tok = _check_tokens(tok)
    rows = tok.numel()
    scale = _check_scale(scale)
    if out is not None:
        _check_matrix(out, "out", (rows, cols))
    _check_place((w, "w"), (tok, "tok"), (out, "out"))
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.bfloat16, device=w.device)
    rc = _lib.lib().kgs_embed_fwd_bf16(w.data_ptr(), tok.data_ptr(), out.data_ptr(), rows, vocab, cols, _ld(w),
                                       _ld(out), scale, _lib.stream_handle(w.device))
    _lib.check(rc, f"embedding_rows[{rows}x{cols}]")
    return out


def embedding_rows_backward(dy: torch.Tensor, tok: torch.Tensor, vocab: int, scale: float = 1.0,
                            padding_idx: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """``dw[v, :] = bf16(scale * sum_{t: tok[t] == v} dy[t, :])``: the dense bf16
    ``[vocab, cols]`` gradient of :func:`embedding_rows`' table from ``dy [rows,
    cols]`` bf16 and the int64 tokens (any shape, flattened to ``rows``). The sum
    is taken in fp32 in ascending ``t`` and rounded once. Every element of ``dw``
    is written: a row with no token, and row ``padding_idx`` whatever its tokens,
    is zeros. Tokens outside ``[0, vocab)`` contribute nothing. ``out``: a bf16
    ``[vocab, cols]`` view (any row stride) that need not be zeroed. One stable
    device sort of the tokens and one kernel; no atomics, bitwise repeatable."""
    _check_matrix(dy, "dy")
    rows, cols = dy.shape
    tok = _check_tokens(tok)
    if tok.numel() != rows:
        raise ValueError(f"tok must have dy's {rows} rows, got {tok.numel()}")
    if isinstance(vocab, bool) or not isinstance(vocab, int):
        raise TypeError("vocab must be an int")
    if not 0 < vocab < 2 ** 31:
        raise ValueError("vocab must be positive and below 2^31")
    scale = _check_scale(scale)
    pad = _check_padding(padding_idx, vocab)
    if out is not None:
        _check_matrix(out, "out", (vocab, cols))
    _check_place((dy, "dy"), (tok, "tok"), (out, "out"))
    if out is None:
        out = torch.empty((vocab, cols), dtype=torch.bfloat16, device=dy.device)
    srt, order = torch.sort(tok, stable=True)
    rc = _lib.lib().kgs_embed_bwd_bf16(dy.data_ptr(), srt.data_ptr(), order.data_ptr(), out.data_ptr(), rows, vocab,
                                       cols, _ld(dy), _ld(out), scale, pad, _lib.stream_handle(dy.device))
    _lib.check(rc, f"embedding_rows_backward[{rows}x{cols} -> {vocab}]")
    return out


# ---------------------------------------------------------------------------
# the autograd op and the module
def _grad_rows(g: torch.Tensor) -> torch.Tensor:
    """An incoming ``[rows, cols]`` gradient as the kernel takes it: unit column
    stride, a row stride that is a multiple of 8, 16-byte aligned."""
    cols = g.shape[1]
    ok = g.stride(1) == 1 and (g.shape[0] <= 1 or (g.stride(0) >= cols and g.stride(0) % 8 == 0)) and \
        g.data_ptr() % 16 == 0
    return g if ok else g.contiguous()


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, tok, scale, padding_idx):
        ctx.save_for_backward(tok)
        ctx.vocab, ctx.scale, ctx.padding_idx = w.shape[0], scale, padding_idx
        return embedding_rows(w, tok, scale)  # a tensor of its own: the caller reshapes it outside

    @staticmethod
    def backward(ctx, dy):
        (tok,) = ctx.saved_tensors
        dw = embedding_rows_backward(_grad_rows(dy), tok, ctx.vocab, ctx.scale, ctx.padding_idx)
        return dw, None, None, None


def embedding(w: torch.Tensor, tok: torch.Tensor, scale: float = 1.0, padding_idx: int | None = None) -> torch.Tensor:
    """Differentiable ``scale * w[tok]``: bf16 ``[*tok.shape, cols]``. Forward is
    :func:`embedding_rows`; when ``w`` wants no gradient that is all (nothing is
    saved). Otherwise only ``tok`` is saved and the backward returns the dense
    ``dw`` of :func:`embedding_rows_backward`. ``padding_idx`` has torch's meaning:
    the stored row is returned as it is, and its gradient is zero."""
    _check_matrix(w, "w")
    tok_flat = _check_tokens(tok)
    scale = _check_scale(scale)
    _check_padding(padding_idx, w.shape[0])
    if not (torch.is_grad_enabled() and w.requires_grad):
        return embedding_rows(w, tok_flat, scale).reshape(*tok.shape, w.shape[1])
    return _EmbeddingFn.apply(w, tok, scale, padding_idx).reshape(*tok.shape, w.shape[1])


class Embedding(torch.nn.Module):
    """``nn.Embedding`` with a bf16 weight (so :class:`kgs.optim.AdamW` drives it
    unchanged) on :func:`embedding`: ``forward(tokens)`` returns ``[*tokens.shape,
    dim]`` = ``scale * weight[tokens]``. ``dim % 8 == 0``. The initial weight is
    N(0, 1) with row ``padding_idx`` zeroed, as torch's."""

    def __init__(self, vocab: int, dim: int, padding_idx: int | None = None, scale: float = 1.0, device=None):
        super().__init__()
        if vocab <= 0 or dim <= 0 or dim % 8:
            raise ValueError(f"Embedding takes a positive vocab and a dim that is a positive multiple of 8, got "
                             f"{vocab}, {dim}")
        _check_padding(padding_idx, vocab)
        self.vocab, self.dim, self.padding_idx, self.scale = vocab, dim, padding_idx, _check_scale(scale)
        w = torch.empty(vocab, dim, dtype=torch.bfloat16, device=device)
        torch.nn.init.normal_(w)
        if padding_idx is not None:
            w[padding_idx].zero_()
        self.weight = torch.nn.Parameter(w)

    def forward(self, tokens: torch.Tensor) -> torch.Tensor:
        return embedding(self.weight, tokens, self.scale, self.padding_idx)

    def extra_repr(self) -> str:
        return f"{self.vocab}, {self.dim}, padding_idx={self.padding_idx}, scale={self.scale}"


# ---------------------------------------------------------------------------
# the model: the same formulas in torch ops
def _in_range(tok: torch.Tensor, vocab: int) -> torch.Tensor:
    return (tok >= 0) & (tok < vocab)


def ref_embedding_rows(w: torch.Tensor, tok: torch.Tensor, scale: float = 1.0, dtype=torch.float64) -> torch.Tensor:
    """:func:`embedding_rows` evaluated in ``dtype`` (not rounded): ``[rows, cols]``."""
    tok = tok.reshape(-1)
    ok = _in_range(tok, w.shape[0])
    out = torch.zeros((tok.numel(), w.shape[1]), dtype=dtype, device=w.device)
    out[ok] = w.to(dtype)[tok[ok]] * scale
    return out


def ref_embedding_rows_backward(dy: torch.Tensor, tok: torch.Tensor, vocab: int, scale: float = 1.0,
                                padding_idx: int | None = None, dtype=torch.float64) -> torch.Tensor:
    """:func:`embedding_rows_backward` evaluated in ``dtype`` (not rounded): ``[vocab, cols]``."""
    tok = tok.reshape(-1)
    ok = _in_range(tok, vocab)
    if padding_idx is not None:
        ok = ok & (tok != padding_idx)
    dw = torch.zeros((vocab, dy.shape[-1]), dtype=dtype, device=dy.device)
    dw.index_add_(0, tok[ok], dy.reshape(-1, dy.shape[-1]).to(dtype)[ok])
    return dw * scale
