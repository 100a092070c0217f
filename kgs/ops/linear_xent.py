"""The LM head fused with the softmax cross-entropy (``native/kernels/linear_xent.hip``):
the loss of ``z = h @ w.T`` without the logits ``[T, V]`` ever reaching memory.

* :func:`linear_cross_entropy_rows` -- the raw forward: the head GEMM tile by tile on the
  MFMA, each fp32 tile folded into an online softmax; ``(loss, lse)``, fp32 ``[T]``.
* :func:`linear_cross_entropy_dlogits` -- the raw backward piece: the tiles of a column range
  recomputed and stored as ``bf16(grow * (softmax - onehot))``.
* :func:`linear_cross_entropy` -- the autograd op: it keeps ``h``, ``w``, ``target`` and ``lse``
  and walks the vocabulary in chunks backward, one reused ``[T, chunk]`` dlogits buffer feeding
  the project's GEMM for ``dW`` (complete per chunk) and ``dh`` (summed over chunks in fp32).
* :func:`ref_linear_cross_entropy` -- the float64 statement, differentiable on any device.

``T`` and ``V`` are multiples of 128 and ``K`` of 64 (pad the head otherwise); ``h`` and ``w`` may be
column blocks of wider matrices (row strides that are multiples of 8, 16-byte aligned). A row
whose target is outside ``[0, V)`` is ignored: loss 0, a zero gradient, its lse still written.
No atomics, every output element written on every call, bitwise repeatable, capturable.
"""
from __future__ import annotations

import torch

from . import _lib
from .moe import _aligned
from .transformer import _bf16_matrix, _on_gpu, _row_vectors, _typed, _wants_grad, ref_cross_entropy_rows

CHUNK_BYTES = 256 << 20  # the default dlogits buffer of the backward: T * chunk * 2 bytes at most


def _check(h, w, target, tile: int = -1) -> tuple:
    _bf16_matrix(h, "h")
    _bf16_matrix(w, "w")
    _typed([("target", torch.int64, target)])
    (t, k), v = h.shape, w.shape[0]
    if w.shape[1] != k:
        raise ValueError(f"h [T, K] and w [V, K] must agree in K, got {tuple(h.shape)}, {tuple(w.shape)}")
    if t < 128 or v < 128 or k < 64 or t % 128 or v % 128 or k % 64:
        raise ValueError(f"T and V must be multiples of 128 and K of 64, got T {t}, V {v}, K {k}")
    for x, name in ((h, "h"), (w, "w")):
        if x.stride(0) < k or x.stride(0) % 8:
            raise ValueError(f"{name}: the row stride must be a multiple of 8 and at least K, got {x.stride(0)}")
    _row_vectors([("target", None, target)], t)
    if tile not in (-1, 0, 1) or (tile == 1 and t % 256):
        raise ValueError(f"tile must be -1, 0 or 1 (1 with T % 256 == 0 only), got {tile!r}")
    return t, v, k


def linear_cross_entropy_rows(h: torch.Tensor, w: torch.Tensor, target: torch.Tensor, *, tile: int = -1
                              ) -> tuple[torch.Tensor, torch.Tensor]:
    """``(loss, lse)``, fp32 ``[T]``, of the logits ``h @ w.T`` (bf16 ``h [T, K]``, ``w [V, K]``, int64
    ``target [T]``): ``lse`` the row's log-sum-exp over the fp32 accumulators (the logits are not
    rounded to bf16) and ``loss = lse - z[row, target[row]]``, 0 for an ignored row. Two launches
    and a workspace of one float2 per row and strip of 8 vocabulary tiles. ``tile`` is, as
    :func:`kgs.ops.moe_gemm`'s, a measurement knob for the tile-shape A/B and the tests, not a tuning
    option: -1 takes 256 x 128 tiles where ``T % 256 == 0`` and 128 x 128 otherwise; same bits either way."""
    t, v, k = _check(h, w, target, tile)
    _on_gpu((h, "h"), (w, "w"), (target, "target"))
    _aligned((h, "h"), (w, "w"))
    lib = _lib.lib()
    loss = torch.empty(t, dtype=torch.float32, device=h.device)
    lse = torch.empty(t, dtype=torch.float32, device=h.device)
    ws = torch.empty(lib.kgs_linear_xent_workspace(t, v) // 4, dtype=torch.float32, device=h.device)
    rc = lib.kgs_linear_xent_fwd_bf16(h.data_ptr(), w.data_ptr(), target.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                                      ws.data_ptr(), t, v, k, h.stride(0), w.stride(0), tile,
                                      _lib.stream_handle(h.device))
    _lib.check(rc, f"linear_cross_entropy_rows[{t}x{v}x{k}]")
    return loss, lse


def linear_cross_entropy_dlogits(h: torch.Tensor, w: torch.Tensor, target: torch.Tensor, lse: torch.Tensor,
                                 grow: torch.Tensor, cols: tuple | None = None, out: torch.Tensor | None = None,
                                 *, tile: int = -1) -> torch.Tensor:
    """The columns ``cols = (v0, v1)`` (multiples of 128; default all) of the loss' gradient with
    respect to the logits, bf16 ``[T, v1 - v0]``: ``grow[row] * (exp(z - lse[row]) - [col ==
    target[row]])`` with ``z`` recomputed in fp32 and ``p - 1`` at the target taken as ``expm1(z -
    lse)``, which adds no cancellation to the error of ``z - lse`` (where ``p`` is 1 in fp32, ``lse`` equals
    ``z`` and the entry is 0, within ``grow * 2^-24`` of the truth); ignored rows are zeros. ``lse``, ``grow``:
    fp32 ``[T]``. ``out``: a buffer of its own (any row stride that is a multiple of 8)."""
    t, v, k = _check(h, w, target, tile)
    vecs = [("lse", torch.float32, lse), ("grow", torch.float32, grow)]
    _typed(vecs)
    _row_vectors(vecs, t)
    v0, v1 = (0, v) if cols is None else (int(cols[0]), int(cols[1]))
    if not 0 <= v0 < v1 <= v or v0 % 128 or v1 % 128:
        raise ValueError(f"cols must be a range of multiples of 128 inside [0, {v}], got {(v0, v1)}")
    if out is not None:
        _bf16_matrix(out, "out", (t, v1 - v0))
        if out.stride(0) % 8:
            raise ValueError("out: the row stride must be a multiple of 8")
    _on_gpu((h, "h"), (w, "w"), (target, "target"), (lse, "lse"), (grow, "grow"), (out, "out"))
    if out is None:
        out = torch.empty((t, v1 - v0), dtype=torch.bfloat16, device=h.device)
    _aligned((h, "h"), (w, "w"), (out, "out"))
    rc = _lib.lib().kgs_linear_xent_dlogits_bf16(h.data_ptr(), w[v0:].data_ptr(), target.data_ptr(), lse.data_ptr(),
                                                 grow.data_ptr(), out.data_ptr(), t, v1 - v0, k, h.stride(0),
                                                 w.stride(0), out.stride(0), v0, v, tile,
                                                 _lib.stream_handle(h.device))
    _lib.check(rc, f"linear_cross_entropy_dlogits[{t}x{v1 - v0}x{k}]")
    return out


def ref_linear_cross_entropy(h, w, target, dtype=torch.float64):
    """``(loss, lse)`` of :func:`linear_cross_entropy_rows` in ``dtype``: differentiable."""
    return ref_cross_entropy_rows(h.to(dtype) @ w.to(dtype).T, target, dtype)


def default_chunk(t: int, v: int) -> int:
    """The backward's columns per chunk: the largest multiple of 256 whose dlogits buffer stays
    within ``CHUNK_BYTES``, at least 256, at most ``v``."""
    return min(v, max(256, CHUNK_BYTES // (2 * t) // 256 * 256))


class _LinearXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, target, chunk):
        loss, lse = linear_cross_entropy_rows(h, w, target)
        ctx.save_for_backward(h, w, target, lse)
        ctx.chunk = chunk
        return loss

    @staticmethod
    def backward(ctx, grow):
        from .gemm import gemm_bf16

        h, w, target, lse = ctx.saved_tensors
        (t, k), v, chunk = h.shape, w.shape[0], ctx.chunk
        grow = grow.float().contiguous()
        want_h, want_w = ctx.needs_input_grad[:2]
        buf = torch.empty(t * min(chunk, v), dtype=torch.bfloat16, device=h.device)
        dw = torch.empty((v, k), dtype=torch.bfloat16, device=h.device) if want_w else None
        dh = acc = None
        for v0 in range(0, v, chunk):
            v1 = min(v, v0 + chunk)
            dl = linear_cross_entropy_dlogits(h, w, target, lse, grow, (v0, v1),
                                              out=buf[:t * (v1 - v0)].view(t, v1 - v0))
            if want_w:  # dW[v0:v1] = dl^T . h, complete: straight into its rows
                gemm_bf16(dl, h, trans_a=True, out=dw[v0:v1])
            if want_h:  # dh = sum over chunks of dl . w[v0:v1], summed in fp32, rounded once
                part = gemm_bf16(dl, w[v0:v1])
                if chunk >= v:
                    dh = part
                elif acc is None:
                    acc = part.float()
                else:
                    acc.add_(part)
        if acc is not None:
            dh = acc.to(torch.bfloat16)
        return dh, dw, None, None


def linear_cross_entropy(h: torch.Tensor, w: torch.Tensor, target: torch.Tensor, chunk: int | None = None
                         ) -> torch.Tensor:
    """Differentiable :func:`linear_cross_entropy_rows`: the fp32 per-row loss ``[T]`` of the head
    ``w`` on the hidden state ``h`` (0 for ignored rows; the caller takes the mean over the others).
    It saves ``h``, ``w``, ``target`` and the rows' log-sum-exp, never the logits; with no gradient
    wanted it saves nothing. The backward walks the vocabulary in chunks of ``chunk`` columns (a
    multiple of 128; default :func:`default_chunk`; the last chunk takes the remainder):
    :func:`linear_cross_entropy_dlogits` into one reused buffer, ``dW[v0:v1]`` from it in one GEMM,
    and ``dh`` as the fp32 sum of the chunks' products. The chunk count depends on the shapes only."""
    t, v, _ = _check(h, w, target)
    if chunk is None:
        chunk = default_chunk(t, v)
    if not isinstance(chunk, int) or chunk < 128 or chunk % 128:
        raise ValueError(f"chunk must be a positive multiple of 128, got {chunk!r}")
    _on_gpu((h, "h"), (w, "w"), (target, "target"))
    if not _wants_grad(h, w):
        return linear_cross_entropy_rows(h, w, target)[0]
    return _LinearXentFn.apply(h, w, target, chunk)
