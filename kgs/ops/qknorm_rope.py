"""QK-norm fused with RoPE on the kernels of ``native/kernels/qknorm_rope.hip``: the
per-head RMSNorm that Qwen3, OLMo-2 and Gemma-3 apply to q and k before the
rotation, as one forward and one backward kernel over the fused QKV row.

With ``qkv [T, (H + 2 HKV) * 128]`` bf16 (q heads, k heads, v heads), ``wq``, ``wk``
``[128]`` bf16 and fp32 ``cos`` / ``sin`` tables ``[npos, 64]``, for every 128-wide
head row ``x`` of the ``H`` q heads (``w = wq``) and the ``HKV`` k heads (``w = wk``) at
position ``p`` (``pos[t]``, or ``t % seq``)::

    r   = rsqrt(mean(x^2) + eps)
    n   = x * r * w                          (fp32, not rounded)
    out = bf16(rotate_half(n, cos[p], sin[p]))

The v heads are not touched. The Hugging Face implementations round ``n`` to bf16
before they rotate it; this op rounds once, after the rotation, like every other
kernel here. Backward, from ``dy`` (the whole fused row) and the saved pre-norm
head rows::

    g  = rotate_half(dy, cos[p], -sin[p])    nh = x * r      gw = g * w
    dx = bf16(r * (gw - nh * mean(gw * nh)))  dw = sum g * nh   dv = dy

``dwq`` sums over the tokens and the q heads, ``dwk`` over the tokens and the k
heads, in fp32 in an order fixed by ``(T, H, HKV)``: no atomics, bitwise repeatable,
capturable in a graph.

:func:`ref_qknorm_rope` and :func:`ref_qknorm_rope_backward` state the formulas in
torch ops on any device (float64 by default): the model for the tests, and the
torch path of :class:`kgs.models.decoder.DecoderLayer`.
"""
from __future__ import annotations

import sys
import types

import torch

from . import _lib
from .transformer import _bf16_matrix, _grad_rows, _on_gpu, _wants_grad

HD = 128


class _CallableModule(types.ModuleType):
    """``kgs.ops.qknorm_rope`` names both this module and the op (as
    ``kgs.ops.embedding`` does): the module is callable as the op."""

    def __call__(self, *args, **kwargs):
        return qknorm_rope(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule


# ---------------------------------------------------------------------------
# argument checks: dtype and shape before the device, all before the library
def _check_heads(heads, kv_heads) -> int:
    for v, n in ((heads, "heads"), (kv_heads, "kv_heads")):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{n} must be an int")
        if v < 1:
            raise ValueError(f"{n} must be at least 1")
    return (heads + 2 * kv_heads) * HD


def _check_rows(t, name: str, cols: int, rows: int | None = None) -> None:
    _bf16_matrix(t, name)
    if t.shape[1] != cols or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name} must be [{'rows' if rows is None else rows}, {cols}], got {tuple(t.shape)}")
    if t.shape[0] > 1 and (t.stride(0) < cols or t.stride(0) % 8):
        raise ValueError(f"{name}: the row stride must be a multiple of 8 elements, at least {cols}")


def _check_weights(wq, wk) -> None:
    for w, n in ((wq, "wq"), (wk, "wk")):
        if not isinstance(w, torch.Tensor) or w.dtype != torch.bfloat16:
            raise TypeError(f"{n} must be a bf16 tensor")
        if w.shape != (HD,) or not w.is_contiguous():
            raise ValueError(f"{n} must be a contiguous bf16 vector of length {HD}")


def _check_positions(cos, sin, seq, pos, rows: int) -> None:
    for t, n in ((cos, "cos"), (sin, "sin")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{n} must be an fp32 tensor")
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != HD // 2 or not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous fp32 [npos, {HD // 2}]")
    if cos.shape != sin.shape:
        raise ValueError("cos and sin must have one shape")
    if pos is None:
        if isinstance(seq, bool) or not isinstance(seq, int):
            raise TypeError("seq must be an int")
        if not 0 < seq <= cos.shape[0]:
            raise ValueError("without pos, seq must be positive and the tables must hold seq rows")
        return
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int32:
        raise TypeError("pos must be an int32 tensor")
    if pos.shape != (rows,) or not pos.is_contiguous():
        raise ValueError("pos must be a contiguous vector with one entry per row of qkv")


def _check_eps(eps) -> float:
    if isinstance(eps, torch.Tensor) or not isinstance(eps, (int, float)):
        raise TypeError("eps must be a number")
    return float(eps)


def _aligned(*named) -> None:
    for t, name in named:
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")


def _ld(t: torch.Tensor) -> int:
    # a view of at most one row may carry any row stride: the kernels never use it
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


_WS: dict = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """The per-GPU fp32 buffer of the backward's partial dw rows. A buffer it
    outgrows is retired, not freed: graphs captured earlier still point at it."""
    from .decode import device_key, retire

    key = device_key(device)
    ws = _WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        retire(ws)
        ws = _WS[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return ws


# ---------------------------------------------------------------------------
# raw ops
def qknorm_rope_(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 heads: int, kv_heads: int, seq: int, pos: torch.Tensor | None = None, eps: float = 1e-6,
                 save: torch.Tensor | None = None, _wgs: int = 0) -> torch.Tensor:
    """Normalise and rotate, in place, the q and k heads of ``qkv [T, (heads + 2
    kv_heads) * 128]`` (any row stride that is a multiple of 8) and return it; the v
    heads keep their bits. ``n = x * rsqrt(mean(x^2) + eps) * w`` stays in fp32 and
    the rotated value is rounded once (the Hugging Face models round ``n`` first).
    Positions are ``pos`` (int32 ``[T]``, each inside the tables) or ``t % seq``.
    ``save``: a bf16 ``[T, (heads + kv_heads) * 128]`` view that receives the pre-norm
    q and k heads in the same pass (what :func:`qknorm_rope_backward` reads);
    without it nothing is kept."""
    width = _check_heads(heads, kv_heads)
    _check_rows(qkv, "qkv", width)
    rows = qkv.shape[0]
    _check_weights(wq, wk)
    _check_positions(cos, sin, seq, pos, rows)
    eps = _check_eps(eps)
    if save is not None:
        _check_rows(save, "save", (heads + kv_heads) * HD, rows)
    _on_gpu((qkv, "qkv"), (wq, "wq"), (wk, "wk"), (cos, "cos"), (sin, "sin"), (pos, "pos"), (save, "save"))
    _aligned((qkv, "qkv"), (wq, "wq"), (wk, "wk"), (save, "save"))
    rc = _lib.lib().kgs_qknorm_rope_fwd_bf16(
        qkv.data_ptr(), 0 if save is None else save.data_ptr(), wq.data_ptr(), wk.data_ptr(), cos.data_ptr(),
        sin.data_ptr(), 0 if pos is None else pos.data_ptr(), rows, heads, kv_heads, HD, _ld(qkv),
        0 if save is None else _ld(save), 0 if pos is not None else seq, cos.shape[0], eps, _wgs,
        _lib.stream_handle(qkv.device))
    _lib.check(rc, f"qknorm_rope[{rows}x{heads}+{kv_heads}]")
    return qkv


def qknorm_rope_backward(dy: torch.Tensor, save: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos: torch.Tensor,
                         sin: torch.Tensor, heads: int, kv_heads: int, seq: int, pos: torch.Tensor | None = None,
                         eps: float = 1e-6, _wgs: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(dx, dwq, dwk)`` of :func:`qknorm_rope_`: bf16 ``[T, (heads + 2 kv_heads) *
    128]``, ``[128]`` and ``[128]``, from ``dy`` (the gradient of the whole fused row;
    only read) and ``save`` (the forward's pre-norm q and k heads; a ``qkv`` from
    before the forward serves as well). ``dx``'s v columns are ``dy``'s bits. ``dwq`` /
    ``dwk`` are summed in fp32 in a fixed order and rounded once: two launches, no
    atomics, the same bits on every call."""
    width = _check_heads(heads, kv_heads)
    _check_rows(dy, "dy", width)
    rows = dy.shape[0]
    _bf16_matrix(save, "save")
    if save.shape[1] not in ((heads + kv_heads) * HD, width):
        raise ValueError(f"save must hold the {(heads + kv_heads) * HD} pre-norm q and k columns")
    _check_rows(save, "save", save.shape[1], rows)
    _check_weights(wq, wk)
    _check_positions(cos, sin, seq, pos, rows)
    eps = _check_eps(eps)
    _on_gpu((dy, "dy"), (save, "save"), (wq, "wq"), (wk, "wk"), (cos, "cos"), (sin, "sin"), (pos, "pos"))
    _aligned((dy, "dy"), (save, "save"), (wq, "wq"), (wk, "wk"))
    dx = torch.empty((rows, width), dtype=torch.bfloat16, device=dy.device)
    if rows == 0:
        return dx, torch.zeros_like(wq), torch.zeros_like(wk)
    dwq, dwk = torch.empty_like(wq), torch.empty_like(wk)
    lib = _lib.lib()
    ws = _workspace(dy.device, lib.kgs_qknorm_rope_bwd_workspace(rows, heads, kv_heads))
    rc = lib.kgs_qknorm_rope_bwd_bf16(
        dy.data_ptr(), save.data_ptr(), wq.data_ptr(), wk.data_ptr(), cos.data_ptr(), sin.data_ptr(),
        0 if pos is None else pos.data_ptr(), dx.data_ptr(), dwq.data_ptr(), dwk.data_ptr(), ws.data_ptr(), rows,
        heads, kv_heads, HD, _ld(dy), _ld(save), width, 0 if pos is not None else seq, cos.shape[0], eps, _wgs,
        _lib.stream_handle(dy.device))
    _lib.check(rc, f"qknorm_rope_backward[{rows}x{heads}+{kv_heads}]")
    return dx, dwq, dwk


# ---------------------------------------------------------------------------
# the autograd op
class _QkNormRopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, wq, wk, cos, sin, heads, kv_heads, seq, pos, eps):
        save = torch.empty((qkv.shape[0], (heads + kv_heads) * HD), dtype=torch.bfloat16, device=qkv.device)
        if qkv.is_leaf or qkv._base is not None:  # rope_qkv's rule: autograd forbids (a leaf) or restricts (a view)
            out = qkv.clone(memory_format=torch.contiguous_format)
        else:
            ctx.mark_dirty(qkv)
            out = qkv
        qknorm_rope_(out, wq, wk, cos, sin, heads, kv_heads, seq, pos, eps, save=save)
        ctx.save_for_backward(save, wq, wk, cos, sin, pos)
        ctx.cfg = (heads, kv_heads, seq, eps)
        return out

    @staticmethod
    def backward(ctx, dout):
        save, wq, wk, cos, sin, pos = ctx.saved_tensors
        heads, kv_heads, seq, eps = ctx.cfg
        dx, dwq, dwk = qknorm_rope_backward(_grad_rows(dout), save, wq, wk, cos, sin, heads, kv_heads, seq, pos, eps)
        return dx, dwq, dwk, None, None, None, None, None, None, None


def qknorm_rope(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                heads: int, kv_heads: int, seq: int, pos: torch.Tensor | None = None,
                eps: float = 1e-6) -> torch.Tensor:
    """Differentiable :func:`qknorm_rope_`: returns the normalised and rotated rows.
    With no gradient wanted (of ``qkv``, ``wq`` or ``wk``) this IS :func:`qknorm_rope_`,
    in place, nothing saved. Otherwise the forward runs in place where autograd
    allows it (a non-leaf ``qkv`` that is not a view: ``qkv`` itself is returned,
    marked dirty), else on a copy, and writes the pre-norm q and k heads to a buffer
    of its own in the same pass; the backward is one :func:`qknorm_rope_backward`
    call, which only reads the incoming gradient. Rounds once (see the module)."""
    if not _wants_grad(qkv, wq, wk):
        return qknorm_rope_(qkv, wq, wk, cos, sin, heads, kv_heads, seq, pos, eps)
    width = _check_heads(heads, kv_heads)
    _check_rows(qkv, "qkv", width)
    _check_weights(wq, wk)
    _check_positions(cos, sin, seq, pos, qkv.shape[0])
    eps = _check_eps(eps)
    _on_gpu((qkv, "qkv"), (wq, "wq"), (wk, "wk"), (cos, "cos"), (sin, "sin"), (pos, "pos"))
    return _QkNormRopeFn.apply(qkv, wq, wk, cos, sin, heads, kv_heads, seq, pos, eps)


# ---------------------------------------------------------------------------
# the model: the same formulas in torch ops
def _heads_of(x, wq, wk, heads, kv_heads, eps, dtype):
    t = x.shape[0]
    xh = x[:, :(heads + kv_heads) * HD].to(dtype).reshape(t, heads + kv_heads, HD)
    w = torch.cat((wq.to(dtype).expand(heads, HD), wk.to(dtype).expand(kv_heads, HD)))
    return xh, torch.rsqrt(xh.pow(2).mean(-1, keepdim=True) + eps), w


def _tables_at(cos, sin, rows, seq, pos, dtype):
    p = pos.long() if pos is not None else torch.arange(rows, device=cos.device) % seq
    return cos[p].to(dtype)[:, None, :], sin[p].to(dtype)[:, None, :]


def _rotate_half(x, c, s):
    x1, x2 = x[..., :HD // 2], x[..., HD // 2:]
    return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1)


def ref_qknorm_rope(qkv, wq, wk, cos, sin, heads, kv_heads, seq, pos=None, eps=1e-6, dtype=torch.float64):
    """:func:`qknorm_rope_` evaluated in ``dtype`` (not rounded, not in place): ``[T,
    (heads + 2 kv_heads) * 128]``, the v columns as they are. Differentiable."""
    t = qkv.shape[0]
    xh, r, w = _heads_of(qkv, wq, wk, heads, kv_heads, eps, dtype)
    c, s = _tables_at(cos, sin, t, seq, pos, dtype)
    rot = _rotate_half(xh * r * w, c, s).reshape(t, (heads + kv_heads) * HD)
    return torch.cat((rot, qkv[:, (heads + kv_heads) * HD:].to(dtype)), dim=1)


def ref_qknorm_rope_backward(dy, x, wq, wk, cos, sin, heads, kv_heads, seq, pos=None, eps=1e-6,
                             dtype=torch.float64):
    """``(dx, dwq, dwk)`` of :func:`qknorm_rope_backward` in ``dtype``, unrounded, from
    ``dy`` and the pre-norm rows ``x`` (``save``, or the ``qkv`` the forward was given)."""
    t, nqk = dy.shape[0], (heads + kv_heads) * HD
    xh, r, w = _heads_of(x, wq, wk, heads, kv_heads, eps, dtype)
    c, s = _tables_at(cos, sin, t, seq, pos, dtype)
    g = _rotate_half(dy[:, :nqk].to(dtype).reshape(t, heads + kv_heads, HD), c, -s)
    nhat, gw = xh * r, g * w
    dx = r * (gw - nhat * (gw * nhat).mean(-1, keepdim=True))
    dw = (g * nhat).sum(0)
    return (torch.cat((dx.reshape(t, nqk), dy[:, nqk:].to(dtype)), dim=1), dw[:heads].sum(0), dw[heads:].sum(0))
