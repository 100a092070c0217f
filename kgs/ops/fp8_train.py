"""A trainable fp8 Linear: all three GEMMs of a ``Linear`` (forward, dX, dW) on
the e4m3 MFMA GEMM, fed by the fused amax / quantise kernels of
``native/kernels/fp8_train.hip``.

The recipe. Storage is OCP e4m3fn, ``scale(a) = max(a, 1e-12) / 448`` and
``q(x, s) = e4m3(clamp(x * (1 / s), +-448))``. With ``x [T, K]``, ``w [N, K]``,
``dy [T, N]`` in bf16, every product is an NT GEMM on :func:`kgs.ops.gemm_fp8_rows`
(A with per-row scales, B with one per-tensor scale)::

    y  = x8  [T, K] (scale per token)            . w8  [N, K] (sw)
    dx = dy8 [T, N] (scale per token)            . w8t [K, N] = w8^T (sw)
    dw = dy8t[N, T] (scale per output feature)   . x8t [K, T] (sx, per tensor)

B's scale is a device scalar and the GEMM takes only a host float for it, so it
is folded into A's stored row scales when A is quantised (the GEMM then runs
with ``alpha = 1``). The forward saves ``x8t`` and ``sx`` (one byte per element
of ``x``, not two), ``w`` itself and the weight's amax / scale; the backward
rebuilds ``w8t`` from ``w`` with that amax: one quantise pass, the forward's
codes. The weight is quantised again on every forward: :class:`kgs.optim.AdamW`
writes weights through raw pointers, so no cache keyed on ``_version`` would be
safe.

A NaN or Inf in an operand makes the scales that cover it non-finite, and the
GEMM's epilogue multiplies them into every output it touches: a bad step stays
visible to the optimizer's skip-on-non-finite-norm.

:func:`ref_linear_fp8` is the same recipe in torch ops on any device (the model
for the tests and the ``backend="torch"`` decoder).
"""
from __future__ import annotations

import torch

from . import _lib

FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0
TINY = 1e-12


# ---------------------------------------------------------------------------
# argument checks: dtype and shape before the device, so a wrong call fails the
# same way everywhere, and all of them before the native library is touched
def _check_matrix(x: torch.Tensor, name: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be a bf16 tensor")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"{name} must be a row-major 2-D matrix")
    rows, cols = x.shape
    if rows <= 0 or cols <= 0 or rows % 16 or cols % 16:
        raise ValueError(f"{name}: rows and cols must be positive multiples of 16, got {rows} x {cols}")
    if x.stride(0) < cols or x.stride(0) % 8:
        raise ValueError(f"{name}: the row stride must be a multiple of 8 elements")


def _check_place(x: torch.Tensor, name: str) -> None:
    if not x.is_cuda:
        raise ValueError(f"{name} must be on a GPU")
    if x.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")


def _check_vec(v, name: str, n: int, like: torch.Tensor):
    if v is None:
        return None
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32:
        raise TypeError(f"{name} must be an fp32 tensor")
    if v.numel() != n or not v.is_contiguous():
        raise ValueError(f"{name} must be a contiguous vector of {n} floats")
    if v.device != like.device:
        raise ValueError(f"{name} must be on {like.device}")
    return v


def _check_image(img, name: str, rows: int, cols: int, like: torch.Tensor):
    """``img``: False / None (not wanted), True (allocate) or a ``[rows, cols]``
    e4m3 view to write into (row-major, row stride a multiple of 16)."""
    if img is None or img is False:
        return None
    if img is True:
        return True
    if not isinstance(img, torch.Tensor) or img.dtype != FP8_DTYPE:
        raise TypeError(f"{name} must be an {FP8_DTYPE} tensor")
    if img.dim() != 2 or img.stride(1) != 1 or tuple(img.shape) != (rows, cols):
        raise ValueError(f"{name} must be a row-major [{rows}, {cols}] matrix")
    if img.stride(0) < cols or img.stride(0) % 16 or img.data_ptr() % 16:
        raise ValueError(f"{name}: the row stride must be a multiple of 16 and the data 16-byte aligned")
    if img.device != like.device:
        raise ValueError(f"{name} must be on {like.device}")
    return img


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------
# raw ops
def fp8_amax(x: torch.Tensor, rows: bool = False, cols: bool = False, tensor: bool = False):
    """``|x|`` maxima of a bf16 matrix in one pass over it: returns ``(row_amax
    [rows], col_amax [cols], tensor_amax [1])`` as fp32, ``None`` for those not
    asked for. Bit-equal to ``x.float().abs().amax(...)``, NaN and Inf included
    (NaN wins over Inf, Inf over every finite value)."""
    _check_matrix(x, "x")
    if not (rows or cols or tensor):
        raise ValueError("fp8_amax: ask for at least one of rows, cols, tensor")
    _check_place(x, "x")
    r, c = x.shape
    ra = torch.empty(r, dtype=torch.float32, device=x.device) if rows else None
    ca = torch.empty(c, dtype=torch.float32, device=x.device) if cols else None
    ta = torch.empty(1, dtype=torch.float32, device=x.device) if tensor else None
    rc = _lib.lib().kgs_fp8_amax_bf16(x.data_ptr(), r, c, x.stride(0), _ptr(ra), _ptr(ca), _ptr(ta),
                                      _lib.stream_handle(x.device))
    _lib.check(rc, f"fp8_amax[{r}x{c}]")
    return ra, ca, ta


def fp8_quantize(x: torch.Tensor, row_amax: torch.Tensor | None = None, col_amax: torch.Tensor | None = None,
                 tensor_amax: torch.Tensor | None = None, y=True, yt=False, y_fold: torch.Tensor | None = None,
                 yt_fold: torch.Tensor | None = None):
    """One pass over the bf16 matrix ``x [rows, cols]`` that writes ``y [rows,
    cols]`` and / or the transpose ``yt [cols, rows]`` as e4m3.

    ``y`` is scaled per row when ``row_amax`` is given, else per tensor from
    ``tensor_amax``; ``yt`` per output row when ``col_amax`` is given, else per
    tensor. ``y`` / ``yt``: ``True`` (allocate), ``False`` or a preallocated
    e4m3 view. ``y_fold`` / ``yt_fold``: 1-element fp32 device tensors multiplied
    into the returned scales only (the codes use the unfolded scale). Returns
    ``(y, y_scale, yt, yt_scale)`` with ``x ~= y.float() * y_scale[:, None]``
    (unfolded) and likewise for ``yt``; a scale is ``[rows]`` / ``[cols]`` or
    ``[1]``. With both images per tensor ``yt`` is ``y.T`` bit for bit."""
    _check_matrix(x, "x")
    r, c = x.shape
    y = _check_image(y, "y", r, c, x)
    yt = _check_image(yt, "yt", c, r, x)
    if y is None and yt is None:
        raise ValueError("fp8_quantize: ask for at least one of y, yt")
    row_amax = _check_vec(row_amax, "row_amax", r, x)
    col_amax = _check_vec(col_amax, "col_amax", c, x)
    tensor_amax = _check_vec(tensor_amax, "tensor_amax", 1, x)
    y_fold = _check_vec(y_fold, "y_fold", 1, x)
    yt_fold = _check_vec(yt_fold, "yt_fold", 1, x)
    if y is not None and row_amax is None and tensor_amax is None:
        raise ValueError("fp8_quantize: y needs row_amax or tensor_amax")
    if yt is not None and col_amax is None and tensor_amax is None:
        raise ValueError("fp8_quantize: yt needs col_amax or tensor_amax")
    _check_place(x, "x")
    ys = yts = None
    if y is not None:
        if y is True:
            y = torch.empty((r, c), dtype=FP8_DTYPE, device=x.device)
        ys = torch.empty(r if row_amax is not None else 1, dtype=torch.float32, device=x.device)
    if yt is not None:
        if yt is True:
            yt = torch.empty((c, r), dtype=FP8_DTYPE, device=x.device)
        yts = torch.empty(c if col_amax is not None else 1, dtype=torch.float32, device=x.device)
    rc = _lib.lib().kgs_fp8_quant_bf16(
        x.data_ptr(), r, c, x.stride(0), _ptr(row_amax), _ptr(col_amax), _ptr(tensor_amax),
        _ptr(y), y.stride(0) if y is not None else 0, _ptr(ys),
        _ptr(yt), yt.stride(0) if yt is not None else 0, _ptr(yts),
        _ptr(y_fold) if y is not None else None, _ptr(yt_fold) if yt is not None else None,
        _lib.stream_handle(x.device))
    _lib.check(rc, f"fp8_quantize[{r}x{c}]")
    return y, ys, yt, yts


# ---------------------------------------------------------------------------
# the Linear
def _check_linear(x, w, bias) -> None:
    for t, name in ((x, "x"), (w, "w")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
            raise TypeError(f"{name} must be a bf16 tensor")
        if t.dim() != 2:
            raise ValueError(f"{name} must be a 2-D matrix")
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"inner dims differ: x {tuple(x.shape)} w {tuple(w.shape)}")
    T, K = x.shape
    N = w.shape[0]
    if T % 16 or K % 16 or N % 16 or min(T, K, N) <= 0:
        raise ValueError(f"linear_fp8: T, K and N must be positive multiples of 16, got {T}, {K}, {N} "
                         "(there is no bf16 fallback)")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.bfloat16:
            raise TypeError("bias must be a bf16 tensor")
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous bf16 vector of length N")
    _check_matrix(x, "x")
    _check_matrix(w, "w")
    _check_place(x, "x")
    _check_place(w, "w")


class _LinearFp8Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        from .gemm import gemm_fp8_rows

        _check_linear(x, w, bias)
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        w_amax = fp8_amax(w, tensor=True)[2]
        w8, sw, _, _ = fp8_quantize(w, tensor_amax=w_amax)
        x_row, _, x_ten = fp8_amax(x, rows=True, tensor=need_dw)
        # x8 carries sw in its row scales; x8t (for dW) keeps its own per-tensor sx
        x8, xs, x8t, sx = fp8_quantize(x, row_amax=x_row, tensor_amax=x_ten, y=True, yt=need_dw, y_fold=sw)
        y = gemm_fp8_rows(x8, xs, w8, 1.0, bias=bias)
        ctx.has_bias = bias is not None
        if need_dw:
            ctx.save_for_backward(w, w_amax, sw, x8t, sx)
        elif need_dx:
            ctx.save_for_backward(w, w_amax, sw)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .gemm import gemm_fp8_rows

        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        dy = dy.contiguous()
        dx = dw = db = None
        if need_dx or need_dw:
            saved = ctx.saved_tensors
            w, w_amax, sw = saved[:3]
            x8t, sx = saved[3:] if need_dw else (None, None)
            d_row, d_col, _ = fp8_amax(dy, rows=need_dx, cols=need_dw)
            dy8, dys, dy8t, dyts = fp8_quantize(dy, row_amax=d_row, col_amax=d_col, y=need_dx, yt=need_dw,
                                                y_fold=sw, yt_fold=sx)
            if need_dx:
                w8t = fp8_quantize(w, tensor_amax=w_amax, y=False, yt=True)[2]  # the forward's codes, transposed
                dx = gemm_fp8_rows(dy8, dys, w8t, 1.0)
            if need_dw:
                dw = gemm_fp8_rows(dy8t, dyts, x8t, 1.0)
        if need_db:
            db = dy.float().sum(0).to(torch.bfloat16)
        return dx, dw, db


def linear_fp8(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Differentiable ``x @ w.T + bias`` (x: [T, K], w: [N, K], bf16) whose
    forward, dX and dW GEMMs run in e4m3 (module docstring). ``T``, ``K`` and
    ``N`` must be multiples of 16: anything else raises ``ValueError``, there is
    no bf16 fallback. Nothing synchronises with the host; graph-capturable."""
    return _LinearFp8Fn.apply(x, w, bias)


class LinearFp8(torch.nn.Module):
    """``nn.Linear`` with a bf16 weight (so :class:`kgs.optim.AdamW` drives it
    unchanged) whose three GEMMs run in fp8: :func:`linear_fp8`.

    Measured on an MI355X (``profiles/r14/fp8_linear/README.md``), forward +
    backward against :class:`kgs.ops.Linear` at the Llama-3-8B projections with
    8192 and 16384 tokens: 1.33x (4096 -> 4096, 8192 tokens) to 1.70x (4096 ->
    28672, 16384 tokens); it lost at none of the eight shapes. Smaller
    products were not measured: the quantising path is ten launches whatever the
    size. The results carry e4m3's three mantissa bits: about 0.037 relative
    (Frobenius) error per product against the fp32 product."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None):
        super().__init__()
        w = torch.empty(out_features, in_features, dtype=torch.bfloat16, device=device)
        torch.nn.init.normal_(w, std=in_features ** -0.5)
        self.weight = torch.nn.Parameter(w)
        self.bias = torch.nn.Parameter(torch.zeros(out_features, dtype=torch.bfloat16, device=device)) if bias else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shp = x.shape
        y = linear_fp8(x.reshape(-1, shp[-1]).contiguous(), self.weight, self.bias)
        return y.reshape(*shp[:-1], y.shape[-1])


# ---------------------------------------------------------------------------
# the model: the same recipe in torch ops
def ref_scale(amax: torch.Tensor) -> torch.Tensor:
    """``max(amax, 1e-12) / 448``; a NaN or Inf amax gives a NaN or Inf scale."""
    return amax.float().clamp(min=TINY) / FP8_MAX


def ref_quantize(xf: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``e4m3(clamp(x * (1 / scale), +-448))`` with ``scale`` broadcast against ``xf`` (fp32)."""
    return (xf * (1.0 / scale)).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)


class _RefLinearFp8Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        xf, wf = x.detach().float(), w.detach().float()
        sw = ref_scale(wf.abs().amax())
        w8 = ref_quantize(wf, sw)
        xs = ref_scale(xf.abs().amax(dim=1))
        x8 = ref_quantize(xf, xs[:, None])
        y = (x8.float() * xs[:, None]) @ (w8.float() * sw).T
        if bias is not None:
            y = y + bias.detach().float()
        ctx.has_bias = bias is not None
        ctx.x_dtype = x.dtype
        if ctx.needs_input_grad[1]:
            sx = ref_scale(xf.abs().amax())
            ctx.save_for_backward(w, sw, ref_quantize(xf, sx).T.contiguous(), sx)
        elif ctx.needs_input_grad[0]:
            ctx.save_for_backward(w, sw)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dyf = dy.float()
        dx = dw = db = None
        if need_dx or need_dw:
            saved = ctx.saved_tensors
            w, sw = saved[:2]
            if need_dx:
                w8t = ref_quantize(w.detach().float(), sw).T
                ds = ref_scale(dyf.abs().amax(dim=1))
                dy8 = ref_quantize(dyf, ds[:, None])
                dx = ((dy8.float() * ds[:, None]) @ (w8t.float() * sw).T).to(ctx.x_dtype)
            if need_dw:
                x8t, sx = saved[2:]
                cs = ref_scale(dyf.abs().amax(dim=0))
                dy8t = ref_quantize(dyf, cs[None, :]).T
                dw = ((dy8t.float() * cs[:, None]) @ (x8t.float() * sx).T).to(w.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dyf.sum(0).to(dy.dtype)
        return dx, dw, db


def ref_linear_fp8(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`linear_fp8`'s recipe in torch ops, on any device and float dtype:
    quantise with torch, multiply the dequantised operands in fp32, round once
    to the input's dtype; the same tensors saved for the backward."""
    return _RefLinearFp8Fn.apply(x, w, bias)


class RefLinearFp8(torch.nn.Module):
    """``nn.Linear``-shaped module over :func:`ref_linear_fp8` (the
    ``backend="torch"`` decoder's fp8 Linear)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, dtype=torch.bfloat16):
        super().__init__()
        w = torch.empty(out_features, in_features, dtype=dtype, device=device)
        torch.nn.init.normal_(w, std=in_features ** -0.5)
        self.weight = torch.nn.Parameter(w)
        self.bias = torch.nn.Parameter(torch.zeros(out_features, dtype=dtype, device=device)) if bias else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shp = x.shape
        y = ref_linear_fp8(x.reshape(-1, shp[-1]), self.weight, self.bias)
        return y.reshape(*shp[:-1], y.shape[-1])
