"""Mixture-of-experts routing on the kernels of ``native/kernels/moe_route.hip``:
top-k selection with softmax weights, token-priority slots on fixed-capacity
slabs, the dispatch gather, the weighted combine, and their backwards. The FFNs
run as the existing Linears on the row slices ``xe[e * C:(e + 1) * C]``, or all at
once on the batched GEMM of ``native/kernels/moe_gemm.hip`` (:func:`moe_gemm`,
:func:`moe_linear`), which skips each slab's empty rows; either way every shape is
static and a step is capturable in a graph.

With ``logits [T, E]`` bf16 (``E`` a multiple of 8 in 8 .. 128), ``k = top_k`` in
``1 .. min(8, E)`` and ``C = capacity >= 1``::

    experts[t, j]  the k largest logits of row t, descending; ties to the lower index
    weights[t, :]  softmax over those k logits, fp32            (Mixtral; Qwen3 norm_topk_prob)
    f = t * k + j  the flat index;  rank(f) = #{f' < f : experts[f'] == experts[f]}
    slot[t, j]     e * C + rank if rank < C else -1 (dropped);  src[slot] = f, else -1
    counts[e]      the number of f routed to e, before dropping
    xe[s]          x[src[s] // k], a bit copy; a zero row for an empty slot
    y[t]           bf16(sum_j weights[t, j] * ye[slot[t, j]])    fp32, ascending j, drops skipped

Backwards: ``dx[t] = bf16(sum_j dxe[slot[t, j]])``; ``dye[s] = bf16(weights[f] *
dy[t])`` with exact zeros at empty slots; ``dweights[t, j] = dy[t] . ye[slot[t, j]]``
in fp32 (0 for a dropped ``j``); ``dlogits[t, e_j] = w_j (dw_j - sum_i w_i dw_i)`` in
bf16 and 0 in every column the row did not pick. A row with a NaN logit gets NaN
weights and indices that are still in range. Every element of every output is
written by a kernel on every call; no atomics, bitwise repeatable.

The ``ref_*`` functions state the same formulas in torch ops on any device
(float64 by default): the model for the tests and the torch path of
:class:`kgs.models.moe.MoEFFN`.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from .transformer import _bf16_matrix, _grad_rows, _on_gpu, _wants_grad

MAX_E, MAX_K = 128, 8


class Route(NamedTuple):
    """What :func:`moe_router` decided: ``weights`` fp32 ``[T, k]`` (differentiable),
    ``experts`` and ``slot`` int32 ``[T, k]``, ``src`` int32 ``[E * C]``, ``counts`` int32 ``[E]``."""
    weights: torch.Tensor
    experts: torch.Tensor
    slot: torch.Tensor
    src: torch.Tensor
    counts: torch.Tensor


# ---------------------------------------------------------------------------
# argument checks: dtype and shape before the device, all before the library
def _check_int(v, name: str, lo: int) -> None:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int")
    if v < lo:
        raise ValueError(f"{name} must be at least {lo}")


def _check_rows(t, name: str, rows: int | None = None, cols: int | None = None) -> None:
    _bf16_matrix(t, name)
    if (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols) or t.shape[0] < 1:
        raise ValueError(f"{name} must be [{rows or 'rows'}, {cols or 'cols'}], got {tuple(t.shape)}")
    if t.shape[1] % 8:
        raise ValueError(f"{name}: the columns must be a multiple of 8, got {t.shape[1]}")
    if t.shape[0] > 1 and (t.stride(0) < t.shape[1] or t.stride(0) % 8):
        raise ValueError(f"{name}: the row stride must be a multiple of 8 elements, at least {t.shape[1]}")


def _check_route_shape(num: int, top_k, capacity=1) -> None:
    _check_int(top_k, "top_k", 1)
    _check_int(capacity, "capacity", 1)
    if num % 8 or not 8 <= num <= MAX_E:
        raise ValueError(f"the number of experts must be a multiple of 8 in 8 .. {MAX_E}, got {num}")
    if top_k > min(MAX_K, num):
        raise ValueError(f"top_k must be at most min({MAX_K}, experts), got {top_k}")
    if num * capacity > 2 ** 31 - 1:
        raise ValueError("experts * capacity must fit 32 bits")


def _check_table(t, name: str, dtype, shape: tuple) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {str(dtype).removeprefix('torch.')} tensor")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous {tuple(shape)}, got {tuple(t.shape)}")


def _check_flat(t, name: str, dtype, rows: int | None = None) -> int:
    """A contiguous ``[T, k]`` table; returns k."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {str(dtype).removeprefix('torch.')} tensor")
    if t.dim() != 2 or not t.is_contiguous() or not 1 <= t.shape[1] <= MAX_K or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name} must be contiguous [{rows or 'T'}, k] with k in 1 .. {MAX_K}, got {tuple(t.shape)}")
    return t.shape[1]


def _aligned(*named) -> None:
    for t, name in named:
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


_WS: dict = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """The per-GPU int32 buffer of the rank passes' histograms. A buffer it outgrows
    is retired, not freed: graphs captured earlier still point at it."""
    from .decode import device_key, retire

    key = device_key(device)
    ws = _WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        retire(ws)
        ws = _WS[key] = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
    return ws


# ---------------------------------------------------------------------------
# raw ops
def moe_route(logits: torch.Tensor, top_k: int, capacity: int) -> Route:
    """Select, weigh and place: the :class:`Route` of ``logits [T, E]`` (bf16, any row
    stride that is a multiple of 8). Four launches, nothing synchronised."""
    _check_rows(logits, "logits")
    rows, num = logits.shape
    _check_route_shape(num, top_k, capacity)
    _on_gpu((logits, "logits"))
    _aligned((logits, "logits"))
    dev = logits.device
    weights = torch.empty((rows, top_k), dtype=torch.float32, device=dev)
    experts, slot = (torch.empty((rows, top_k), dtype=torch.int32, device=dev) for _ in range(2))
    src = torch.empty(num * capacity, dtype=torch.int32, device=dev)
    counts = torch.empty(num, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    ws = _workspace(dev, lib.kgs_moe_workspace(rows, num, top_k))
    rc = lib.kgs_moe_route_bf16(logits.data_ptr(), weights.data_ptr(), experts.data_ptr(), slot.data_ptr(),
                                src.data_ptr(), counts.data_ptr(), ws.data_ptr(), rows, num, top_k, capacity,
                                _ld(logits), _lib.stream_handle(dev))
    _lib.check(rc, f"moe_route[{rows}x{num}, k={top_k}, C={capacity}]")
    return Route(weights, experts, slot, src, counts)


def moe_route_backward(dweights: torch.Tensor, weights: torch.Tensor, experts: torch.Tensor,
                       num_experts: int) -> torch.Tensor:
    """``dlogits [T, E]`` bf16 from ``dweights`` / ``weights`` (fp32 ``[T, k]``) and
    ``experts`` (int32 ``[T, k]``): the softmax's backward scattered to the picked
    columns, zeros in the others."""
    k = _check_flat(weights, "weights", torch.float32)
    rows = weights.shape[0]
    _check_table(dweights, "dweights", torch.float32, (rows, k))
    _check_table(experts, "experts", torch.int32, (rows, k))
    _check_int(num_experts, "num_experts", 1)
    _check_route_shape(num_experts, k)
    if rows < 1:
        raise ValueError("weights must have at least one row")
    _on_gpu((dweights, "dweights"), (weights, "weights"), (experts, "experts"))
    dlogits = torch.empty((rows, num_experts), dtype=torch.bfloat16, device=weights.device)
    rc = _lib.lib().kgs_moe_route_bwd_bf16(dweights.data_ptr(), weights.data_ptr(), experts.data_ptr(),
                                           dlogits.data_ptr(), rows, num_experts, k, num_experts,
                                           _lib.stream_handle(weights.device))
    _lib.check(rc, f"moe_route_backward[{rows}x{num_experts}, k={k}]")
    return dlogits


def moe_gather(x: torch.Tensor, src: torch.Tensor, top_k: int, scale: torch.Tensor | None = None) -> torch.Tensor:
    """``out[s] = x[src[s] // top_k]``, a bit copy, and a zero row where ``src[s] < 0``:
    bf16 ``[len(src), D]``. With ``scale`` (fp32 ``[T, top_k]``, read by flat index)
    ``bf16(scale[src[s]] * x[src[s] // top_k])``: the combine's ``dye``."""
    _check_rows(x, "x")
    _check_int(top_k, "top_k", 1)
    if top_k > MAX_K:
        raise ValueError(f"top_k must be at most {MAX_K}")
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int32:
        raise TypeError("src must be an int32 tensor")
    if src.dim() != 1 or src.numel() < 1 or not src.is_contiguous():
        raise ValueError("src must be a contiguous int32 vector")
    if scale is not None:
        _check_table(scale, "scale", torch.float32, (x.shape[0], top_k))
    _on_gpu((x, "x"), (src, "src"), (scale, "scale"))
    _aligned((x, "x"))
    out = torch.empty((src.numel(), x.shape[1]), dtype=torch.bfloat16, device=x.device)
    rc = _lib.lib().kgs_moe_gather_bf16(x.data_ptr(), src.data_ptr(), 0 if scale is None else scale.data_ptr(),
                                        out.data_ptr(), x.shape[0], src.numel(), top_k, x.shape[1], _ld(x),
                                        x.shape[1], _lib.stream_handle(x.device))
    _lib.check(rc, f"moe_gather[{src.numel()}x{x.shape[1]}]")
    return out


def _combine(ye: torch.Tensor, slot: torch.Tensor, weights: torch.Tensor | None) -> torch.Tensor:
    _check_rows(ye, "ye")
    k = _check_flat(slot, "slot", torch.int32)
    if weights is not None:
        _check_table(weights, "weights", torch.float32, tuple(slot.shape))
    if slot.shape[0] < 1:
        raise ValueError("slot must have at least one row")
    _on_gpu((ye, "ye"), (slot, "slot"), (weights, "weights"))
    _aligned((ye, "ye"))
    y = torch.empty((slot.shape[0], ye.shape[1]), dtype=torch.bfloat16, device=ye.device)
    rc = _lib.lib().kgs_moe_combine_bf16(ye.data_ptr(), slot.data_ptr(), 0 if weights is None else weights.data_ptr(),
                                         y.data_ptr(), slot.shape[0], ye.shape[0], k, ye.shape[1], _ld(ye),
                                         ye.shape[1], _lib.stream_handle(ye.device))
    _lib.check(rc, f"moe_combine[{slot.shape[0]}x{ye.shape[1]}, k={k}]")
    return y


def moe_combine_backward(dy: torch.Tensor, ye: torch.Tensor, slot: torch.Tensor, src: torch.Tensor,
                         weights: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(dye, dweights)`` of the combine: bf16 ``[E * C, D]`` with exact zeros at empty
    slots, and fp32 ``[T, k]`` (0 for a dropped pick). Two launches."""
    _check_rows(ye, "ye")
    k = _check_flat(slot, "slot", torch.int32)
    rows = slot.shape[0]
    _check_rows(dy, "dy", rows, ye.shape[1])
    _check_table(weights, "weights", torch.float32, (rows, k))
    _check_table(src, "src", torch.int32, (ye.shape[0],))
    _on_gpu((dy, "dy"), (ye, "ye"), (slot, "slot"), (src, "src"), (weights, "weights"))
    _aligned((dy, "dy"), (ye, "ye"))
    dye = torch.empty((ye.shape[0], ye.shape[1]), dtype=torch.bfloat16, device=ye.device)
    dweights = torch.empty((rows, k), dtype=torch.float32, device=ye.device)
    rc = _lib.lib().kgs_moe_combine_bwd_bf16(dy.data_ptr(), ye.data_ptr(), slot.data_ptr(), src.data_ptr(),
                                             weights.data_ptr(), dye.data_ptr(), dweights.data_ptr(), rows,
                                             ye.shape[0], k, ye.shape[1], _ld(dy), _ld(ye), ye.shape[1],
                                             _lib.stream_handle(ye.device))
    _lib.check(rc, f"moe_combine_backward[{rows}x{ye.shape[1]}, k={k}]")
    return dye, dweights


# ---------------------------------------------------------------------------
# the autograd ops
class _RouterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, top_k, capacity):
        r = moe_route(logits, top_k, capacity)
        ctx.save_for_backward(r.weights, r.experts)
        ctx.num = logits.shape[1]
        ctx.mark_non_differentiable(r.experts, r.slot, r.src, r.counts)
        return tuple(r)

    @staticmethod
    def backward(ctx, dweights, *_):
        weights, experts = ctx.saved_tensors
        dweights = torch.zeros_like(weights) if dweights is None else dweights.contiguous()
        return moe_route_backward(dweights, weights, experts, ctx.num), None, None


class _DispatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, src, slot):
        ctx.save_for_backward(slot)
        return moe_gather(x, src, slot.shape[1])

    @staticmethod
    def backward(ctx, dxe):
        (slot,) = ctx.saved_tensors
        return _combine(_grad_rows(dxe), slot, None), None, None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ye, weights, slot, src):
        ctx.save_for_backward(ye, weights, slot, src)
        return _combine(ye, slot, weights)

    @staticmethod
    def backward(ctx, dy):
        ye, weights, slot, src = ctx.saved_tensors
        dye, dweights = moe_combine_backward(_grad_rows(dy), ye, slot, src, weights)
        return dye, dweights, None, None


def moe_router(logits: torch.Tensor, top_k: int, capacity: int) -> Route:
    """Differentiable :func:`moe_route`: ``route.weights`` carries the gradient back to
    ``logits`` through one :func:`moe_route_backward`. With no gradient wanted this IS
    :func:`moe_route`, nothing saved."""
    if not _wants_grad(logits):
        return moe_route(logits, top_k, capacity)
    _check_rows(logits, "logits")
    _check_route_shape(logits.shape[1], top_k, capacity)
    _on_gpu((logits, "logits"))
    return Route(*_RouterFn.apply(logits, top_k, capacity))


def moe_dispatch(x: torch.Tensor, route: Route) -> torch.Tensor:
    """``xe [E * C, D]``: the rows of ``x`` in slot order (:func:`moe_gather`). Its
    backward is the unweighted combine of ``dxe``. With no gradient wanted nothing
    is saved."""
    if not _wants_grad(x):
        return moe_gather(x, route.src, route.slot.shape[1])
    _check_rows(x, "x", route.slot.shape[0])
    _on_gpu((x, "x"), (route.src, "src"), (route.slot, "slot"))
    return _DispatchFn.apply(x, route.src, route.slot)


def moe_combine(ye: torch.Tensor, route, weights: torch.Tensor | None = None) -> torch.Tensor:
    """``y [T, D] = bf16(sum_j weights[t, j] * ye[slot[t, j]])``, dropped picks skipped.
    ``route`` is a :class:`Route` -- then the op is differentiable in ``ye`` and in
    ``route.weights``, and with no gradient wanted it is the raw forward, nothing
    saved -- or the raw ``slot`` table, with ``weights`` fp32 ``[T, k]`` or ``None`` for
    all ones (the dispatch's ``dx``): the raw forward."""
    if not isinstance(route, Route):
        return _combine(ye, route, weights)
    if not _wants_grad(ye, route.weights):
        return _combine(ye, route.slot, route.weights.detach())
    _check_rows(ye, "ye", route.src.numel())
    _on_gpu((ye, "ye"), (route.slot, "slot"), (route.weights, "weights"), (route.src, "src"))
    return _CombineFn.apply(ye, route.weights, route.slot, route.src)


# ---------------------------------------------------------------------------
# the batched expert GEMM (native/kernels/moe_gemm.hip)
GEMM_BK = 64        # mode 2 runs whole K-steps of this many columns: [n_e, roundup(n_e, GEMM_BK)) is read
MODES = {None: 0, "rows": 1, "reduce": 2}


def _check_batched(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be a bf16 tensor")
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"{name} must be [E, rows, cols] with unit column stride")
    if t.stride(1) < t.shape[2] or t.stride(1) % 8 or t.stride(0) < 0 or t.stride(0) % 8:
        raise ValueError(f"{name}: the row stride must be a multiple of 8 elements, at least {t.shape[2]}, and the "
                         "batch stride a non-negative multiple of 8")


def _check_gemm(a, b, counts, mode, out) -> tuple:
    if mode not in MODES:
        raise ValueError(f"mode must be None, 'rows' or 'reduce', not {mode!r}")
    _check_batched(a, "a")
    _check_batched(b, "b")
    (num, m, k), n = a.shape, b.shape[1]
    if b.shape[0] != num or b.shape[2] != k or num < 1:
        raise ValueError(f"a [E, M, K] and b [E, N, K] must agree in E and K, got {tuple(a.shape)}, {tuple(b.shape)}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % GEMM_BK:
        raise ValueError(f"M and N must be multiples of 128 and K of {GEMM_BK}, got M {m}, N {n}, K {k}")
    if (counts is None) != (mode is None):
        raise ValueError("counts and mode go together")
    if counts is not None:
        _check_table(counts, "counts", torch.int32, (num,))
    if out is not None:
        _check_batched(out, "out")
        if tuple(out.shape) != (num, m, n):
            raise ValueError(f"out must be {(num, m, n)}, got {tuple(out.shape)}")
        if num > 1 and out.stride(0) < m * out.stride(1):  # a and b may overlap or repeat; outputs may not
            raise ValueError(f"out: the batch stride must be at least M * the row stride, {m * out.stride(1)}")
    return num, m, n, k


def moe_gemm(a: torch.Tensor, b: torch.Tensor, counts: torch.Tensor | None = None, mode: str | None = None,
             out: torch.Tensor | None = None, *, tile: int = -1) -> torch.Tensor:
    """``out[e] = a[e] @ b[e].T`` for every e in one launch: bf16 ``a [E, M, K]``, ``b [E, N, K]``
    -> ``[E, M, N]``, fp32 accumulation in ascending k, rounded once. Any row and batch
    strides that are multiples of 8 elements (an operand may be a column block of a wider
    matrix); ``M``, ``N`` multiples of 128, ``K`` of 64. ``counts`` (int32 ``[E]``, read on the
    device) with ``n_e = clamp(counts[e], 0, limit)``:

    * ``mode="rows"``, limit ``M``: rows ``m >= n_e`` of ``out[e]`` are zeros whatever ``a[e]`` holds
      there, and tiles wholly past ``n_e`` do no work;
    * ``mode="reduce"``, limit ``K``: the sum runs over ``k < roundup(n_e, GEMM_BK)`` only. Columns
      past that are never read; those in ``[n_e, roundup(n_e, GEMM_BK))`` are, and the caller keeps
      them zero (the dispatch and the combine's backward write zero rows there).

    Every element of ``out`` is written; no atomics; bitwise repeatable; capturable. The slabs of
    ``out`` must not overlap (batch stride at least ``M`` rows); those of ``a`` and ``b`` may.
    ``tile`` is a measurement knob for the tile-shape A/B and the tests, not a tuning option: -1
    (the default) takes 256 x 128 tiles with 3 stages where ``M % 256 == 0`` and 128 x 128 with 2
    stages otherwise; 0 / 1 force the one or the other (1 needs ``M % 256 == 0``). Same bits either way."""
    num, m, n, k = _check_gemm(a, b, counts, mode, out)
    if tile not in (-1, 0, 1) or (tile == 1 and m % 256):
        raise ValueError(f"tile must be -1, 0 or 1 (1 with M % 256 == 0 only), got {tile!r} with M {m}")
    _on_gpu((a, "a"), (b, "b"), (counts, "counts"), (out, "out"))
    _aligned((a, "a"), (b, "b"), (out, "out"))
    if out is None:
        out = torch.empty((num, m, n), dtype=torch.bfloat16, device=a.device)
    rc = _lib.lib().kgs_moe_gemm_bf16_nt(a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                         0 if counts is None else counts.data_ptr(), num, m, n, k, a.stride(1),
                                         b.stride(1), out.stride(1), a.stride(0), b.stride(0), out.stride(0),
                                         MODES[mode], tile, _lib.stream_handle(a.device))
    _lib.check(rc, f"moe_gemm[{num}x{m}x{n}x{k}, mode={mode}]")
    return out


def ref_moe_gemm(a, b, counts=None, mode=None, dtype=torch.float64):
    """:func:`moe_gemm` in ``dtype``, unrounded: ``[E, M, N]``. ``"reduce"`` sums over ``k < n_e``, which
    is the kernel's sum when the columns up to ``roundup(n_e, GEMM_BK)`` are zero. Differentiable."""
    if mode not in MODES or (counts is None) != (mode is None):
        raise ValueError("mode must be None, 'rows' or 'reduce', with counts exactly when it is not None")
    a, b = a.to(dtype), b.to(dtype)
    if mode == "reduce":
        live = torch.arange(a.shape[2], device=a.device)[None, :] < counts.clamp(0, a.shape[2])[:, None]  # [E, K]
        a = torch.where(live[:, None, :], a, torch.zeros_like(a))
        b = torch.where(live[:, None, :], b, torch.zeros_like(b))
    if mode == "rows":
        live = torch.arange(a.shape[1], device=a.device)[None, :] < counts.clamp(0, a.shape[1])[:, None]  # [E, M]
        a = torch.where(live[:, :, None], a, torch.zeros_like(a))
    return a @ b.transpose(1, 2)


def _stacked(weights) -> torch.Tensor:
    """The E per-expert ``[N, K]`` weights as one ``[E, N, K]`` view; they must be consecutive
    slices of one allocation."""
    weights = list(weights)
    if not weights:
        raise ValueError("weights must hold at least one matrix")
    w0 = weights[0]
    for w in weights:
        _bf16_matrix(w, "weights", tuple(w0.shape))
    n, k = w0.shape
    for i, w in enumerate(weights):
        if not w.is_contiguous() or w.device != w0.device or \
                w.untyped_storage().data_ptr() != w0.untyped_storage().data_ptr() or \
                w.storage_offset() != w0.storage_offset() + i * n * k:
            raise ValueError("weights must be consecutive contiguous slices of one [E, N, K] allocation (a MoEFFN with "
                             "expert_gemm='batched' restacks its own on Module.to, not after load_state_dict(assign=True))")
    return w0.detach().as_strided((len(weights), n, k), (n * k, k, 1))


def _blocks(t: torch.Tensor, num: int) -> torch.Tensor:
    """``[R, num * c]`` -> the ``num`` column blocks as a ``[num, R, c]`` view."""
    c = t.shape[1] // num
    return t.as_strided((num, t.shape[0], c), (c, t.stride(0), 1))


def _slabs(t: torch.Tensor, num: int) -> torch.Tensor:
    """``[num * C, cols]`` -> the ``num`` row slabs as a ``[num, C, cols]`` view."""
    c = t.shape[0] // num
    return t.as_strided((num, c, t.shape[1]), (c * t.stride(0), t.stride(0), 1))


class _MoeLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xe, counts, *weights):
        w3 = _stacked(weights)
        ctx.save_for_backward(xe, counts, w3)
        return moe_gemm(_slabs(xe, w3.shape[0]), w3, counts, "rows").view(-1, w3.shape[1])

    @staticmethod
    def backward(ctx, dy):
        from .gemm import transpose

        xe, counts, w3 = ctx.saved_tensors
        num, n, k = w3.shape
        dy = _grad_rows(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:  # dx_e = dy_e W_e: B the column block e of the stacked weights' transpose
            wt = transpose(w3.view(num * n, k))  # [K, E N]
            dx = moe_gemm(_slabs(dy, num), _blocks(wt, num), counts, "rows").view(-1, k)
        if any(ctx.needs_input_grad[2:]):  # dW_e = dy_e^T x_e, summed over the filled rows only
            dw = moe_gemm(_blocks(transpose(dy), num), _blocks(transpose(xe), num), counts, "reduce")
        return (dx, None, *(dw.unbind(0) if dw is not None else (None,) * num))


def moe_linear(xe: torch.Tensor, weights, counts: torch.Tensor) -> torch.Tensor:
    """``ye[e C:(e + 1) C] = xe[e C:(e + 1) C] @ weights[e].T`` for the E slabs of ``xe [E C, K]`` in one
    :func:`moe_gemm` launch (``"rows"``: rows past ``counts[e]`` give zero rows); differentiable in
    ``xe`` and in the weights. The backward is two more launches and three 2-D transposes:
    ``dx`` (``"rows"``) against the transposed stack, ``dW`` (``"reduce"`` over the filled rows, which
    needs ``C % GEMM_BK == 0`` and the rows of ``xe`` and of the incoming gradient past
    ``counts[e]`` to be zero, as :func:`moe_dispatch` and :func:`moe_combine` leave them). ``weights``:
    the E ``[N, K]`` matrices, consecutive slices of one allocation (else ``ValueError``); their
    gradients are views of one ``[E, N, K]`` buffer. ``N``, ``K`` and ``C`` multiples of 128."""
    w3 = _stacked(weights)
    num, n, k = w3.shape
    _check_rows(xe, "xe", cols=k)
    if xe.shape[0] % num:
        raise ValueError(f"xe must be [E * C, {k}] with E = {num}, got {tuple(xe.shape)}")
    _check_gemm(_slabs(xe, num), w3, counts, "rows", None)
    if k % 128:
        raise ValueError(f"K must be a multiple of 128 (it is the N of dx), got {k}")
    _on_gpu((xe, "xe"), (w3, "weights"), (counts, "counts"))
    if not _wants_grad(xe, *weights):
        return moe_gemm(_slabs(xe, num), w3, counts, "rows").view(-1, n)
    return _MoeLinearFn.apply(xe, counts, *weights)


# ---------------------------------------------------------------------------
# the model: the same formulas in torch ops
def ref_moe_route(logits, top_k, capacity, dtype=torch.float64) -> Route:
    """:func:`moe_route` in torch ops: the indices exactly, ``weights`` in ``dtype``
    (differentiable in ``logits``)."""
    rows, num = logits.shape
    order = torch.sort(logits.detach().float(), dim=1, descending=True, stable=True).indices[:, :top_k]
    weights = torch.softmax(logits.to(dtype).gather(1, order), dim=1)
    flat = order.reshape(-1)
    by_e = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=num)
    start = torch.cumsum(counts, 0) - counts
    rank = torch.empty_like(flat)
    rank[by_e] = torch.arange(flat.numel(), device=flat.device) - start[flat[by_e]]
    slot = torch.where(rank < capacity, flat * capacity + rank, torch.full_like(flat, -1))
    src = torch.full((num * capacity,), -1, dtype=torch.int64, device=flat.device)
    kept = slot >= 0
    src[slot[kept]] = torch.arange(flat.numel(), device=flat.device)[kept]
    return Route(weights, order.int(), slot.reshape(rows, top_k).int(), src.int(), counts.int())


def ref_moe_gather(x, src, top_k, scale=None, dtype=None):
    """:func:`moe_gather`: rows ``x[src // top_k]`` (times ``scale`` by flat index), zero
    where ``src < 0``; in ``dtype``, or as a copy in ``x``'s own. Differentiable in ``x``."""
    f = src.long().clamp(min=0)
    rows = x[f // top_k] if dtype is None else x[f // top_k].to(dtype)
    if scale is not None:
        rows = rows * scale.reshape(-1)[f].to(rows.dtype)[:, None]
    return torch.where((src >= 0)[:, None], rows, torch.zeros_like(rows))


def ref_moe_combine(ye, slot, weights=None, dtype=torch.float64):
    """:func:`moe_combine` in ``dtype``, unrounded: ``[T, D]``. Differentiable."""
    picked = ye.to(dtype)[slot.long().clamp(min=0)]  # [T, k, D]
    w = (slot >= 0).to(dtype) if weights is None else torch.where(slot >= 0, weights.to(dtype), 0.0)
    return (torch.where((slot >= 0)[..., None], picked, torch.zeros_like(picked)) * w[..., None]).sum(1)


def ref_moe_dispatch_backward(dxe, slot, dtype=torch.float64):
    """``dx`` of :func:`moe_dispatch`: the unweighted combine of ``dxe``."""
    return ref_moe_combine(dxe, slot, None, dtype)


def ref_moe_combine_backward(dy, ye, slot, src, weights, dtype=torch.float64):
    """``(dye, dweights)`` of :func:`moe_combine_backward` in ``dtype``, unrounded."""
    dye = ref_moe_gather(dy, src, slot.shape[1], scale=weights, dtype=dtype)
    picked = ye.to(dtype)[slot.long().clamp(min=0)]
    dw = (picked * dy.to(dtype)[:, None, :]).sum(-1)
    return dye, torch.where(slot >= 0, dw, torch.zeros_like(dw))


def ref_moe_route_backward(dweights, weights, experts, num_experts, dtype=torch.float64):
    """``dlogits [T, E]`` of :func:`moe_route_backward` in ``dtype``, unrounded."""
    w, d = weights.to(dtype), dweights.to(dtype)
    g = w * (d - (w * d).sum(1, keepdim=True))
    return torch.zeros((w.shape[0], num_experts), dtype=dtype, device=w.device).scatter_(1, experts.long(), g)
