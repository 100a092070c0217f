"""The fused AdamW step on the gfx950 kernels (``native/kernels/optimizer.hip``) and
the float64 references the tests compare it with. :class:`kgs.optim.AdamW` is the
optimizer built on these.

* :func:`adamw_table` -- the tensor table of a model (weights, fp32 masters and
  moments, gradients, groups), checked and laid out on the host
* :func:`grad_norm` -- the global gradient norm, the clip factor, the skip
  decision, the step counter and the bias corrections, into the device state block
* :func:`adamw_step_` -- the update of every tensor of the table, in place
* :func:`grad_accumulate_` -- one micro-batch's bf16 gradients into fp32 main
  gradients (``native/kernels/grad_accum.hip``); ``grad_norm`` and ``adamw_step_``
  with ``main=True`` then step from those
* :func:`ref_adamw_step`, :func:`ref_grad_norm`, :func:`ref_clip`,
  :func:`ref_grad_accumulate` -- the same formulas stated directly, float64 unless
  asked otherwise

The step of all tensors is three launches (two without clipping) and no host
synchronisation: lr, the step counter and the clip factor are read from device
memory, so a captured step replays with new values. There is no PyTorch fallback:
a missing native library raises :class:`kgs.ops.NativeUnavailable`.
"""
from __future__ import annotations

import torch

from . import _lib

ROW_WORDS = 8    # int64 words of a table row: w, p, m, v, g, numel, group, chunk0
STATE_WORDS = 8  # 32-bit words of the state block
# word index in the state block (ints: step, skipped, skip; the rest fp32)
STATE_STEP, STATE_SKIPPED, STATE_GRAD_NORM, STATE_CLIP, STATE_BC1, STATE_BC2, STATE_SKIP = range(7)
# word 7 (int), main gradients only: > 0 that many micro-batches are accumulated and wait for a step, <= 0 the
# cycle is consumed (the last step left -n) and the next accumulate starts a fresh sum
STATE_MICRO = 7


def adamw_chunk() -> int:
    """Elements of one work chunk (one workgroup); chunks never span tensors."""
    return int(_lib.lib().kgs_adamw_chunk())


def _flat(t, name: str, dtype, numel: int | None = None) -> None:
    # dtype and shape before the device, so a wrong call fails the same way everywhere
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must have {numel} elements, got {t.numel()}")


def _on_gpu(named, dev=None):
    for t, name in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{name} must be on a GPU")
        if dev is not None and t.device != dev:
            raise ValueError(f"{name} must be on the device of the other operands")
        dev = t.device
    return dev


def adamw_table(weights, masters, exp_avgs, exp_avg_sqs, grads, group_index, ngroups: int, pin: bool = True,
                grad_dtype=torch.bfloat16):
    """The tensor table of :func:`grad_norm` / :func:`adamw_step_` as a host int64
    tensor ``[n, 8]`` (pinned unless ``pin`` is false), and its number of work chunks.
    ``grad_dtype=torch.float32`` builds the main table of :func:`grad_accumulate_` and
    of the ``main=True`` steps: ``grads`` are then the fp32 main gradients. Built from
    the same tensors, the two tables have the same ``numel``, ``group`` and ``chunk0``
    per row: row ``i`` and chunk ``c`` mean the same in both.

    Per tensor: a contiguous bf16 weight, contiguous fp32 master, first and second
    moment of the same number of elements, a contiguous bf16 gradient or ``None``
    (the tensor is skipped by the step) and the index of its parameter group. All on
    one GPU, every pointer 16-byte aligned; zero elements are legal. The checks
    here are the only ones: the kernels trust the table they are given."""
    if grad_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("grad_dtype must be torch.bfloat16 or torch.float32")
    n = len(weights)
    if not (len(masters) == len(exp_avgs) == len(exp_avg_sqs) == len(grads) == len(group_index) == n):
        raise ValueError("weights, masters, exp_avgs, exp_avg_sqs, grads and group_index need one entry per tensor")
    if n == 0:
        raise ValueError("the table needs at least one tensor")
    for i in range(n):
        _flat(weights[i], f"weights[{i}]", torch.bfloat16)
        ne = weights[i].numel()
        _flat(masters[i], f"masters[{i}]", torch.float32, ne)
        _flat(exp_avgs[i], f"exp_avgs[{i}]", torch.float32, ne)
        _flat(exp_avg_sqs[i], f"exp_avg_sqs[{i}]", torch.float32, ne)
        if grads[i] is not None:
            _flat(grads[i], f"grads[{i}]", grad_dtype, ne)
        if not 0 <= int(group_index[i]) < int(ngroups):
            raise ValueError(f"group_index[{i}] must be in [0, {int(ngroups)})")
    dev = None
    for i in range(n):
        dev = _on_gpu(((weights[i], f"weights[{i}]"), (masters[i], f"masters[{i}]"), (exp_avgs[i], f"exp_avgs[{i}]"),
                       (exp_avg_sqs[i], f"exp_avg_sqs[{i}]"), (grads[i], f"grads[{i}]")), dev)
    rows = []
    for i in range(n):
        ptrs = [t.data_ptr() if t is not None and t.numel() else 0
                for t in (weights[i], masters[i], exp_avgs[i], exp_avg_sqs[i], grads[i])]
        if any(p % 16 for p in ptrs):
            raise ValueError(f"tensor {i}: weight, master, moments and gradient must be 16-byte aligned")
        rows.append(ptrs + [weights[i].numel(), int(group_index[i]), 0])
    lib = _lib.lib()
    chunk, done = int(lib.kgs_adamw_chunk()), 0
    for r in rows:
        r[7] = done
        done += -(-r[5] // chunk)
    host = torch.tensor(rows, dtype=torch.int64)
    if pin:
        host = host.pin_memory()
    rc = int(lib.kgs_adamw_table_check(host.data_ptr(), n, int(ngroups)))
    if rc < 0:
        _lib.check(rc, "adamw_table")
    assert rc == done
    return host, done


def _device_blocks(table, nchunks, state, partials=None, groups=None):
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64:
        raise TypeError("table must be an int64 tensor (adamw_table's, copied to the GPU)")
    if table.dim() != 2 or table.shape[1] != ROW_WORDS or not table.is_contiguous() or table.shape[0] == 0:
        raise ValueError(f"table must be a contiguous [n, {ROW_WORDS}] tensor")
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32:
        raise TypeError("state must be an int32 tensor")
    if state.shape != (STATE_WORDS,) or not state.is_contiguous():
        raise ValueError(f"state must be a contiguous vector of {STATE_WORDS} words")
    if int(nchunks) < 0:
        raise ValueError("nchunks must not be negative")
    if partials is not None:
        _flat(partials, "partials", torch.float32)
        if partials.numel() < int(nchunks):
            raise ValueError(f"partials must hold one value per chunk ({int(nchunks)})")
    if groups is not None:
        _flat(groups, "groups", torch.float32)
        if groups.dim() != 2 or groups.shape[1] != 2 or groups.shape[0] == 0:
            raise ValueError("groups must be [ngroups, 2]: lr and weight_decay per group")
    _on_gpu(((table, "table"), (state, "state"), (partials, "partials"), (groups, "groups")))
    for t, name in ((table, "table"), (state, "state"), (partials, "partials"), (groups, "groups")):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")


def _betas(betas):
    b1, b2 = float(betas[0]), float(betas[1])
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError("betas must be in [0, 1)")
    return b1, b2


def grad_accum_tables_check(grad_host: torch.Tensor, main_host: torch.Tensor) -> None:
    """The host-side check of the pair of tables :func:`grad_accumulate_` takes (both
    from :func:`adamw_table`, before they are uploaded): row for row the same
    ``numel``, ``group`` and ``chunk0``, and a main gradient for every tensor that has
    elements. The kernel trusts the device copies."""
    for t, name in ((grad_host, "grad_host"), (main_host, "main_host")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError(f"{name} must be an int64 tensor (adamw_table's)")
        if t.is_cuda or t.dim() != 2 or t.shape[1] != ROW_WORDS or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous host [n, {ROW_WORDS}] tensor")
    if grad_host.shape != main_host.shape:
        raise ValueError("the two tables need the same number of rows")
    rc = int(_lib.lib().kgs_grad_accum_table_check(grad_host.data_ptr(), main_host.data_ptr(), grad_host.shape[0]))
    _lib.check(rc, "grad_accum_tables_check")


def grad_accumulate_(grad_table: torch.Tensor, main_table: torch.Tensor, nchunks: int, state: torch.Tensor,
                     zero_grads: bool = True) -> None:
    """One micro-batch into the fp32 main gradients of every tensor, in one launch
    over the two device tables, and a one-thread launch behind it that advances the
    micro-batch count (word 7 of ``state``). Per element ``main = float(g)`` when the
    count says that the cycle is consumed (<= 0: the first micro-batch), ``main = main +
    float(g)`` otherwise: one fp32 add. With ``zero_grads`` the bf16 gradient is left
    as zero bits in the same pass. A row without a bf16 gradient contributes nothing;
    on a first micro-batch its main gradient is written as zeros."""
    for t in (grad_table, main_table):  # both types before any device check
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError("grad_table and main_table must be int64 tensors (adamw_table's, copied to the GPU)")
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32:
        raise TypeError("state must be an int32 tensor")
    if grad_table.shape != main_table.shape:
        raise ValueError("the two tables need the same number of rows")
    _device_blocks(grad_table, nchunks, state)
    _device_blocks(main_table, nchunks, state)
    _on_gpu(((grad_table, "grad_table"), (main_table, "main_table")))
    rc = _lib.lib().kgs_grad_accumulate(grad_table.data_ptr(), main_table.data_ptr(), grad_table.shape[0],
                                        int(nchunks), state.data_ptr(), 1 if zero_grads else 0,
                                        _lib.stream_handle(grad_table.device))
    _lib.check(rc, "grad_accumulate_")


def grad_norm(table: torch.Tensor, nchunks: int, state: torch.Tensor, betas, partials: torch.Tensor | None = None,
              max_norm: float | None = None, variant: int | None = None, main: bool = False,
              average: bool = True) -> None:
    """The scalar half of a step, into the device ``state`` block (int32 ``[8]``).

    With ``max_norm``: one fp32 sum of squares of the bf16 gradients per chunk into
    ``partials`` (fp32, at least ``nchunks``), then one workgroup adds them in index
    order and writes ``grad_norm`` and ``clip = min(1, max_norm / (grad_norm + 1e-6))``
    (``torch.nn.utils.clip_grad_norm_``'s factor). A norm that is not finite sets the
    skip flag, counts the step in ``skipped`` and leaves ``step`` alone. Without
    ``max_norm`` there is no norm pass: ``clip = 1``, never skipped. A step that is
    not skipped increments ``step`` and gets ``bc1 = 1 - b1^step``, ``bc2 = 1 -
    b2^step``, evaluated in double. Two launches (one without clipping), no atomics:
    bitwise repeatable. ``variant``: odd reads the gradients with non-temporal loads
    (the measured default), even with plain ones.

    ``main=True``: ``table`` is the fp32 main table. The norm is that of ``s * main``
    with ``s = 1 / n`` for ``average`` (``n`` the micro-batch count of the state block)
    and 1 otherwise; the cycle is consumed whether the step is skipped or not, and a
    step with nothing accumulated counts as skipped. There are no variants."""
    _device_blocks(table, nchunks, state, partials=partials)
    b1, b2 = _betas(betas)
    if (max_norm is None) != (partials is None):
        raise ValueError("max_norm and partials come together")
    if max_norm is not None and not float(max_norm) > 0.0:
        raise ValueError("max_norm must be positive")
    if main and variant is not None:
        raise ValueError("the main-gradient norm pass has no variants")
    lib, st = _lib.lib(), _lib.stream_handle(table.device)
    if main:
        avg = 1 if average else 0
        if max_norm is None or int(nchunks) == 0:
            _lib.check(lib.kgs_main_finalize(0, 0, 1.0, b1, b2, avg, state.data_ptr(), st), "grad_norm")
            return
        _lib.check(lib.kgs_main_sumsq(table.data_ptr(), table.shape[0], int(nchunks), partials.data_ptr(), st),
                   "grad_norm")
        _lib.check(lib.kgs_main_finalize(partials.data_ptr(), int(nchunks), float(max_norm), b1, b2, avg,
                                         state.data_ptr(), st), "grad_norm")
        return
    if max_norm is None or int(nchunks) == 0:
        _lib.check(lib.kgs_adamw_finalize(0, 0, 1.0, b1, b2, state.data_ptr(), st), "grad_norm")
        return
    v = int(lib.kgs_adamw_sumsq_default_variant()) if variant is None else int(variant)
    _lib.check(lib.kgs_adamw_grad_sumsq_v(table.data_ptr(), table.shape[0], int(nchunks), partials.data_ptr(), v, st),
               "grad_norm")
    _lib.check(lib.kgs_adamw_finalize(partials.data_ptr(), int(nchunks), float(max_norm), b1, b2, state.data_ptr(),
                                      st), "grad_norm")


def adamw_step_(table: torch.Tensor, nchunks: int, groups: torch.Tensor, state: torch.Tensor, betas, eps: float,
                variant: int | None = None, main: bool = False, average: bool = True) -> None:
    """AdamW on every tensor of the table that has a gradient, in place, one launch.
    Per element, in fp32, with ``clip``, ``bc1``, ``bc2`` and the skip flag from
    ``state`` (:func:`grad_norm` ran before) and ``lr``, ``wd`` from the tensor's row
    of ``groups`` (fp32 ``[ngroups, 2]`` on the device)::

        g = clip * float(g_bf16)
        m = b1 m + (1 - b1) g;    v = b2 v + (1 - b2) g^2
        p = p (1 - lr wd) - lr (m / bc1) / (sqrt(v / bc2) + eps)

    ``p``, ``m`` and ``v`` are stored as fp32 and the bf16 weight is the stored ``p``
    rounded to nearest even, once. On a skipped step nothing is written.
    ``variant``: 0 plain accesses, 1 non-temporal, 2 / 3 the same with two 16-byte
    groups per thread and trip, 4 / 5 two groups with non-temporal loads / stores
    only; ``None`` is the measured default (2).

    ``main=True``: ``table`` is the fp32 main table and ``g = clip * s * main`` with
    the ``s`` of :func:`grad_norm` (which ran before with the same ``average``); the
    same arithmetic otherwise, two groups per trip and plain accesses, no variants."""
    _device_blocks(table, nchunks, state, groups=groups)
    b1, b2 = _betas(betas)
    if not float(eps) >= 0.0:
        raise ValueError("eps must not be negative")
    lib = _lib.lib()
    if main:
        if variant is not None:
            raise ValueError("the main-gradient step has no variants")
        rc = lib.kgs_adamw_step_main(table.data_ptr(), table.shape[0], int(nchunks), groups.data_ptr(),
                                     state.data_ptr(), b1, b2, float(eps), 1 if average else 0,
                                     _lib.stream_handle(table.device))
        _lib.check(rc, "adamw_step_")
        return
    v = int(lib.kgs_adamw_step_default_variant()) if variant is None else int(variant)
    rc = lib.kgs_adamw_step_v(table.data_ptr(), table.shape[0], int(nchunks), groups.data_ptr(), state.data_ptr(),
                              b1, b2, float(eps), v, _lib.stream_handle(table.device))
    _lib.check(rc, "adamw_step_")


# ----------------------------------------------------------------------------
# references: the formulas, stated directly

def ref_adamw_step(p, m, v, g, step, lr, betas, eps, weight_decay, clip=1.0, dtype=torch.float64, scale=1.0):
    """``(p, m, v)`` after AdamW step number ``step`` (1 for the first) in ``dtype``,
    unrounded: decoupled weight decay, bias-corrected moments, ``g`` scaled by ``clip``
    and by ``scale`` (a main-gradient step's ``1 / n``)."""
    b1, b2 = betas
    pf, mf, vf, gf = p.to(dtype), m.to(dtype), v.to(dtype), (clip * scale) * g.to(dtype)
    mf = b1 * mf + (1 - b1) * gf
    vf = b2 * vf + (1 - b2) * gf * gf
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return pf * (1 - lr * weight_decay) - lr * (mf / bc1) / ((vf / bc2).sqrt() + eps), mf, vf


def ref_grad_norm(grads, dtype=torch.float64, scale=1.0):
    """The 2-norm of all gradients, each times ``scale``, taken as one vector, in
    ``dtype``; ``None`` entries do not count."""
    total = torch.zeros((), dtype=dtype)
    for g in grads:
        if g is not None:
            total = total + (scale * g.to(dtype)).pow(2).sum().to(total.device)
    return total.sqrt()


def ref_grad_accumulate(main, grad, first: bool, dtype=torch.float64):
    """The main gradient after one micro-batch, in ``dtype``, unrounded: ``grad`` on
    the first micro-batch of a cycle (zeros for a ``None`` gradient), ``main + grad``
    afterwards (``main`` for a ``None`` gradient)."""
    if first:
        return torch.zeros_like(main, dtype=dtype) if grad is None else grad.to(dtype)
    return main.to(dtype) if grad is None else main.to(dtype) + grad.to(dtype)


def ref_clip(norm, max_norm):
    """``torch.nn.utils.clip_grad_norm_``'s factor: ``min(1, max_norm / (norm + 1e-6))``."""
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)
