"""Fused decoder-block ops on the gfx950 kernels (``native/kernels/transformer.hip``
and ``native/kernels/attention.hip``), plus the plain-PyTorch fp32 references the
tests compare them with.

* :func:`add_rmsnorm` -- ``x += d`` (bf16 residual stream, in place) then
  ``rmsnorm(x) * w``; :func:`rms_norm` without the add
* :func:`rope_qkv_` -- rotate-half RoPE on the q and k heads of a fused QKV
  projection output, in place
* :func:`silu_mul` -- SwiGLU ``silu(gate) * up`` from a fused gate|up output
* :func:`add_rmsnorm_fp8`, :func:`silu_mul_fp8`, :func:`quantize_rows_fp8` -- the
  same producers emitting e4m3 rows + per-row scales for
  :func:`kgs.ops.gemm.gemm_fp8_rows` (W8A8, per-token dynamic activation scales)
* :func:`attention_qkv` -- causal/full GQA flash attention (head_dim 128) reading
  q, k, v straight out of the fused QKV buffer and writing ``[tokens, H*128]``
* :func:`attention_qkv_lse`, :func:`attention_qkv_backward`, :func:`flash_attention_qkv`
  -- the same attention for training: the forward that keeps the log-sum-exp, the
  dQ / dK / dV kernels and the autograd op over them
  (``native/kernels/attention_train.hip``)
* :func:`rmsnorm_backward`, :func:`silu_mul_backward`, :func:`cross_entropy_rows`,
  :func:`cross_entropy_rows_backward` -- the backward kernels of the norm and of
  SwiGLU and the softmax cross-entropy over logit rows
  (``native/kernels/train_ops.hip``); :func:`rmsnorm_residual`, :func:`swiglu`,
  :func:`rope_qkv`, :func:`softmax_cross_entropy` -- the autograd ops over them
* :func:`paged_prefill_plan`, :func:`paged_prefill_attention` -- every prompt
  chunk of a chunked-prefill step in one launch, keys / values read in place
  from the bf16 KV pages (``native/kernels/attention_paged.hip``)
* :func:`sample_rows` -- temperature / top-k / top-p / seeded Gumbel-max sampling
  of every logits row in one launch (``native/kernels/sampling.hip``), with
  :func:`sample_rows_reference`, its float64 numpy statement
* :func:`penalize_rows`, :func:`token_counts_add`, :func:`logprob_rows` -- penalties
  from a device token-count table and logprobs of the sampled token and the top k
  (``native/kernels/logit_ops.hip``), with :func:`penalize_rows_reference` (float32,
  bit for bit) and :func:`logprob_rows_reference` (float64)

Every op raises :class:`kgs.ops.NativeUnavailable` when the native library is
missing -- there is no silent PyTorch fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _lib


def _need(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a GPU")
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be bf16")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be a row-major 2-D matrix")


def add_rmsnorm(x: torch.Tensor, d: torch.Tensor | None, w: torch.Tensor, eps: float = 1e-5,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """``x += d`` (when ``d`` is given; bf16, in place) and return ``rmsnorm(x) * w``.

    cols must be a multiple of 512 (up to 8192)."""
    _need(x, "x")
    rows, cols = x.shape
    if d is not None:
        _need(d, "d")
        if d.shape != x.shape or d.stride(0) != x.stride(0):
            raise ValueError("d must match x in shape and row stride")
    if w.shape != (cols,) or w.dtype != torch.bfloat16 or not w.is_contiguous():
        raise ValueError("w must be a contiguous bf16 vector of length cols")
    y = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device) if out is None else out
    _need(y, "out")
    rc = _lib.lib().kgs_add_rmsnorm_bf16(x.data_ptr(), 0 if d is None else d.data_ptr(),
                                         0 if d is None else x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, cols,
                                         x.stride(0), y.stride(0), float(eps), _lib.stream_handle(x.device))
    _lib.check(rc, "add_rmsnorm")
    return y


def splitk_add_rmsnorm(partials: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """``x += bf16(sum(partials))`` (in place) and return ``rmsnorm(x) * w``:
    the split-K reduce of a decode projection fused with the residual add and
    norm after it. ``partials``: contiguous fp32 ``[nslice, rows, cols]``
    (``kgs.ops.gemm.gemm_nt_w4x_partials``); cols a multiple of 2048 up to 8192.
    The delta is rounded to bf16 as the unfused reduce would round it."""
    _need(x, "x")
    rows, cols = x.shape
    if partials.dtype != torch.float32 or partials.dim() != 3 or tuple(partials.shape[1:]) != (rows, cols) or \
            not partials.is_contiguous():
        raise ValueError("partials must be a contiguous fp32 [nslice, rows, cols] tensor")
    if w.shape != (cols,) or w.dtype != torch.bfloat16 or not w.is_contiguous():
        raise ValueError("w must be a contiguous bf16 vector of length cols")
    y = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device) if out is None else out
    _need(y, "out")
    rc = _lib.lib().kgs_splitk_add_rmsnorm_bf16(partials.data_ptr(), partials.shape[0], x.data_ptr(), w.data_ptr(),
                                                y.data_ptr(), rows, cols, x.stride(0), y.stride(0), float(eps),
                                                _lib.stream_handle(x.device))
    _lib.check(rc, "splitk_add_rmsnorm")
    return y


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """``x.argmax(dim=-1)`` for bf16 GPU logits ``[rows, cols]`` (cols % 8 == 0):
    int64, the first index of each row's maximum (NaN counts as the maximum)."""
    _need(x, "x")
    rows, cols = x.shape
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    rc = _lib.lib().kgs_argmax_rows_bf16(x.data_ptr(), out.data_ptr(), rows, cols, x.stride(0),
                                         _lib.stream_handle(x.device))
    _lib.check(rc, "argmax_rows")
    return out


_SAMPLE_PARAMS = (("temperature", torch.float32), ("top_k", torch.int32), ("top_p", torch.float32),
                  ("seed", torch.int64), ("counter", torch.int64))


def sample_rows(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                seed: torch.Tensor, counter: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """One token per row of bf16 GPU logits ``[rows, cols]`` (cols % 8 == 0), int64,
    in one launch (``native/kernels/sampling.hip``). Per-row device vectors:
    ``temperature`` fp32 (``<= 0``: greedy, :func:`argmax_rows`' answer), ``top_k``
    int32 (on when ``0 < k < cols``; ties with the k-th largest logit are kept),
    ``top_p`` fp32 (on when ``0 < p < 1``, applied after top-k; equal logits are kept
    or dropped together), ``seed`` and ``counter`` int64 (the Philox4x32-10 key and
    counter of the row's Gumbel-max draw). A row's token depends on its own logits
    and its own five parameters only. :func:`sample_rows_reference` states the
    semantics in numpy."""
    # types first, then shapes, then devices: the first two are checked the same on any machine
    vecs = (temperature, top_k, top_p, seed, counter)
    named = list(zip(_SAMPLE_PARAMS, vecs)) + ([(("out", torch.int64), out)] if out is not None else [])
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.bfloat16:
        raise TypeError("logits must be a bf16 tensor")
    for (name, dtype), v in named:
        if not isinstance(v, torch.Tensor) or v.dtype != dtype:
            raise TypeError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be a row-major 2-D matrix")
    rows, cols = logits.shape
    for (name, _), v in named:
        if v.shape != (rows,) or not v.is_contiguous():
            raise ValueError(f"{name} must be a contiguous vector of length rows ({rows})")
    _need(logits, "logits")
    for (name, _), v in named:
        if v.device != logits.device:
            raise ValueError(f"{name} must be on the logits' device")
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    rc = _lib.lib().kgs_sample_rows_bf16(logits.data_ptr(), out.data_ptr(), *(v.data_ptr() for v in vecs), rows, cols,
                                         logits.stride(0), _lib.stream_handle(logits.device))
    _lib.check(rc, "sample_rows")
    return out


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in exact integer arithmetic:
    ``counter`` ``[..., 4]`` and ``key`` ``[..., 2]`` of 32-bit words (numpy,
    broadcast against each other) -> uint32 ``[..., 4]``."""
    import numpy as np

    c = [np.asarray(counter)[..., j].astype(np.uint64) for j in range(4)]
    k = [np.asarray(key)[..., j].astype(np.uint64) for j in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def sample_uniforms(seed, counter, cols: int):
    """The sampler's uniforms, float64 ``[rows, cols]`` (exact): element i of a row
    is ``((w >> 8) + 0.5) * 2**-24`` with w word ``i % 4`` of Philox4x32-10, key
    ``(seed lo, seed hi)``, counter ``(i // 4, counter lo, counter hi, 0)``."""
    import numpy as np

    sd = np.asarray(seed, dtype=np.int64).astype(np.uint64)[:, None]
    ct = np.asarray(counter, dtype=np.int64).astype(np.uint64)[:, None]
    lo = np.uint64(0xFFFFFFFF)
    blocks = np.arange((cols + 3) // 4, dtype=np.uint64)[None, :]
    ctr = np.stack(np.broadcast_arrays(blocks, ct & lo, ct >> np.uint64(32), np.uint64(0)), axis=-1)
    key = np.stack(np.broadcast_arrays(sd & lo, sd >> np.uint64(32)), axis=-1)[:, :1]
    w = philox4x32_10(ctr, key).reshape(len(sd), -1)[:, :cols]
    return ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


class SampleReference(NamedTuple):
    tokens: "np.ndarray"    # int64 [rows]
    kept: "np.ndarray"      # bool [rows, cols]: the set the draw is made over (greedy rows: the token alone)
    gap: "np.ndarray"       # float64 [rows]: best minus second-best perturbed score (inf: one candidate)
    p_margin: "np.ndarray"  # float64 [rows]: min |M(v) - top_p| over the survivors' distinct logits (inf: top-p off)


def sample_rows_reference(logits, temperature, top_k, top_p, seed, counter) -> SampleReference:
    """:func:`sample_rows` on the CPU in float64 (numpy): the semantics in code.

    * greedy rows (``temperature <= 0``), rows holding a NaN and rows without a
      finite maximum: the first index of the maximum, NaN counting as the maximum
    * top-k (``0 < k < cols``): keep logits ``>=`` the k-th largest
    * top-p (``0 < p < 1``), over the top-k survivors' softmax at temperature T:
      with M(v) the mass of the survivors strictly above v, keep a token iff
      M(its logit) < p
    * token: first argmax of ``x / T - log(-log(u))`` over the kept set
      (:func:`sample_uniforms`); ``-inf`` is never kept"""
    import numpy as np

    x = logits.detach().float().cpu().numpy().astype(np.float64) if isinstance(logits, torch.Tensor) \
        else np.asarray(logits, dtype=np.float64)

    def vec(v, dt):
        return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(dt)

    rows, cols = x.shape
    T, k, p = vec(temperature, np.float64), vec(top_k, np.int64), vec(top_p, np.float64)
    nan = np.isnan(x)
    amax = np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, x).argmax(1)).astype(np.int64)
    xmax = x[np.arange(rows), amax]
    greedy = ~(T > 0) | ~np.isfinite(xmax)
    Ts = np.where(greedy, 1.0, T)[:, None]
    xs = np.where(greedy[:, None], 0.0, x)  # greedy rows: placeholders, overwritten below
    srt = -np.sort(-xs, axis=1)
    kon = (k > 0) & (k < cols)
    thr_k = np.where(kon, srt[np.arange(rows), np.clip(k, 1, cols) - 1], -np.inf)
    surv = (xs >= thr_k[:, None]) & (xs > -np.inf)
    # top-p on the sorted row: exclusive cumulative mass at the first occurrence of each value
    ssurv = (srt >= thr_k[:, None]) & (srt > -np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(ssurv, np.exp((srt - srt[:, :1]) / Ts), 0.0)
    prob = w / w.sum(1, keepdims=True)
    excl = np.cumsum(prob, axis=1) - prob
    idx = np.broadcast_to(np.arange(cols), srt.shape)
    first = np.maximum.accumulate(np.where(np.concatenate([np.ones((rows, 1), bool), srt[:, 1:] != srt[:, :-1]], 1),
                                           idx, 0), axis=1)
    above = np.take_along_axis(excl, first, axis=1)  # M(v) of every sorted entry
    pon = (p > 0) & (p < 1)
    keep_s = ssurv & (~pon[:, None] | (above < p[:, None]))
    thr_p = np.where(keep_s, srt, np.inf).min(1)
    kept = surv & (xs >= thr_p[:, None])
    p_margin = np.where(pon, np.where(ssurv, np.abs(above - p[:, None]), np.inf).min(1), np.inf)
    u = sample_uniforms(vec(seed, np.int64), vec(counter, np.int64), cols)
    score = np.where(kept, xs / Ts - np.log(-np.log(u)), -np.inf)
    tokens = score.argmax(1).astype(np.int64)
    if cols > 1:
        top2 = -np.partition(-score, 1, axis=1)[:, :2]
        with np.errstate(invalid="ignore"):
            gap = top2[:, 0] - top2[:, 1]
    else:
        gap = np.full(rows, np.inf)
    tokens = np.where(greedy, amax, tokens)
    onehot = np.arange(cols)[None, :] == amax[:, None]
    kept = np.where(greedy[:, None], onehot, kept)
    gap = np.where(greedy, np.inf, gap)
    p_margin = np.where(greedy, np.inf, p_margin)
    return SampleReference(tokens, kept, gap, p_margin)


LOGPROB_KMAX = 32            # logprob_rows: the most top entries a row can ask for
COUNT_PROMPT = 1 << 30       # count word: the token occurs in the request's prompt
COUNT_MASK = COUNT_PROMPT - 1  # count word: the token's count in the request's output


def _typed(named) -> None:
    for name, dtype, v in named:
        if not isinstance(v, torch.Tensor) or v.dtype != dtype:
            raise TypeError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor")


def _row_vectors(named, rows: int) -> None:
    for name, _, v in named:
        if v.shape != (rows,) or not v.is_contiguous():
            raise ValueError(f"{name} must be a contiguous vector of length rows ({rows})")


def _same_device(named, ref: torch.Tensor, what: str) -> None:
    for name, _, v in named:
        if v.device != ref.device:
            raise ValueError(f"{name} must be on the {what}' device")


def penalize_rows(logits: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor, rep: torch.Tensor,
                  slot: torch.Tensor, counts: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The penalised copy of bf16 GPU logits ``[rows, cols]`` (cols % 8 == 0) in one
    launch (``native/kernels/logit_ops.hip``): contiguous bf16 ``[rows, cols]``.
    Per-row device vectors ``freq``, ``pres``, ``rep`` (fp32) and ``slot`` (int32): row
    j reads the count words ``counts[slot[j]]`` of the int32 table ``[slots, cols]``
    (``w & COUNT_MASK``: the token's count n in the output, ``w & COUNT_PROMPT``: a
    prompt token). Rows with a slot outside ``[0, slots)`` and elements with ``w == 0``
    are copied bit for bit. Otherwise, in fp32 and each step rounded once:
    ``v -= freq * n + pres`` when ``n > 0``, then ``v = v / rep if v > 0 else v * rep``
    when ``rep != 1``, then bf16 nearest-even (a NaN comes out as 0x7fc0).
    :func:`penalize_rows_reference` is the same in numpy, bit for bit."""
    vecs = [("freq", torch.float32, freq), ("pres", torch.float32, pres), ("rep", torch.float32, rep),
            ("slot", torch.int32, slot)]
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.bfloat16:
        raise TypeError("logits must be a bf16 tensor")
    _typed(vecs + [("counts", torch.int32, counts)] + ([("out", torch.bfloat16, out)] if out is not None else []))
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be a row-major 2-D matrix")
    rows, cols = logits.shape
    _row_vectors(vecs, rows)
    if counts.dim() != 2 or counts.shape[1] != cols or not counts.is_contiguous():
        raise ValueError(f"counts must be a contiguous [slots, cols ({cols})] table")
    if out is not None and (tuple(out.shape) != (rows, cols) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous [rows ({rows}), cols ({cols})] matrix")
    _need(logits, "logits")
    _same_device(vecs + [("counts", None, counts)] + ([("out", None, out)] if out is not None else []), logits,
                 "logits")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.bfloat16, device=logits.device)
    rc = _lib.lib().kgs_penalize_rows_bf16(logits.data_ptr(), out.data_ptr(), freq.data_ptr(), pres.data_ptr(),
                                           rep.data_ptr(), slot.data_ptr(), counts.data_ptr(), rows, cols,
                                           logits.stride(0), counts.shape[0], _lib.stream_handle(logits.device))
    _lib.check(rc, "penalize_rows")
    return out


def token_counts_add(counts: torch.Tensor, tok: torch.Tensor, slot: torch.Tensor) -> torch.Tensor:
    """``counts[slot[j], tok[j]] += 1`` for every j with ``0 <= slot[j] < slots`` and
    ``0 <= tok[j] < cols``, in place and in one launch; other rows write nothing.
    ``counts``: int32 GPU table ``[slots, cols]``; ``tok``: int64 ``[rows]`` (the
    sampler's output); ``slot``: int32 ``[rows]``. The slots ``>= 0`` of one call must
    be distinct: the update is not atomic."""
    vecs = [("tok", torch.int64, tok), ("slot", torch.int32, slot)]
    _typed([("counts", torch.int32, counts)] + vecs)
    if counts.dim() != 2 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous [slots, cols] table")
    if tok.dim() != 1:
        raise ValueError("tok must be a vector")
    _row_vectors(vecs, tok.shape[0])
    if not counts.is_cuda:
        raise ValueError("counts must be on a GPU")
    _same_device(vecs, counts, "counts")
    rc = _lib.lib().kgs_token_counts_add(counts.data_ptr(), tok.data_ptr(), slot.data_ptr(), tok.shape[0],
                                         counts.shape[0], counts.shape[1], _lib.stream_handle(counts.device))
    _lib.check(rc, "token_counts_add")
    return counts


def logprob_rows(logits: torch.Tensor, tok: torch.Tensor, want: torch.Tensor, lp: torch.Tensor | None = None,
                 top_val: torch.Tensor | None = None, top_idx: torch.Tensor | None = None):
    """Logprobs of bf16 GPU logits ``[rows, cols]`` (cols % 8 == 0) in one launch:
    ``(lp, top_val, top_idx)``, fp32 ``[rows]``, fp32 ``[rows, 32]``, int32 ``[rows, 32]``.
    ``tok`` int64 ``[rows]``: the token whose logprob goes to ``lp`` (NaN outside
    ``[0, cols)``); ``want`` int32 ``[rows]``: ``< 0`` skips the row, else its
    ``k = min(want, cols, 32)`` most likely tokens, by logit descending then index
    ascending (-0 equals +0), go to ``top_idx[:k]`` with their logprobs in ``top_val[:k]``.
    Entries past k and skipped rows are left as they were (NaN / -1 in buffers made
    here). A logprob is ``(x_i - m) - log(sum_j exp(x_j - m))`` in fp32, m the row
    maximum; a row with a NaN or without a finite maximum gives NaN and indices
    ``0..k-1``. :func:`logprob_rows_reference` states the same in float64."""
    vecs = [("tok", torch.int64, tok), ("want", torch.int32, want)]
    outs = [(n, d, v) for n, d, v in (("lp", torch.float32, lp), ("top_val", torch.float32, top_val),
                                      ("top_idx", torch.int32, top_idx)) if v is not None]
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.bfloat16:
        raise TypeError("logits must be a bf16 tensor")
    _typed(vecs + outs)
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be a row-major 2-D matrix")
    rows, cols = logits.shape
    _row_vectors(vecs + outs[:1 if lp is not None else 0], rows)
    for name, _, v in outs:
        if name != "lp" and (tuple(v.shape) != (rows, LOGPROB_KMAX) or not v.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous [rows ({rows}), {LOGPROB_KMAX}] matrix")
    _need(logits, "logits")
    _same_device(vecs + outs, logits, "logits")
    dev = logits.device
    if lp is None:
        lp = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    if top_val is None:
        top_val = torch.full((rows, LOGPROB_KMAX), float("nan"), dtype=torch.float32, device=dev)
    if top_idx is None:
        top_idx = torch.full((rows, LOGPROB_KMAX), -1, dtype=torch.int32, device=dev)
    rc = _lib.lib().kgs_logprob_rows_bf16(logits.data_ptr(), tok.data_ptr(), want.data_ptr(), lp.data_ptr(),
                                          top_val.data_ptr(), top_idx.data_ptr(), rows, cols, logits.stride(0),
                                          _lib.stream_handle(dev))
    _lib.check(rc, "logprob_rows")
    return lp, top_val, top_idx


def _np(v, dt):
    import numpy as np

    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(dt)


def bf16_bits(x):
    """bf16 bit patterns (numpy uint16) of a bf16 tensor, of an array of bit patterns
    (uint16, taken as they are) or of floats (rounded to bf16, nearest-even; a NaN
    becomes 0x7fc0)."""
    import numpy as np

    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bfloat16:
            return x.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype == np.uint16:
        return x.copy()
    f = np.ascontiguousarray(x, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7FC0), r)


def bf16_bits_to_float(bits):
    """float32 values of bf16 bit patterns (numpy uint16)."""
    import numpy as np

    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def penalize_rows_reference(logits, freq, pres, rep, slot, counts):
    """:func:`penalize_rows` on the CPU in float32 numpy, one rounding per step:
    the bf16 bit patterns (uint16 ``[rows, cols]``) the kernel must produce.
    ``logits``: a bf16 tensor, uint16 bit patterns or floats (:func:`bf16_bits`)."""
    import numpy as np

    h = bf16_bits(logits)
    rows, cols = h.shape
    f, p, r = _np(freq, np.float32), _np(pres, np.float32), _np(rep, np.float32)
    sl, tab = _np(slot, np.int64), _np(counts, np.int64).reshape(-1, cols)
    out = h.copy()
    with np.errstate(all="ignore"):
        for j in range(rows):
            if not 0 <= sl[j] < len(tab):
                continue
            w = tab[sl[j]]
            n = w & COUNT_MASK
            v = bf16_bits_to_float(h[j])
            a = f[j] * n.astype(np.float32)
            t = a + p[j]
            v = np.where(n > 0, v - t, v).astype(np.float32)
            if r[j] != np.float32(1):
                v = np.where(v > 0, v / r[j], v * r[j]).astype(np.float32)
            out[j] = np.where(w != 0, bf16_bits(v), h[j])
    return out


def logprob_rows_reference(logits, tok, want):
    """:func:`logprob_rows` on the CPU in float64 numpy: ``(lp [rows], top_val
    [rows, 32], top_idx [rows, 32])`` (float64, float64, int64); skipped rows and
    entries past k hold NaN / -1."""
    import numpy as np

    x = bf16_bits_to_float(logits).astype(np.float64) if getattr(logits, "dtype", None) == np.uint16 else \
        (logits.detach().float().cpu().numpy().astype(np.float64) if isinstance(logits, torch.Tensor)
         else np.asarray(logits, dtype=np.float64))
    rows, cols = x.shape
    tk, wk = _np(tok, np.int64), _np(want, np.int64)
    lp = np.full(rows, np.nan)
    tv = np.full((rows, LOGPROB_KMAX), np.nan)
    ti = np.full((rows, LOGPROB_KMAX), -1, dtype=np.int64)
    for j in range(rows):
        if wk[j] < 0:
            continue
        k = int(min(wk[j], cols, LOGPROB_KMAX))
        m = np.nan if np.isnan(x[j]).any() else x[j].max()
        if not np.isfinite(m):
            ti[j, :k] = np.arange(k)
            continue
        with np.errstate(divide="ignore"):
            lps = (x[j] - m) - np.log(np.exp(x[j] - m).sum())
        if 0 <= tk[j] < cols:
            lp[j] = lps[tk[j]]
        order = np.lexsort((np.arange(cols), -x[j]))[:k]  # logit descending, then index ascending (-0 == +0)
        ti[j, :k], tv[j, :k] = order, lps[order]
    return lp, tv, ti


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return add_rmsnorm(x, None, w, eps)


def _fp8_out(rows, cols, device):
    from .gemm import FP8_DTYPE

    return (torch.empty((rows, cols), dtype=FP8_DTYPE, device=device),
            torch.empty(rows, dtype=torch.float32, device=device))


def add_rmsnorm_fp8(x: torch.Tensor, d: torch.Tensor | None, w: torch.Tensor, eps: float = 1e-5):
    """As :func:`add_rmsnorm`, but the normalised rows come back as e4m3 with a
    per-row scale: returns ``(y8, scales)``, ``y ~= y8.float() * scales[:, None]``."""
    _need(x, "x")
    rows, cols = x.shape
    if d is not None:
        _need(d, "d")
        if d.shape != x.shape or d.stride(0) != x.stride(0):
            raise ValueError("d must match x in shape and row stride")
    if w.shape != (cols,) or w.dtype != torch.bfloat16 or not w.is_contiguous():
        raise ValueError("w must be a contiguous bf16 vector of length cols")
    y8, ys = _fp8_out(rows, cols, x.device)
    rc = _lib.lib().kgs_add_rmsnorm_fp8(x.data_ptr(), 0 if d is None else d.data_ptr(),
                                        0 if d is None else x.data_ptr(), w.data_ptr(), y8.data_ptr(), ys.data_ptr(),
                                        rows, cols, x.stride(0), y8.stride(0), float(eps),
                                        _lib.stream_handle(x.device))
    _lib.check(rc, "add_rmsnorm_fp8")
    return y8, ys


def quantize_rows_fp8(x: torch.Tensor):
    """bf16 rows -> ``(e4m3 rows, per-row f32 scales)`` in one pass (cols % 512 == 0)."""
    _need(x, "x")
    rows, cols = x.shape
    y8, ys = _fp8_out(rows, cols, x.device)
    rc = _lib.lib().kgs_quant_rows_fp8(x.data_ptr(), y8.data_ptr(), ys.data_ptr(), rows, cols, x.stride(0),
                                       y8.stride(0), _lib.stream_handle(x.device))
    _lib.check(rc, "quantize_rows_fp8")
    return y8, ys


def silu_mul_fp8(gu: torch.Tensor):
    """SwiGLU into e4m3 rows with per-row scales: ``(a8, scales)``."""
    _need(gu, "gu")
    rows, w2 = gu.shape
    inter = w2 // 2
    y8, ys = _fp8_out(rows, inter, gu.device)
    rc = _lib.lib().kgs_silu_mul_fp8(gu.data_ptr(), y8.data_ptr(), ys.data_ptr(), rows, inter, gu.stride(0),
                                     y8.stride(0), _lib.stream_handle(gu.device))
    _lib.check(rc, "silu_mul_fp8")
    return y8, ys


def rope_tables(seq: int, head_dim: int, theta: float, device) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``cos``/``sin`` of ``pos * theta**(-2i/head_dim)``, shape [seq, head_dim/2]."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device=device, dtype=torch.float32) / head_dim))
    ang = torch.arange(seq, device=device, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rope_qkv_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int, head_dim: int, seq: int,
              positions: torch.Tensor | None = None) -> torch.Tensor:
    """Rotate (in place) the first ``heads`` heads of every token row of ``qkv``
    (q heads then k heads). Positions are ``token % seq`` unless given: then the
    tables must hold ``seq`` rows; given, one int32 position per row of ``qkv``, on
    its device, each below the tables' row count. Bad arguments raise before the
    device is looked at, so nothing is launched with them."""
    if qkv.dim() != 2:
        raise ValueError("qkv must be a row-major 2-D matrix")
    for t in (cos, sin):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != head_dim // 2:
            raise ValueError("cos/sin must be contiguous fp32 [max_pos, head_dim/2]")
    pos = 0
    if positions is not None:
        if positions.dtype != torch.int32 or not positions.is_contiguous():
            raise ValueError("positions must be contiguous int32")
        if positions.dim() != 1 or positions.numel() != qkv.shape[0]:
            raise ValueError("positions must be a 1-D tensor with one entry per row of qkv")
        if positions.device != qkv.device:
            raise ValueError("positions must be on qkv's device")
    elif cos.shape[0] < seq or sin.shape[0] < seq:  # the kernel reads table row token % seq
        raise ValueError("cos/sin must hold at least seq rows when no positions are given")
    _need(qkv, "qkv")
    if positions is not None:
        pos = positions.data_ptr()
    rc = _lib.lib().kgs_rope_qkv_bf16(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos, qkv.shape[0], heads,
                                      head_dim, qkv.stride(0), seq, _lib.stream_handle(qkv.device))
    _lib.check(rc, "rope_qkv")
    return qkv


def silu_mul(gu: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``silu(gu[:, :I]) * gu[:, I:]`` for a fused gate|up output of width 2I."""
    _need(gu, "gu")
    rows, w2 = gu.shape
    inter = w2 // 2
    out = torch.empty((rows, inter), dtype=torch.bfloat16, device=gu.device) if out is None else out
    _need(out, "out")
    rc = _lib.lib().kgs_silu_mul_bf16(gu.data_ptr(), out.data_ptr(), rows, inter, gu.stride(0), out.stride(0),
                                      _lib.stream_handle(gu.device))
    _lib.check(rc, "silu_mul")
    return out


def attention_qkv(qkv: torch.Tensor, batch: int, seq: int, heads: int, kv_heads: int, head_dim: int = 128,
                  causal: bool = True, scale: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Flash attention over a fused QKV buffer ``[batch*seq, (heads + 2*kv_heads) * head_dim]``
    (q heads, then k heads, then v heads per token). Returns ``[batch*seq, heads*head_dim]``."""
    _need(qkv, "qkv")
    if qkv.shape[0] != batch * seq or qkv.shape[1] < (heads + 2 * kv_heads) * head_dim:
        raise ValueError("qkv shape does not match batch/seq/heads")
    out = torch.empty((batch * seq, heads * head_dim), dtype=torch.bfloat16, device=qkv.device) \
        if out is None else out
    _need(out, "out")
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    ld = qkv.stride(0)
    esz = qkv.element_size()
    base = qkv.data_ptr()
    rc = _lib.lib().kgs_attn_fwd_bf16(base, base + heads * head_dim * esz, base + (heads + kv_heads) * head_dim * esz,
                                      out.data_ptr(), batch, seq, heads, kv_heads, head_dim, ld, ld, ld, out.stride(0),
                                      float(scale), 1 if causal else 0, _lib.stream_handle(qkv.device))
    _lib.check(rc, "attention")
    return out


def _bf16_rows(t: torch.Tensor, name: str, rows: int, cols: int) -> None:
    # dtype and shape before the device, so a wrong call fails the same way everywhere
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be bf16")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be a row-major 2-D matrix")
    if t.shape[0] < rows or t.shape[1] < cols:
        raise ValueError(f"{name} shape does not match batch/seq/heads")


def _attn_check(qkv, batch, seq, heads, kv_heads, head_dim):
    if head_dim != 128:
        raise ValueError("the training attention kernels take head_dim 128")
    if heads <= 0 or kv_heads <= 0 or heads % kv_heads:
        raise ValueError("heads must be a positive multiple of kv_heads")
    if batch <= 0 or seq <= 0 or seq % 128:
        raise ValueError("seq must be a positive multiple of 128")
    _bf16_rows(qkv, "qkv", batch * seq, (heads + 2 * kv_heads) * head_dim)
    if qkv.shape[0] != batch * seq:
        raise ValueError("qkv shape does not match batch/seq/heads")
    _need(qkv, "qkv")


def attention_qkv_lse(qkv: torch.Tensor, batch: int, seq: int, heads: int, kv_heads: int, causal: bool = True,
                      scale: float | None = None, head_dim: int = 128) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`attention_qkv` (the same output bits) that also returns each query
    row's log-sum-exp of the scaled, masked scores: ``lse`` fp32 ``[batch*heads,
    seq]``, natural log -- what :func:`attention_qkv_backward` recomputes P from."""
    _attn_check(qkv, batch, seq, heads, kv_heads, head_dim)
    out = torch.empty((batch * seq, heads * head_dim), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((batch * heads, seq), dtype=torch.float32, device=qkv.device)
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    ld, esz, base = qkv.stride(0), qkv.element_size(), qkv.data_ptr()
    rc = _lib.lib().kgs_attn_fwd_lse_bf16(base, base + heads * head_dim * esz,
                                          base + (heads + kv_heads) * head_dim * esz, out.data_ptr(), lse.data_ptr(),
                                          batch, seq, heads, kv_heads, head_dim, ld, ld, ld, out.stride(0),
                                          float(scale), 1 if causal else 0, _lib.stream_handle(qkv.device))
    _lib.check(rc, "attention_qkv_lse")
    return out, lse


def attention_qkv_backward(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, batch: int,
                           seq: int, heads: int, kv_heads: int, causal: bool = True, scale: float | None = None,
                           dqkv: torch.Tensor | None = None, head_dim: int = 128, _stages: int = 7) -> torch.Tensor:
    """Gradients of :func:`attention_qkv_lse` with respect to ``qkv`` from the
    output's gradient ``dout`` (bf16 ``[batch*seq, >= heads*128]``, any row
    stride), in the fused layout: ``dqkv`` bf16 ``[batch*seq, >= (heads +
    2*kv_heads)*128]`` holds dq, dk and dv as its three column groups (only those
    columns are written), so the QKV projection's backward consumes it with no
    ``cat``. Three launches (delta, dK/dV, dQ), no atomics: bitwise reproducible."""
    t, qc, w = batch * seq, heads * head_dim, (heads + 2 * kv_heads) * head_dim
    for x, n in ((out, "out"), (dout, "dout")):
        _bf16_rows(x, n, t, qc)
        if x.shape[0] != t:
            raise ValueError(f"{n} shape does not match batch/seq/heads")
    if lse.dtype != torch.float32:
        raise TypeError("lse must be fp32")
    if lse.shape != (batch * heads, seq) or not lse.is_contiguous():
        raise ValueError("lse must be contiguous [batch*heads, seq]")
    if dqkv is not None:
        _bf16_rows(dqkv, "dqkv", t, w)
    _attn_check(qkv, batch, seq, heads, kv_heads, head_dim)
    for x, n in ((out, "out"), (dout, "dout"), (lse, "lse")) + (((dqkv, "dqkv"),) if dqkv is not None else ()):
        if not x.is_cuda:
            raise ValueError(f"{n} must be on a GPU")
    if dqkv is None:
        dqkv = torch.empty((t, w), dtype=torch.bfloat16, device=qkv.device)
    ws = torch.empty((batch * heads, seq), dtype=torch.float32, device=qkv.device)
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    ld, esz, base = qkv.stride(0), qkv.element_size(), qkv.data_ptr()
    dld, dbase = dqkv.stride(0), dqkv.data_ptr()
    ko, vo = heads * head_dim * esz, (heads + kv_heads) * head_dim * esz
    rc = _lib.lib().kgs_attn_bwd_bf16_ex(base, base + ko, base + vo, out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                         dbase, dbase + ko, dbase + vo, ws.data_ptr(), batch, seq, heads, kv_heads,
                                         head_dim, ld, ld, ld, out.stride(0), dout.stride(0), dld, dld, dld,
                                         float(scale), 1 if causal else 0, int(_stages),
                                         _lib.stream_handle(qkv.device))
    _lib.check(rc, "attention_qkv_backward")
    return dqkv


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, batch, seq, heads, kv_heads, causal, scale):
        if not ctx.needs_input_grad[0]:
            return attention_qkv(qkv, batch, seq, heads, kv_heads, causal=causal, scale=scale)  # inference: unchanged
        out, lse = attention_qkv_lse(qkv, batch, seq, heads, kv_heads, causal=causal, scale=scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (batch, seq, heads, kv_heads, causal, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        batch, seq, heads, kv_heads, causal, scale = ctx.cfg
        if dout.stride(1) != 1:
            dout = dout.contiguous()
        dqkv = attention_qkv_backward(qkv, out, dout, lse, batch, seq, heads, kv_heads, causal=causal, scale=scale)
        if qkv.shape[1] != dqkv.shape[1]:  # a qkv wider than its three groups: the rest has no gradient
            full = torch.zeros_like(qkv)
            full[:, :dqkv.shape[1]] = dqkv
            dqkv = full
        return dqkv, None, None, None, None, None, None


def flash_attention_qkv(qkv: torch.Tensor, batch: int, seq: int, heads: int, kv_heads: int, causal: bool = True,
                        scale: float | None = None) -> torch.Tensor:
    """Differentiable :func:`attention_qkv` (head_dim 128, ``seq % 128 == 0``):
    forward and backward on the HIP kernels. When ``qkv`` needs no gradient this
    IS :func:`attention_qkv` (nothing saved)."""
    _attn_check(qkv, batch, seq, heads, kv_heads, 128)
    return _FlashAttnFn.apply(qkv, batch, seq, heads, kv_heads, causal, scale)


# ----------------------------------------------------------------------------
# training glue (native/kernels/train_ops.hip): raw backward ops, then the autograd ops

def _bf16_matrix(t: torch.Tensor, name: str, shape: tuple | None = None) -> None:
    # dtype and shape before the device, so a wrong call fails the same way everywhere
    if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be a bf16 tensor")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be a row-major 2-D matrix")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")


def _on_gpu(*named) -> None:
    dev = None
    for t, name in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{name} must be on a GPU")
        if dev is not None and t.device != dev:
            raise ValueError(f"{name} must be on the device of the other operands")
        dev = t.device


def rmsnorm_backward(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, dres: torch.Tensor | None = None,
                     eps: float = 1e-5) -> tuple[torch.Tensor, torch.Tensor]:
    """Gradients of ``y = rmsnorm(x) * w`` (the norm half of :func:`add_rmsnorm`):
    ``(dx, dw)``, bf16 ``[rows, cols]`` and ``[cols]``. ``x`` is the stream value the
    forward normalised (``x + d`` as it wrote it back), ``dy`` the gradient of ``y``
    and ``dres``, when given, the gradient that reaches the same stream value
    through the residual branch: it is added in fp32, before dx's one rounding.
    Per row ``r = rsqrt(mean(x^2) + eps)`` is recomputed, ``g = dy * w``, ``c =
    sum(g * x) / cols``, ``dx = dres + r g - x r^3 c``; ``dw = sum_rows dy x r``.
    Any row strides (multiples of 8); cols a multiple of 512 up to 8192. Two
    launches, no atomics: bitwise reproducible."""
    _bf16_matrix(x, "x")
    rows, cols = x.shape
    if cols % 512 or not 0 < cols <= 8192:
        raise ValueError("cols must be a multiple of 512 up to 8192")
    if not isinstance(w, torch.Tensor) or w.dtype != torch.bfloat16:
        raise TypeError("w must be a bf16 tensor")
    if w.shape != (cols,) or not w.is_contiguous():
        raise ValueError("w must be a contiguous bf16 vector of length cols")
    _bf16_matrix(dy, "dy", (rows, cols))
    if dres is not None:
        _bf16_matrix(dres, "dres", (rows, cols))
    _on_gpu((x, "x"), (w, "w"), (dy, "dy"), (dres, "dres"))
    dx = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    dw = torch.empty(cols, dtype=torch.bfloat16, device=x.device)
    lib = _lib.lib()
    ws = torch.empty(lib.kgs_rmsnorm_bwd_workspace(rows, cols) // 4, dtype=torch.float32, device=x.device)
    rc = lib.kgs_rmsnorm_bwd_bf16(x.data_ptr(), w.data_ptr(), dy.data_ptr(), 0 if dres is None else dres.data_ptr(),
                                  dx.data_ptr(), dw.data_ptr(), ws.data_ptr(), rows, cols, x.stride(0), dy.stride(0),
                                  0 if dres is None else dres.stride(0), dx.stride(0), float(eps),
                                  _lib.stream_handle(x.device))
    _lib.check(rc, "rmsnorm_backward")
    return dx, dw


def silu_mul_backward(gu: torch.Tensor, dh: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Gradient of :func:`silu_mul` with respect to the fused gate|up input:
    ``dgu`` bf16 ``[rows, 2I]`` (dgate | dup, the layout the gate/up projection's
    backward consumes with no ``cat``) from ``gu`` ``[rows, 2I]`` and ``dh`` ``[rows, I]``.
    With ``s = sigmoid(g)``: ``dgate = dh u s (1 + g (1 - s))``, ``dup = dh g s``.
    Any row strides (multiples of 8); ``I % 8 == 0``."""
    _bf16_matrix(gu, "gu")
    rows, w2 = gu.shape
    if w2 % 16 or w2 == 0:
        raise ValueError("gu must be [rows, 2I] with I a positive multiple of 8")
    inter = w2 // 2
    _bf16_matrix(dh, "dh", (rows, inter))
    if out is not None:
        _bf16_matrix(out, "out", (rows, w2))
    _on_gpu((gu, "gu"), (dh, "dh"), (out, "out"))
    if out is None:
        out = torch.empty((rows, w2), dtype=torch.bfloat16, device=gu.device)
    rc = _lib.lib().kgs_silu_mul_bwd_bf16(gu.data_ptr(), dh.data_ptr(), out.data_ptr(), rows, inter, gu.stride(0),
                                          dh.stride(0), out.stride(0), _lib.stream_handle(gu.device))
    _lib.check(rc, "silu_mul_backward")
    return out


def _xent_check(logits, target):
    _bf16_matrix(logits, "logits")
    rows, cols = logits.shape
    if cols % 8 or cols == 0:
        raise ValueError("logits must have a positive multiple of 8 columns")
    _typed([("target", torch.int64, target)])
    _row_vectors([("target", None, target)], rows)
    return rows, cols


def cross_entropy_rows(logits: torch.Tensor, target: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Softmax cross-entropy of every row of bf16 GPU logits ``[rows, cols]`` (cols % 8
    == 0, any row stride) in one pass: ``(loss, lse)``, fp32 ``[rows]``. ``lse`` is the
    row's log-sum-exp (natural log) and ``loss = lse - logits[row, target[row]]``. A
    target outside ``[0, cols)`` (``ignore_index = -100``) makes the row ignored:
    its loss is 0, its lse is still written."""
    rows, cols = _xent_check(logits, target)
    _on_gpu((logits, "logits"), (target, "target"))
    loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    rc = _lib.lib().kgs_xent_fwd_bf16(logits.data_ptr(), target.data_ptr(), loss.data_ptr(), lse.data_ptr(), rows,
                                      cols, logits.stride(0), _lib.stream_handle(logits.device))
    _lib.check(rc, "cross_entropy_rows")
    return loss, lse


def cross_entropy_rows_backward(logits: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, grow: torch.Tensor,
                                out: torch.Tensor | None = None) -> torch.Tensor:
    """Gradient of :func:`cross_entropy_rows`' loss with respect to the logits:
    ``dlogits[row, j] = bf16(grow[row] * (exp(logits[row, j] - lse[row]) - [j ==
    target[row]]))``, ``grow`` the fp32 gradient of each row's loss. At the target
    column ``p - 1`` is evaluated as minus the sum of the other columns' ``p``, which
    does not cancel when ``p`` is 1 in fp32. An ignored row is written as zeros.
    ``out``: a bf16 ``[rows, cols]`` buffer of its own (any row stride); only its
    columns ``< cols`` are written."""
    rows, cols = _xent_check(logits, target)
    vecs = [("lse", torch.float32, lse), ("grow", torch.float32, grow)]
    _typed(vecs)
    _row_vectors(vecs, rows)
    if out is not None:
        _bf16_matrix(out, "out", (rows, cols))
    _on_gpu((logits, "logits"), (target, "target"), (lse, "lse"), (grow, "grow"), (out, "out"))
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.bfloat16, device=logits.device)
    rc = _lib.lib().kgs_xent_bwd_bf16(logits.data_ptr(), target.data_ptr(), lse.data_ptr(), grow.data_ptr(),
                                      out.data_ptr(), rows, cols, logits.stride(0), out.stride(0),
                                      _lib.stream_handle(logits.device))
    _lib.check(rc, "cross_entropy_rows_backward")
    return out


def _add_rmsnorm_out_of_place(x, d, w, eps):
    """``(bf16(x + d), rmsnorm(x + d) * w)`` on kgs_add_rmsnorm_bf16 with its separate
    ``xo`` pointer: ``x`` is left alone."""
    rows, cols = x.shape
    res = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    y = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    if d.stride(0) != cols or x.stride(0) != cols:  # one row stride serves x, d and xo
        x, d = x.contiguous(), d.contiguous()
    rc = _lib.lib().kgs_add_rmsnorm_bf16(x.data_ptr(), d.data_ptr(), res.data_ptr(), w.data_ptr(), y.data_ptr(), rows,
                                         cols, cols, cols, float(eps), _lib.stream_handle(x.device))
    _lib.check(rc, "rmsnorm_residual")
    return res, y


def _grad_rows(g: torch.Tensor) -> torch.Tensor:
    """An incoming gradient as the kernels take it: unit column stride, a row stride
    that is a multiple of 8, 16-byte aligned (autograd may hand over expanded views)."""
    ok = g.dim() == 2 and g.stride(1) == 1 and g.stride(0) >= g.shape[1] and g.stride(0) % 8 == 0 and \
        g.data_ptr() % 16 == 0
    return g if ok else g.contiguous()


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


class _RmsNormResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, d, w, eps):
        if d is None:
            res, y = x, add_rmsnorm(x, None, w, eps)
        else:
            res, y = _add_rmsnorm_out_of_place(x, d, w, eps)
        ctx.save_for_backward(res, w)
        ctx.eps, ctx.has_d = eps, d is not None
        return res, y

    @staticmethod
    def backward(ctx, dres, dy):
        res, w = ctx.saved_tensors
        dy = torch.zeros_like(res) if dy is None else _grad_rows(dy)
        dx, dw = rmsnorm_backward(res, w, dy, None if dres is None else _grad_rows(dres), ctx.eps)
        return dx, (dx if ctx.has_d else None), dw, None


def rmsnorm_residual(x: torch.Tensor, d: torch.Tensor | None, w: torch.Tensor, eps: float = 1e-5
                     ) -> tuple[torch.Tensor, torch.Tensor]:
    """Differentiable, out-of-place :func:`add_rmsnorm`: ``(res, y)`` with ``res =
    bf16(x + d)`` (``x`` itself when ``d`` is None) and ``y = rmsnorm(res) * w``; ``x``
    and ``d`` are left alone. It saves ``res`` and ``w``; its backward takes ``(dres,
    dy)`` and makes ONE :func:`rmsnorm_backward` call, whose ``dx`` is the gradient
    of both ``x`` and ``d`` (the same tensor). With no gradient wanted it is the
    inference kernel alone, nothing saved."""
    _bf16_matrix(x, "x")
    rows, cols = x.shape
    if cols % 512 or not 0 < cols <= 8192:
        raise ValueError("cols must be a multiple of 512 up to 8192")
    if d is not None:
        _bf16_matrix(d, "d", (rows, cols))
    if not isinstance(w, torch.Tensor) or w.dtype != torch.bfloat16:
        raise TypeError("w must be a bf16 tensor")
    if w.shape != (cols,) or not w.is_contiguous():
        raise ValueError("w must be a contiguous bf16 vector of length cols")
    _on_gpu((x, "x"), (d, "d"), (w, "w"))
    if _wants_grad(x, d, w):
        return _RmsNormResidualFn.apply(x, d, w, eps)
    if d is None:
        return x, add_rmsnorm(x, None, w, eps)
    return _add_rmsnorm_out_of_place(x, d, w, eps)


class _SwiGluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return silu_mul(gu)

    @staticmethod
    def backward(ctx, dh):
        (gu,) = ctx.saved_tensors
        return silu_mul_backward(gu, _grad_rows(dh))


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    """Differentiable :func:`silu_mul`: ``silu(gu[:, :I]) * gu[:, I:]``; the backward is
    :func:`silu_mul_backward` on the saved ``gu``. With no gradient wanted this IS
    :func:`silu_mul` (nothing saved)."""
    _bf16_matrix(gu, "gu")
    if gu.shape[1] % 16 or gu.shape[1] == 0:
        raise ValueError("gu must be [rows, 2I] with I a positive multiple of 8")
    _on_gpu((gu, "gu"))
    return _SwiGluFn.apply(gu) if _wants_grad(gu) else silu_mul(gu)


class _RopeQkvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, heads, head_dim, seq):
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (heads, head_dim, seq)
        if qkv.is_leaf or qkv._base is not None:  # autograd forbids (a leaf) or restricts (a view) the in-place form
            return rope_qkv_(qkv.clone(memory_format=torch.contiguous_format), cos, sin, heads, head_dim, seq)
        ctx.mark_dirty(qkv)
        return rope_qkv_(qkv, cos, sin, heads, head_dim, seq)

    @staticmethod
    def backward(ctx, dout):
        cos, sin = ctx.saved_tensors
        heads, head_dim, seq = ctx.cfg
        # the transposed rotation is the rotation by -angle; on a private copy: autograd may share dout
        g = dout.clone(memory_format=torch.contiguous_format)
        return rope_qkv_(g, cos, -sin, heads, head_dim, seq), None, None, None, None, None


def rope_qkv(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int, head_dim: int, seq: int
             ) -> torch.Tensor:
    """Differentiable :func:`rope_qkv_` (positions ``token % seq`` only): returns the
    rotated rows. With no gradient wanted this IS :func:`rope_qkv_`, in place. When
    ``qkv`` needs a gradient the rotation is in place too where autograd allows it (a
    non-leaf that is not a view: ``qkv`` itself is returned, marked dirty), otherwise
    on a copy. The backward is the same kernel with the negated ``sin`` table -- the
    transposed rotation -- on a private copy of the incoming gradient, which is
    never touched; columns past the rotated heads pass through unchanged."""
    _bf16_matrix(qkv, "qkv")
    if head_dim <= 0 or head_dim % 16 or heads <= 0 or seq <= 0:
        raise ValueError("heads and seq must be positive and head_dim a positive multiple of 16")
    if qkv.shape[1] < heads * head_dim:
        raise ValueError("qkv rows must hold heads * head_dim rotated elements")
    for t, n in ((cos, "cos"), (sin, "sin")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{n} must be an fp32 tensor")
        if t.dim() != 2 or t.shape[0] < seq or t.shape[1] != head_dim // 2 or not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous fp32 [>= seq, head_dim/2]")
    _on_gpu((qkv, "qkv"), (cos, "cos"), (sin, "sin"))
    if not _wants_grad(qkv):
        return rope_qkv_(qkv, cos, sin, heads, head_dim, seq)
    return _RopeQkvFn.apply(qkv, cos, sin, heads, head_dim, seq)


class _SoftmaxXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, lse = cross_entropy_rows(logits, target)
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    def backward(ctx, grow):
        logits, target, lse = ctx.saved_tensors
        return cross_entropy_rows_backward(logits, target, lse, grow.float().contiguous()), None


def softmax_cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Differentiable :func:`cross_entropy_rows`: the fp32 per-row loss ``[rows]`` (0 for
    ignored rows; the caller takes the mean over the others in torch). It saves
    ``logits``, ``target`` and the rows' log-sum-exp; the backward is
    :func:`cross_entropy_rows_backward`. With no gradient wanted nothing is saved."""
    _xent_check(logits, target)
    _on_gpu((logits, "logits"), (target, "target"))
    if not _wants_grad(logits):
        return cross_entropy_rows(logits, target)[0]
    return _SoftmaxXentFn.apply(logits, target)


def attention_chunk(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, kv_heads: int,
                    head_dim: int = 128, scale: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Causal flash attention of one sequence's prefill CHUNK over its whole
    context: ``q`` rows ``[S, >= heads*128]`` are the last S positions (S % 128
    == 0), ``k``/``v`` ``[Sk, >= kv_heads*128]`` every key up to and including
    them (Sk - S % 64 == 0) -- row i sees keys 0 .. Sk - S + i. Any row strides."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _need(t, n)
    S, Sk = q.shape[0], k.shape[0]
    if v.shape[0] != Sk:
        raise ValueError("k and v differ in length")
    out = torch.empty((S, heads * head_dim), dtype=torch.bfloat16, device=q.device) if out is None else out
    _need(out, "out")
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    rc = _lib.lib().kgs_attn_fwd_bf16_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, S, Sk, heads,
                                         kv_heads, head_dim, q.stride(0), k.stride(0), v.stride(0), out.stride(0),
                                         float(scale), 1, _lib.stream_handle(q.device))
    _lib.check(rc, "attention_chunk")
    return out


class PagedPrefillPlan:
    """One step's prompt chunks as :func:`paged_prefill_attention` takes them
    (built by :func:`paged_prefill_plan`, shared by every layer of the step):
    ``chunks`` the host list of ``(row0, n, padded, ctx0)``, ``desc`` the same as
    int32 ``[nchunks, 4]`` on the device, ``qmap`` int32 ``[nqb, 2]`` mapping a
    q-block to ``(chunk, q-block in chunk)`` heaviest first, ``block_tables``
    int32 ``[nchunks, max_pages]``, ``rows`` one past the last Q row any chunk
    touches, ``max_page`` the largest page index in the tables (None when they
    were handed over on the device: reading them back would synchronise)."""

    __slots__ = ("chunks", "desc", "qmap", "block_tables", "rows", "max_page")

    def __init__(self, chunks, desc, qmap, block_tables, rows, max_page):
        self.chunks, self.desc, self.qmap, self.block_tables = chunks, desc, qmap, block_tables
        self.rows, self.max_page = rows, max_page


_PP_QB, _PP_KB, _PP_PAGE = 128, 64, 32  # attention_paged.hip: q-block rows, keys per tile, tokens per page


def paged_prefill_plan(chunks, block_tables, device) -> PagedPrefillPlan:
    """Validate one step's prompt chunks and build what the paged prefill
    kernel reads, once per step. ``chunks``: host ``(row0, n, padded, ctx0)`` per
    chunk -- Q rows ``row0 .. row0+padded-1`` hold positions ``ctx0 ..
    ctx0+padded-1``, ``n`` of them real; ``block_tables``: ``[nchunks, max_pages]``
    (an int tensor on any device, or nested lists), entries ``0 ..
    ceil((ctx0+n)/32)-1`` of a row the sequence's pages and every later entry a
    valid page index. Raises ``ValueError`` naming the offending chunk."""
    chunks = [tuple(int(v) for v in ch[:4]) for ch in chunks]
    if not chunks:
        raise ValueError("paged_prefill_plan: no chunks")
    bt = block_tables if isinstance(block_tables, torch.Tensor) else torch.as_tensor(block_tables, dtype=torch.int32)
    if bt.dim() != 2 or bt.shape[0] != len(chunks) or bt.shape[1] < 1:
        raise ValueError(f"block_tables must be [nchunks = {len(chunks)}, max_pages], got {tuple(bt.shape)}")
    width = bt.shape[1]
    work = []
    for ci, ch in enumerate(chunks):
        row0, n, padded, ctx0 = ch
        if row0 < 0 or padded <= 0 or padded % _PP_QB:
            raise ValueError(f"chunk {ci} {ch}: padded must be a positive multiple of {_PP_QB} (and row0 >= 0)")
        if ctx0 < 0 or ctx0 % _PP_KB:
            raise ValueError(f"chunk {ci} {ch}: ctx0 must be a non-negative multiple of {_PP_KB}")
        if not 1 <= n <= padded:
            raise ValueError(f"chunk {ci} {ch}: need 1 <= n <= padded")
        need = -(-(ctx0 + n) // _PP_PAGE)
        if width < need:
            raise ValueError(f"chunk {ci} {ch}: block table holds {width} pages, the chunk's context needs {need}")
        nreal = -(-(ctx0 + n) // _PP_KB)
        for qb in range(padded // _PP_QB):
            tiles = 0 if qb * _PP_QB >= n else min((ctx0 + (qb + 1) * _PP_QB) // _PP_KB, nreal)
            work.append((tiles, ci, qb))
    work.sort(key=lambda t: -t[0])  # heaviest first (stable: equal weights keep chunk order)
    max_page = None
    if bt.device.type == "cpu":
        if int(bt.min()) < 0:
            raise ValueError("block_tables holds a negative page index")
        max_page = int(bt.max())
    dev = torch.device(device)
    host = torch.tensor([v for ch in chunks for v in ch] + [v for _, ci, qb in work for v in (ci, qb)],
                        dtype=torch.int32)
    if dev.type == "cuda":
        host = host.pin_memory().to(dev, non_blocking=True)
    nd = 4 * len(chunks)
    bt = bt.to(device=dev, dtype=torch.int32).contiguous()
    return PagedPrefillPlan(chunks, host[:nd].view(len(chunks), 4), host[nd:].view(len(work), 2), bt,
                            max(ch[0] + ch[2] for ch in chunks), max_page)


def paged_prefill_attention(qkv: torch.Tensor, cache_layer: torch.Tensor, plan: PagedPrefillPlan, heads: int,
                            kv_heads: int, out: torch.Tensor | None = None, scale: float | None = None
                            ) -> torch.Tensor:
    """Causal flash attention of every prompt chunk of ``plan`` in ONE launch,
    keys and values read in place from ``cache_layer`` (one layer of a bf16
    :class:`kgs.ops.decode.PagedKVCache`, which already holds the chunks' own
    rows). ``qkv``: the fused, rotated QKV rows (the q heads are read). Row ``r <
    n`` of a chunk sees keys ``0 .. ctx0+r``; rows ``>= n`` come back as zeros;
    rows of ``out`` ``[rows, heads*128]`` outside every chunk are left alone.
    Call once per layer with the step's plan."""
    _need(qkv, "qkv")
    if cache_layer.dtype != torch.bfloat16:
        raise TypeError("paged_prefill_attention reads bf16 KV pages (an fp8 cache keeps the gather path)")
    if not cache_layer.is_cuda or cache_layer.dim() != 4 or not cache_layer.is_contiguous() or \
            tuple(cache_layer.shape[1:]) != (kv_heads, 2, _PP_PAGE * 128):
        raise ValueError("cache_layer must be a contiguous GPU [pages, kv_heads, 2, 4096] page array")
    if heads % kv_heads or qkv.shape[1] < heads * 128:
        raise ValueError("qkv rows must hold heads * 128 q elements, heads a multiple of kv_heads")
    if plan.rows > qkv.shape[0]:
        raise ValueError(f"the plan's chunks reach row {plan.rows}, qkv has {qkv.shape[0]}")
    if plan.max_page is not None and plan.max_page >= cache_layer.shape[0]:
        raise ValueError(f"block table entry {plan.max_page} outside the cache's {cache_layer.shape[0]} pages")
    if plan.desc.device != qkv.device:
        raise ValueError("the plan was built for another device")
    out = torch.empty((qkv.shape[0], heads * 128), dtype=torch.bfloat16, device=qkv.device) if out is None else out
    _need(out, "out")
    if out.shape[0] < plan.rows or out.shape[1] < heads * 128:
        raise ValueError("out must be [>= rows of the plan, >= heads*128]")
    scale = 1.0 / math.sqrt(128) if scale is None else scale
    rc = _lib.lib().kgs_attn_prefill_paged_bf16(qkv.data_ptr(), cache_layer.data_ptr(), plan.block_tables.data_ptr(),
                                                plan.desc.data_ptr(), plan.qmap.data_ptr(), out.data_ptr(),
                                                len(plan.chunks), plan.qmap.shape[0], heads, kv_heads, 128,
                                                plan.block_tables.shape[1], qkv.stride(0), out.stride(0),
                                                float(scale), _lib.stream_handle(qkv.device))
    _lib.check(rc, "paged_prefill_attention")
    return out


def ref_paged_prefill_attention(qkv, cache_layer, plan, heads, kv_heads, out=None, scale=None):
    """fp32 reference of :func:`paged_prefill_attention` (CPU or GPU tensors):
    per chunk, the context through :func:`kgs.ops.decode.ref_gather_kv` and a
    plain softmax(q k^T) v; rows ``>= n`` zero. Returns fp32 ``[rows, heads*128]``."""
    from .decode import ref_gather_kv

    scale = 1.0 / math.sqrt(128) if scale is None else scale
    res = torch.zeros((qkv.shape[0], heads * 128), dtype=torch.float32, device=qkv.device)
    rep = heads // kv_heads
    for ci, (row0, n, _, ctx0) in enumerate(plan.chunks):
        k, v = ref_gather_kv(cache_layer, plan.block_tables[ci], ctx0 + n)  # [ctx0+n, HKV, 128] fp32
        k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
        q = qkv[row0:row0 + n, :heads * 128].float().reshape(n, heads, 128)
        s = torch.einsum("qhd,khd->hqk", q, k) * scale
        dev = qkv.device
        seen = torch.arange(ctx0 + n, device=dev)[None, :] <= (ctx0 + torch.arange(n, device=dev))[:, None]
        p = torch.softmax(s.masked_fill(~seen, float("-inf")), dim=-1)
        res[row0:row0 + n] = torch.einsum("hqk,khd->qhd", p, v).reshape(n, heads * 128)
    if out is not None:
        out[:res.shape[0]].copy_(res)
        return out
    return res


def ref_attention_chunk(q, k, v, heads, kv_heads, head_dim=128, scale=None):
    """fp32 reference of :func:`attention_chunk` (bottom-right causal)."""
    S, Sk = q.shape[0], k.shape[0]
    qf = q[:, :heads * head_dim].float().reshape(S, heads, head_dim).transpose(0, 1)
    kf = k[:, :kv_heads * head_dim].float().reshape(Sk, kv_heads, head_dim).transpose(0, 1)
    vf = v[:, :kv_heads * head_dim].float().reshape(Sk, kv_heads, head_dim).transpose(0, 1)
    rep = heads // kv_heads
    kf, vf = kf.repeat_interleave(rep, 0), vf.repeat_interleave(rep, 0)
    mask = torch.arange(Sk, device=q.device)[None, :] <= (Sk - S + torch.arange(S, device=q.device))[:, None]
    o = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=mask, scale=scale)
    return o.transpose(0, 1).reshape(S, heads * head_dim)


# ----------------------------------------------------------------------------
# fp32 PyTorch references (tests, the "torch" model backend)

def ref_add_rmsnorm(x, d, w, eps=1e-5):
    """Returns (new residual bf16, normalised bf16) with the kernel's rounding points."""
    xs = x if d is None else (x.float() + d.float()).to(torch.bfloat16)
    xf = xs.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return xs, y.to(torch.bfloat16)


def ref_rope_qkv(qkv, cos, sin, heads, head_dim, seq):
    t = qkv.shape[0]
    x = qkv[:, :heads * head_dim].float().reshape(t, heads, head_dim)
    pos = torch.arange(t, device=qkv.device) % seq
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x1, x2 = x[..., :head_dim // 2], x[..., head_dim // 2:]
    rot = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1)
    out = qkv.clone()
    out[:, :heads * head_dim] = rot.reshape(t, heads * head_dim).to(qkv.dtype)
    return out


def ref_silu_mul(gu):
    i = gu.shape[1] // 2
    g, u = gu[:, :i].float(), gu[:, i:].float()
    return (g * torch.sigmoid(g) * u).to(torch.bfloat16)


def ref_attention_qkv(qkv, batch, seq, heads, kv_heads, head_dim=128, causal=True, scale=None):
    t = batch * seq
    q = qkv[:, :heads * head_dim].float().reshape(batch, seq, heads, head_dim).transpose(1, 2)
    k = qkv[:, heads * head_dim:(heads + kv_heads) * head_dim].float().reshape(batch, seq, kv_heads, head_dim)
    v = qkv[:, (heads + kv_heads) * head_dim:(heads + 2 * kv_heads) * head_dim].float().reshape(
        batch, seq, kv_heads, head_dim)
    rep = heads // kv_heads
    k = k.transpose(1, 2).repeat_interleave(rep, dim=1)
    v = v.transpose(1, 2).repeat_interleave(rep, dim=1)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale)
    return o.transpose(1, 2).reshape(t, heads * head_dim)


def ref_attention_qkv_backward(qkv, dout, batch, seq, heads, kv_heads, head_dim=128, causal=True, scale=None):
    """fp32 reference of :func:`attention_qkv_backward` (CPU or GPU tensors):
    autograd through :func:`ref_attention_qkv` on an fp32 leaf. Returns the fp32
    gradient in the fused layout ``[batch*seq, (heads + 2*kv_heads) * head_dim]``."""
    w = (heads + 2 * kv_heads) * head_dim
    leaf = qkv[:, :w].detach().float().clone().requires_grad_(True)
    with torch.enable_grad():
        o = ref_attention_qkv(leaf, batch, seq, heads, kv_heads, head_dim=head_dim, causal=causal, scale=scale)
    (g,) = torch.autograd.grad(o, leaf, dout[:, :heads * head_dim].detach().to(o.dtype))
    return g


# ----------------------------------------------------------------------------
# references of the training glue: the formulas stated directly (not through
# autograd, which the CPU tests compare them with), fp64 unless asked otherwise

def ref_rmsnorm_backward(x, w, dy, dres=None, eps=1e-5, dtype=torch.float64):
    """``(dx, dw)`` of :func:`rmsnorm_backward` in ``dtype``, unrounded."""
    xf, wf, gy = x.to(dtype), w.to(dtype), dy.to(dtype)
    cols = xf.shape[-1]
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    g = gy * wf
    c = (g * xf).sum(-1, keepdim=True) / cols
    dx = r * g - xf * r.pow(3) * c
    if dres is not None:
        dx = dres.to(dtype) + dx
    return dx, (gy * xf * r).sum(0)


def ref_silu_mul_backward(gu, dh, dtype=torch.float64):
    """``dgu`` (dgate | dup) of :func:`silu_mul_backward` in ``dtype``, unrounded."""
    i = gu.shape[1] // 2
    g, u, d = gu[:, :i].to(dtype), gu[:, i:].to(dtype), dh.to(dtype)
    s = torch.sigmoid(g)
    return torch.cat((d * u * s * (1 + g * (1 - s)), d * g * s), dim=1)


def ref_rope_qkv_backward(dout, cos, sin, heads, head_dim, seq, dtype=torch.float64):
    """Gradient of :func:`rope_qkv` in ``dtype``, unrounded: the transposed rotation
    ``(g1 c + g2 s, g2 c - g1 s)`` on the rotated heads, ``dout`` itself elsewhere."""
    t = dout.shape[0]
    g = dout[:, :heads * head_dim].to(dtype).reshape(t, heads, head_dim)
    pos = torch.arange(t, device=dout.device) % seq
    c, s = cos[pos][:, None, :].to(dtype), sin[pos][:, None, :].to(dtype)
    g1, g2 = g[..., :head_dim // 2], g[..., head_dim // 2:]
    rot = torch.cat((g1 * c + g2 * s, g2 * c - g1 * s), dim=-1).reshape(t, heads * head_dim)
    return torch.cat((rot, dout[:, heads * head_dim:].to(dtype)), dim=1)


def ref_cross_entropy_rows(logits, target, dtype=torch.float64):
    """``(loss, lse)`` of :func:`cross_entropy_rows` in ``dtype``."""
    x = logits.to(dtype)
    cols = x.shape[1]
    m = x.max(dim=1, keepdim=True).values
    lse = (m + (x - m).exp().sum(dim=1, keepdim=True).log())[:, 0]
    live = (target >= 0) & (target < cols)
    xt = x.gather(1, target.clamp(0, cols - 1)[:, None])[:, 0]
    return torch.where(live, lse - xt, torch.zeros_like(lse)), lse


def ref_cross_entropy_rows_backward(logits, target, lse, grow, dtype=torch.float64):
    """``dlogits`` of :func:`cross_entropy_rows_backward` in ``dtype``, unrounded."""
    x = logits.to(dtype)
    cols = x.shape[1]
    live = (target >= 0) & (target < cols)
    onehot = torch.arange(cols, device=x.device)[None, :] == target[:, None]
    d = grow.to(dtype)[:, None] * ((x - lse.to(dtype)[:, None]).exp() - onehot.to(dtype))
    return torch.where(live[:, None], d, torch.zeros_like(d))
