"""Sliding-window flash-attention forward + backward timings on one MI355X.

    python bench/attention_window_bench.py [--batch 4 --heads 32 --kv-heads 8 --rounds 5]

Sweeps ``seq`` in {2048, 8192} x ``window`` in {128, 1024, 4096} (``window <
seq``) at head_dim 128 and prints one JSON line per shape with

* ``win_*``: the windowed forward (``attention_qkv(window=W)``), forward +
  backward (``attention_qkv_lse`` + ``attention_qkv_backward``) and the split of
  the backward's three launches (``native/kernels/attention_window.hip``);
* ``causal_*``: the plain causal kgs kernels at the same ``seq``. They compute a
  different function (every earlier key): this is what the shape cost before
  the window kernels, the cost baseline;
* ``sdpa_*``: PyTorch-ROCm's ``scaled_dot_product_attention`` with the dense
  boolean ``[S, S]`` window mask on the same values, pre-transposed to
  [B, H, S, D] (the layout change is not timed): the only route that computed
  the windowed function before.

All sides alternate inside every round (same process, same tensors); medians
and the min-max spread of the rounds are reported. ``fwd_bwd_vs_causal`` is the
windowed forward + backward time over the causal kernels', next to
``visible_ratio``, the windowed mask's share of the causal mask's score
entries; ``*_beats_spread`` says whether a difference of medians exceeds the
larger of the two spreads. TFLOP/s count the unmasked products only: 4
(forward) + 10 (backward) . B.H.D per visible score entry. Random (gaussian)
data.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HD = 128


def _time(fn, iters, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _stat(xs):
    return {"ms": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _kgs_fns(T, qkv, dout, dqkv, b, s, nh, nkv, window):
    out, lse = T.attention_qkv_lse(qkv, b, s, nh, nkv, window=window)

    def bwd(stages=7):
        T.attention_qkv_backward(qkv, out, dout, lse, b, s, nh, nkv, dqkv=dqkv, _stages=stages, window=window)

    def fwd_bwd():
        o, l = T.attention_qkv_lse(qkv, b, s, nh, nkv, window=window)
        T.attention_qkv_backward(qkv, o, dout, l, b, s, nh, nkv, dqkv=dqkv, window=window)

    return {"fwd": lambda: T.attention_qkv(qkv, b, s, nh, nkv, out=out, window=window), "fwd_bwd": fwd_bwd, "bwd": bwd,
            "bwd_prep": lambda: bwd(1), "bwd_dkdv": lambda: bwd(2), "bwd_dq": lambda: bwd(4)}


def _versus(line, name, mine, other):
    spread = max(mine["max"] - mine["min"], other["max"] - other["min"])
    line.update({f"{name}_spread_ms": round(spread, 4), f"{name}_beats_spread": bool(abs(other["ms"] - mine["ms"]) > spread)})


def main(argv=None) -> int:
    import torch

    from kgs.ops import transformer as T

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--seqs", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--windows", type=int, nargs="+", default=[128, 1024, 4096])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sdpa-iters", type=int, default=3, help="the dense-mask SDPA runs are long: fewer per round")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved timing rounds (medians reported)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("attention_window_bench needs a GPU")
    dev = "cuda"
    b, nh, nkv = a.batch, a.heads, a.kv_heads
    torch.manual_seed(0)
    for s in a.seqs:
        t = b * s
        qkv = torch.randn(t, (nh + 2 * nkv) * HD, device=dev).to(torch.bfloat16)
        dout = torch.randn(t, nh * HD, device=dev).to(torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        q = qkv[:, :nh * HD].reshape(b, s, nh, HD).transpose(1, 2).contiguous().requires_grad_(True)
        k = qkv[:, nh * HD:(nh + nkv) * HD].reshape(b, s, nkv, HD).transpose(1, 2).contiguous().requires_grad_(True)
        v = qkv[:, (nh + nkv) * HD:].reshape(b, s, nkv, HD).transpose(1, 2).contiguous().requires_grad_(True)
        do_t = dout.reshape(b, s, nh, HD).transpose(1, 2).contiguous()
        for window in [w for w in a.windows if w < s]:
            mask = T._window_mask(s, window, dev)

            def sdpa_fwd():
                with torch.no_grad():
                    torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True)

            def sdpa_fwd_bwd():
                o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True)
                q.grad = k.grad = v.grad = None
                o.backward(do_t)

            fns = {f"win_{n}": f for n, f in _kgs_fns(T, qkv, dout, dqkv, b, s, nh, nkv, window).items()}
            fns.update({f"causal_{n}": f for n, f in _kgs_fns(T, qkv, dout, dqkv, b, s, nh, nkv, None).items()
                        if n in ("fwd", "fwd_bwd")})
            fns.update(sdpa_fwd=sdpa_fwd, sdpa_fwd_bwd=sdpa_fwd_bwd)
            times = {n: [] for n in fns}
            for _ in range(a.rounds):
                for n, f in fns.items():
                    sd = n.startswith("sdpa")
                    times[n].append(_time(f, a.sdpa_iters if sd else a.iters, 1 if sd else 2))
            st = {n: _stat(x) for n, x in times.items()}
            # same values on both sides: the SDPA dq against the kgs one (the
            # single-stage timings above ran on an unset delta: recompute dqkv)
            sdpa_fwd_bwd()
            fns["win_bwd"]()
            torch.cuda.synchronize()
            dq_ref = q.grad.transpose(1, 2).reshape(t, nh * HD).float()
            err = ((dqkv[:, :nh * HD].float() - dq_ref).abs().max() / dq_ref.abs().max()).item()
            visible = window * (window + 1) // 2 + (s - window) * window  # score entries per (batch, head)
            unit = b * nh * visible * HD
            line = {"op": "attention_window_bench", "batch": b, "seq": s, "heads": nh, "kv_heads": nkv, "window": window,
                    "rounds": a.rounds, **st,
                    "win_fwd_tflops": round(4 * unit / st["win_fwd"]["ms"] / 1e9, 1),
                    "win_fwd_bwd_tflops": round(14 * unit / st["win_fwd_bwd"]["ms"] / 1e9, 1),
                    "win_bwd_dkdv_mfma_tflops": round(8 * unit / st["win_bwd_dkdv"]["ms"] / 1e9, 1),
                    "win_bwd_dq_mfma_tflops": round(6 * unit / st["win_bwd_dq"]["ms"] / 1e9, 1),
                    "visible_ratio": round(visible / (s * (s + 1) // 2), 4),
                    "fwd_vs_causal": round(st["win_fwd"]["ms"] / st["causal_fwd"]["ms"], 4),
                    "fwd_bwd_vs_causal": round(st["win_fwd_bwd"]["ms"] / st["causal_fwd_bwd"]["ms"], 4),
                    "fwd_bwd_vs_sdpa": round(st["win_fwd_bwd"]["ms"] / st["sdpa_fwd_bwd"]["ms"], 4),
                    "dq_rel_diff_vs_sdpa": round(err, 5)}
            _versus(line, "fwd_vs_causal", st["win_fwd"], st["causal_fwd"])
            _versus(line, "fwd_bwd_vs_causal", st["win_fwd_bwd"], st["causal_fwd_bwd"])
            _versus(line, "fwd_bwd_vs_sdpa", st["win_fwd_bwd"], st["sdpa_fwd_bwd"])
            print(json.dumps(line), flush=True)
            del mask
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
