"""Flash-attention forward + backward timings on one MI355X.

    python bench/attention_bwd_bench.py [--batch 4 --seq 2048 --heads 32 --kv-heads 8 --rounds 7]

Per mask (causal, full), one JSON line each for

* ``fwd_lse`` (``kgs.ops.attention_qkv_lse``) against the production forward
  (``kgs.ops.attention_qkv``): the log-sum-exp store should be free;
* kgs ``fwd_lse`` + backward (``attention_qkv_backward``: delta, dK/dV, dQ)
  against PyTorch-ROCm's ``scaled_dot_product_attention`` forward + backward on
  the same values, pre-transposed to [B, H, S, D] (its best case: the layout
  change is not timed), with the split of the three backward launches.

The sides alternate inside every round (same process, same tensors); medians
and the min-max spread of the rounds are reported. TFLOP/s use the
4 (forward) + 10 (backward) . B.H.N^2.D convention, halved under the causal
mask, for BOTH sides -- the kgs backward executes 14, its price for dQ without
atomics or a cross-workgroup hand-off. Random (gaussian) data.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main(argv=None) -> int:
    import torch

    from kgs.ops import transformer as T

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("attention_bwd_bench needs a GPU")
    dev, hd = "cuda", 128
    b, s, nh, nkv = a.batch, a.seq, a.heads, a.kv_heads
    t = b * s
    torch.manual_seed(0)
    qkv = torch.randn(t, (nh + 2 * nkv) * hd, device=dev).to(torch.bfloat16)
    dout = torch.randn(t, nh * hd, device=dev).to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    q = qkv[:, :nh * hd].reshape(b, s, nh, hd).transpose(1, 2).contiguous().requires_grad_(True)
    k = qkv[:, nh * hd:(nh + nkv) * hd].reshape(b, s, nkv, hd).transpose(1, 2).contiguous().requires_grad_(True)
    v = qkv[:, (nh + nkv) * hd:].reshape(b, s, nkv, hd).transpose(1, 2).contiguous().requires_grad_(True)
    do_t = dout.reshape(b, s, nh, hd).transpose(1, 2).contiguous()
    for causal in (True, False):
        unit = b * nh * s * s * hd * (0.5 if causal else 1.0)
        out, lse = T.attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal)

        def bwd(stages=7):
            T.attention_qkv_backward(qkv, out, dout, lse, b, s, nh, nkv, causal=causal, dqkv=dqkv, _stages=stages)

        def kgs_fwd_bwd():
            o, l = T.attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal)
            T.attention_qkv_backward(qkv, o, dout, l, b, s, nh, nkv, causal=causal, dqkv=dqkv)

        def sdpa_fwd():
            with torch.no_grad():
                torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=True)

        def sdpa_fwd_bwd():
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=True)
            q.grad = k.grad = v.grad = None
            o.backward(do_t)

        fns = {"fwd": lambda: T.attention_qkv(qkv, b, s, nh, nkv, causal=causal, out=out),
               "fwd_lse": lambda: T.attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal),
               "kgs_fwd_bwd": kgs_fwd_bwd, "sdpa_fwd": sdpa_fwd, "sdpa_fwd_bwd": sdpa_fwd_bwd,
               "bwd": bwd, "bwd_prep": lambda: bwd(1), "bwd_dkdv": lambda: bwd(2), "bwd_dq": lambda: bwd(4)}
        times = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, f in fns.items():
                times[n].append(_time(f, a.iters))
        st = {n: _stat(x) for n, x in times.items()}
        print(json.dumps({"op": "attention_fwd_lse", "causal": causal, "batch": b, "seq": s, "heads": nh,
                          "kv_heads": nkv, "rounds": a.rounds, "fwd": st["fwd"], "fwd_lse": st["fwd_lse"],
                          "fwd_tflops": round(4 * unit / st["fwd"]["ms"] / 1e9, 1),
                          "fwd_lse_tflops": round(4 * unit / st["fwd_lse"]["ms"] / 1e9, 1),
                          "fwd_lse_over_fwd": round(st["fwd_lse"]["ms"] / st["fwd"]["ms"], 4)}), flush=True)
        # same values on both sides: the SDPA gradients against the kgs ones
        # (the single-stage timings above ran on an unset delta: recompute dqkv)
        sdpa_fwd_bwd()
        bwd()
        torch.cuda.synchronize()
        dq_ref = q.grad.transpose(1, 2).reshape(t, nh * hd).float()
        err = ((dqkv[:, :nh * hd].float() - dq_ref).abs().max() / dq_ref.abs().max()).item()
        print(json.dumps({"op": "attention_fwd_bwd", "causal": causal, "batch": b, "seq": s, "heads": nh,
                          "kv_heads": nkv, "rounds": a.rounds, "kgs_fwd_bwd": st["kgs_fwd_bwd"],
                          "sdpa_fwd_bwd": st["sdpa_fwd_bwd"], "sdpa_fwd": st["sdpa_fwd"],
                          "kgs_tflops": round(14 * unit / st["kgs_fwd_bwd"]["ms"] / 1e9, 1),
                          "sdpa_tflops": round(14 * unit / st["sdpa_fwd_bwd"]["ms"] / 1e9, 1),
                          "speedup": round(st["sdpa_fwd_bwd"]["ms"] / st["kgs_fwd_bwd"]["ms"], 3),
                          "kgs_bwd": st["bwd"], "kgs_bwd_tflops": round(10 * unit / st["bwd"]["ms"] / 1e9, 1),
                          "bwd_prep": st["bwd_prep"], "bwd_dkdv": st["bwd_dkdv"], "bwd_dq": st["bwd_dq"],
                          "bwd_dkdv_mfma_tflops": round(8 * unit / st["bwd_dkdv"]["ms"] / 1e9, 1),
                          "bwd_dq_mfma_tflops": round(6 * unit / st["bwd_dq"]["ms"] / 1e9, 1),
                          "dq_rel_diff_vs_sdpa": round(err, 5)}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
