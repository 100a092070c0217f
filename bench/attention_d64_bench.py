"""Head_dim 64 flash-attention forward + backward timings on one MI355X.

    python bench/attention_d64_bench.py [--batch 4 --seq 2048 --heads 32 --kv-heads 8 --rounds 7]

The default shape is Llama-3.2-1B's attention (32 / 8 heads of 64). Per mask
(causal, full), one JSON line each for

* ``head_dim`` 64: the forward (``attention_qkv``), the forward with
  log-sum-exp and forward + backward (``attention_qkv_lse`` +
  ``attention_qkv_backward``, with the split of its three launches) against
  PyTorch-ROCm's ``scaled_dot_product_attention`` forward and forward +
  backward on the same values, pre-transposed to [B, H, S, D] (its best case:
  the layout change is not timed). That is what this shape had to run before
  the head_dim 64 kernels;
* ``head_dim`` 128, for context: the same kgs calls at the same batch, seq and
  head counts (no SDPA side).

All sides alternate inside every round (same process, same tensors); medians
and the min-max spread of the rounds are reported, and ``beats_spread`` says
whether SDPA's median minus the kgs median exceeds the larger of the two
spreads. TFLOP/s use the 4 (forward) + 10 (backward) . B.H.N^2.D convention,
halved under the causal mask, for both sides; the per-kernel figures count the
products a kernel executes (dK/dV 8, dQ 6). Random (gaussian) data.
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


def _kgs_fns(T, qkv, dout, dqkv, b, s, nh, nkv, hd, causal):
    out, lse = T.attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal, head_dim=hd)

    def bwd(stages=7):
        T.attention_qkv_backward(qkv, out, dout, lse, b, s, nh, nkv, causal=causal, dqkv=dqkv, head_dim=hd,
                                 _stages=stages)

    def fwd_bwd():
        o, l = T.attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal, head_dim=hd)
        T.attention_qkv_backward(qkv, o, dout, l, b, s, nh, nkv, causal=causal, dqkv=dqkv, head_dim=hd)

    return {"fwd": lambda: T.attention_qkv(qkv, b, s, nh, nkv, head_dim=hd, causal=causal, out=out),
            "fwd_lse": lambda: T.attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal, head_dim=hd),
            "fwd_bwd": fwd_bwd, "bwd": bwd, "bwd_prep": lambda: bwd(1), "bwd_dkdv": lambda: bwd(2),
            "bwd_dq": lambda: bwd(4)}


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
    ap.add_argument("--counters", type=int, default=0, metavar="N",
                    help="time nothing: N causal launches of each head_dim 64 and 128 kernel (the program of a "
                         "rocprofv3 --pmc pass; the kernels are told apart by name in its CSV)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("attention_d64_bench needs a GPU")
    dev = "cuda"
    b, s, nh, nkv = a.batch, a.seq, a.heads, a.kv_heads
    t = b * s
    torch.manual_seed(0)
    data = {}
    for hd in (64, 128):
        qkv = torch.randn(t, (nh + 2 * nkv) * hd, device=dev).to(torch.bfloat16)
        dout = torch.randn(t, nh * hd, device=dev).to(torch.bfloat16)
        data[hd] = (qkv, dout, torch.empty_like(qkv))
    if a.counters:
        for hd in (64, 128):
            fns = _kgs_fns(T, *data[hd], b, s, nh, nkv, hd, True)
            for _ in range(a.counters):
                fns["fwd"]()
                fns["fwd_bwd"]()
        torch.cuda.synchronize()
        print("ok", flush=True)
        return 0
    qkv, dout, dqkv = data[64]
    q = qkv[:, :nh * 64].reshape(b, s, nh, 64).transpose(1, 2).contiguous().requires_grad_(True)
    k = qkv[:, nh * 64:(nh + nkv) * 64].reshape(b, s, nkv, 64).transpose(1, 2).contiguous().requires_grad_(True)
    v = qkv[:, (nh + nkv) * 64:].reshape(b, s, nkv, 64).transpose(1, 2).contiguous().requires_grad_(True)
    do_t = dout.reshape(b, s, nh, 64).transpose(1, 2).contiguous()
    for causal in (True, False):
        def sdpa_fwd():
            with torch.no_grad():
                torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=True)

        def sdpa_fwd_bwd():
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=True)
            q.grad = k.grad = v.grad = None
            o.backward(do_t)

        fns = {f"d{hd}_{n}": f for hd in (64, 128)
               for n, f in _kgs_fns(T, *data[hd], b, s, nh, nkv, hd, causal).items()}
        fns.update(sdpa_fwd=sdpa_fwd, sdpa_fwd_bwd=sdpa_fwd_bwd)
        times = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, f in fns.items():
                times[n].append(_time(f, a.iters))
        st = {n: _stat(x) for n, x in times.items()}
        # same values on both sides: the SDPA dq against the kgs one (the
        # single-stage timings above ran on an unset delta: recompute dqkv)
        sdpa_fwd_bwd()
        fns["d64_bwd"]()
        torch.cuda.synchronize()
        dq_ref = q.grad.transpose(1, 2).reshape(t, nh * 64).float()
        err = ((dqkv[:, :nh * 64].float() - dq_ref).abs().max() / dq_ref.abs().max()).item()
        for hd in (64, 128):
            unit = b * nh * s * s * hd * (0.5 if causal else 1.0)
            g = {n: st[f"d{hd}_{n}"] for n in ("fwd", "fwd_lse", "fwd_bwd", "bwd", "bwd_prep", "bwd_dkdv", "bwd_dq")}
            line = {"op": "attention_d64_bench", "head_dim": hd, "causal": causal, "batch": b, "seq": s, "heads": nh,
                    "kv_heads": nkv, "rounds": a.rounds, **g,
                    "fwd_tflops": round(4 * unit / g["fwd"]["ms"] / 1e9, 1),
                    "fwd_lse_tflops": round(4 * unit / g["fwd_lse"]["ms"] / 1e9, 1),
                    "fwd_bwd_tflops": round(14 * unit / g["fwd_bwd"]["ms"] / 1e9, 1),
                    "bwd_tflops": round(10 * unit / g["bwd"]["ms"] / 1e9, 1),
                    "bwd_dkdv_mfma_tflops": round(8 * unit / g["bwd_dkdv"]["ms"] / 1e9, 1),
                    "bwd_dq_mfma_tflops": round(6 * unit / g["bwd_dq"]["ms"] / 1e9, 1)}
            if hd == 64:
                for n, mine in (("fwd", g["fwd"]), ("fwd_bwd", g["fwd_bwd"])):
                    other = st[f"sdpa_{n}"]
                    spread = max(mine["max"] - mine["min"], other["max"] - other["min"])
                    line.update({f"sdpa_{n}": other, f"{n}_speedup": round(other["ms"] / mine["ms"], 3),
                                 f"{n}_spread_ms": round(spread, 4),
                                 f"{n}_beats_spread": bool(other["ms"] - mine["ms"] > spread)})
                line["sdpa_fwd_bwd_tflops"] = round(14 * unit / st["sdpa_fwd_bwd"]["ms"] / 1e9, 1)
                line["dq_rel_diff_vs_sdpa"] = round(err, 5)
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
