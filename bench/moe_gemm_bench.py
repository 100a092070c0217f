"""Batched expert GEMM timings on one MI355X: ``native/kernels/moe_gemm.hip`` against a
loop of ``gemm_nt`` over the same capacity slabs, and one ``MoEFFN`` step with
``expert_gemm="batched"`` against ``"loop"``.

    python bench/moe_gemm_bench.py [--rounds 7 --iters 100] [--no-ffn] [--configs 8,2,2048 64,8,768]

16384 tokens of 4096 columns, capacity factor 1.25, E 8 / k 2 / inter 2048 and E 64 / k 8 /
inter 768; ``counts`` comes from a route of random logits. One JSON line per configuration and
part. Kernel lines: the three products of a gate|up ``moe_linear`` (``y`` and ``dx`` in mode
"rows", ``dW`` in mode "reduce") for both tile shapes of the kernel (``tile`` 0: 128 x 128,
2 stages, two workgroups per CU; 1: 256 x 128, 3 stages, one) against E ``gemm_nt`` launches on the
full slabs; ``tflops`` counts the filled rows only. The sides alternate inside every round (same
process, same tensors, device events after a warm-up); medians and min-max of the rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENS, DIM, FACTOR = 16384, 4096, 1.25


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


def _alternate(fns: dict, rounds: int, iters: int) -> dict:
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            times[n].append(_time(f, iters))
    return {n: {"ms": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}
            for n, x in times.items()}


def _kernel(num, k, inter, rounds, iters):
    import torch

    from kgs.models.moe import slab_capacity
    from kgs.ops import moe
    from kgs.ops.gemm import gemm_nt

    gen = torch.Generator(device="cuda").manual_seed(num)
    cap, n = slab_capacity(TOKENS, k, num, FACTOR), 2 * inter
    counts = moe.moe_route(torch.randn(TOKENS, num, device="cuda", generator=gen).bfloat16(), k, cap).counts
    live = (torch.arange(cap, device="cuda")[None, :] < counts.clamp(max=cap)[:, None])[..., None]
    xe = (torch.randn(num, cap, DIM, device="cuda", generator=gen) * live).bfloat16()
    dy = (torch.randn(num, cap, n, device="cuda", generator=gen) * live).bfloat16()
    w = torch.randn(num, n, DIM, device="cuda", generator=gen).bfloat16()
    wt, xt, dyt = (t.transpose(1, 2).contiguous() for t in (w, xe, dy))
    filled = int(counts.clamp(max=cap).sum())
    parts = {"y": (xe, w, "rows"), "dx": (dy, wt, "rows"), "dw": (dyt, xt, "reduce")}
    for what, (a, b, mode) in parts.items():
        fns = {"loop": lambda a=a, b=b: [gemm_nt(a[e], b[e]) for e in range(num)]}
        for tile in (0, 1):
            fns[f"tile{tile}"] = lambda a=a, b=b, mode=mode, tile=tile: moe.moe_gemm(a, b, counts, mode, tile=tile)
        st = _alternate(fns, rounds, iters)
        got, want = moe.moe_gemm(a, b, counts, mode), torch.stack([gemm_nt(a[e], b[e]) for e in range(num)])
        flops = 2.0 * filled * n * DIM
        yield {"part": what, "experts": num, "top_k": k, "inter": inter, "capacity": cap, "filled": filled,
               "shape": [num, a.shape[1], b.shape[1], a.shape[2]], "mode": mode, "rounds": rounds, "iters": iters, **st,
               "tflops": {s: round(flops / v["ms"] / 1e9, 1) for s, v in st.items()},
               "max_abs_diff_vs_loop": float((got.float() - want.float()).abs().max())}


def _ffn(num, k, inter, rounds, iters):
    import torch

    from kgs.models.moe import MoEFFN

    mods = {g: MoEFFN(DIM, inter, num, k, capacity_factor=FACTOR, device="cuda", expert_gemm=g)
            for g in ("loop", "batched")}
    gen = torch.Generator(device="cuda").manual_seed(1)
    h = torch.randn(TOKENS, DIM, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    dy = torch.randn(TOKENS, DIM, device="cuda", generator=gen).bfloat16()

    def step(m):
        def run():
            h.grad = None
            for p in m.parameters():
                p.grad = None
            m(h).backward(dy)
        return run

    st = _alternate({g: step(m) for g, m in mods.items()}, rounds, iters)
    outs = {g: m(h).detach().float() for g, m in mods.items()}
    return {"part": "moe_ffn_step", "experts": num, "top_k": k, "inter": inter, "tokens": TOKENS, "dim": DIM,
            "capacity": mods["loop"].capacity(TOKENS), "rounds": rounds, "iters": iters, **st,
            "speedup": round(st["loop"]["ms"] / st["batched"]["ms"], 3),
            "max_abs_diff_vs_loop": float((outs["batched"] - outs["loop"]).abs().max())}


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=100, help="launches per timed window (0.1 s or more)")
    ap.add_argument("--no-ffn", action="store_true", help="skip the MoEFFN steps")
    ap.add_argument("--no-kernel", action="store_true", help="skip the kernel lines")
    ap.add_argument("--configs", nargs="*", default=["8,2,2048", "64,8,768"], help="experts,top_k,inter")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("moe_gemm_bench needs a GPU")
    for cfg in a.configs:
        num, k, inter = (int(v) for v in cfg.split(","))
        if not a.no_kernel:
            for line in _kernel(num, k, inter, a.rounds, a.iters):
                print(json.dumps(line), flush=True)
        if not a.no_ffn:
            print(json.dumps(_ffn(num, k, inter, a.rounds, max(2, a.iters // 2))), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
