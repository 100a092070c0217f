"""Fused LM head + loss timings and peak memory on one MI355X: ``native/kernels/linear_xent.hip``
against ``kgs.ops.linear`` + ``softmax_cross_entropy`` on the same tensors.

    python bench/linear_xent_bench.py [--rounds 7 --iters 5] [--no-kernel] [--chunks 4096 16384 65536]

8192 tokens x 4096 columns x a vocabulary of 128256. One JSON line per part:

* ``step``: forward + backward (dh and dW) of ``linear_cross_entropy`` per backward chunk size against
  the unfused pair, and ``torch.cuda.max_memory_allocated`` of one step of each above the operands alone
  (the gradients of the step before are dropped first, so ``h.grad`` and ``w.grad`` are inside every figure).
* ``fwd``: the raw forward per tile shape (0: 128 x 128, 2 stages; 1: 256 x 128, 3 stages) against
  ``gemm_nt`` writing the logits.
* ``dlogits``: the raw backward piece over one default chunk per tile shape against ``gemm_nt``.

The sides alternate inside every round (same process, same tensors, device events after a warm-up);
medians and min-max of the rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters, warmup=1):
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


def _peak(fn, clear) -> float:
    """MiB allocated at the peak of one call above what was allocated before it, after ``clear()``
    dropped what the call before left: every side starts from the operands alone."""
    import torch

    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--shape", type=int, nargs=3, default=[8192, 4096, 128256], metavar=("T", "K", "V"))
    ap.add_argument("--chunks", type=int, nargs="*", default=[4096, 16384, 65536], help="backward chunk sizes")
    ap.add_argument("--no-kernel", action="store_true", help="skip the raw kernel lines")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("linear_xent_bench needs a GPU")
    from kgs.ops import linear_xent as lx
    from kgs.ops.gemm import gemm_nt, linear
    from kgs.ops.transformer import softmax_cross_entropy

    t, k, v = a.shape
    gen = torch.Generator(device="cuda").manual_seed(0)
    h = torch.randn(t, k, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    w = (torch.randn(v, k, device="cuda", generator=gen) * k ** -0.5).bfloat16().requires_grad_(True)
    tg = torch.randint(0, v, (t,), device="cuda", generator=gen)
    grow = torch.full((t,), 1.0 / t, device="cuda")
    tiles = (0, 1) if t % 256 == 0 else (0,)
    shape = {"tokens": t, "dim": k, "vocab": v, "rounds": a.rounds, "iters": a.iters}

    def step(loss_rows):
        def run():
            h.grad = w.grad = None
            loss_rows().backward(grow)
        return run

    fns = {"unfused": step(lambda: softmax_cross_entropy(linear(h, w), tg))}
    for c in a.chunks:
        fns[f"fused_chunk{c}"] = step(lambda c=c: lx.linear_cross_entropy(h, w, tg, chunk=c))
    st = _alternate(fns, a.rounds, a.iters)

    def clear():
        h.grad = w.grad = None

    peaks = {n: _peak(f, clear) for n, f in fns.items()}
    print(json.dumps({"part": "step", **shape, "default_chunk": lx.default_chunk(t, v), **st, "peak_mib": peaks,
                      "logits_mib": round(t * v * 2 / 2 ** 20, 1),
                      "time_vs_unfused": {n: round(x["ms"] / st["unfused"]["ms"], 3) for n, x in st.items()}}),
          flush=True)
    if a.no_kernel:
        return 0
    h.grad = w.grad = None
    hd, wd = h.detach(), w.detach()
    fns = {"gemm_nt": lambda: gemm_nt(hd, wd)}
    for tile in tiles:
        fns[f"tile{tile}"] = lambda tile=tile: lx.linear_cross_entropy_rows(hd, wd, tg, tile=tile)
    st = _alternate(fns, a.rounds, a.iters)
    flops = 2.0 * t * k * v
    print(json.dumps({"part": "fwd", **shape, **st, "tflops": {n: round(flops / x["ms"] / 1e9, 1) for n, x in st.items()}}),
          flush=True)
    c = lx.default_chunk(t, v)
    lse = lx.linear_cross_entropy_rows(hd, wd, tg)[1]
    out = torch.empty(t, c, dtype=torch.bfloat16, device="cuda")
    fns = {"gemm_nt": lambda: gemm_nt(hd, wd[:c], out=out)}
    for tile in tiles:
        fns[f"tile{tile}"] = lambda tile=tile: lx.linear_cross_entropy_dlogits(hd, wd, tg, lse, grow, (0, c), out=out,
                                                                               tile=tile)
    st = _alternate(fns, a.rounds, a.iters * 4)
    flops = 2.0 * t * k * c
    print(json.dumps({"part": "dlogits", **shape, "cols": c, **st,
                      "tflops": {n: round(flops / x["ms"] / 1e9, 1) for n, x in st.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
