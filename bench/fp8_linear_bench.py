"""The fp8 training Linear on one MI355X: forward + backward of ``kgs.ops.LinearFp8``
against the bf16 ``kgs.ops.Linear``, the two quantising kernels on their own,
and one DecoderLayer step with ``linear="fp8"`` against ``"bf16"``.

    python bench/fp8_linear_bench.py [--rounds 7 --iters 10] [--only linear kernels layer]

One JSON line per measurement:

* ``linear``  -- forward + backward (dX and dW) at the four Llama-3-8B projection
  shapes (qkv 4096 -> 6144, o 4096 -> 4096, gate|up 4096 -> 28672, down 14336 ->
  4096) with T = 8192 and T = 16384 tokens. ``tflops`` counts the three GEMMs
  (6 T K N) over the whole time, quantising passes included.
* ``kernels`` -- ``fp8_amax`` and ``fp8_quantize`` alone on the operands of those
  shapes, in microseconds and in TB/s of the bytes they must move (the matrix
  read once as bf16, each image written once as one byte per element; the amax
  and scale vectors ignored).
* ``layer``   -- one DecoderLayer step (dim 4096, heads 32/8, inter 14336, batch 4,
  seq 2048, the shape of profiles/r12/train_ops) with the four projections in fp8
  against bf16, same weights, and how far apart the two input gradients are.

The two routes alternate inside every round (same process, same tensors, device
events after a warm-up); medians and the min-max spread of the rounds are
reported. Random (gaussian) data.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROJECTIONS = {"qkv": (4096, 6144), "o": (4096, 4096), "gate_up": (4096, 28672), "down": (14336, 4096)}
TOKENS = (8192, 16384)


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


def _graphed(fn, iters):
    """``iters`` calls of ``fn`` captured into one hipGraph: a kernel of tens of
    microseconds is timed without the host's per-call cost between launches."""
    import torch

    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def _stat(xs):
    return {"ms": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _alternate(fns: dict, rounds: int, iters: int) -> dict:
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            times[n].append(_time(f, iters))
    return {n: _stat(x) for n, x in times.items()}


def _spread(stats) -> float:
    return round(max((s["max"] - s["min"]) / s["ms"] for s in stats), 4)


def _linear_step(lin, x, dy):
    def run():
        x.grad = None
        lin.weight.grad = None
        lin(x).backward(dy)
    return run


def bench_linear(a):
    import torch

    from kgs.ops import Linear, LinearFp8

    for name, (K, N) in PROJECTIONS.items():
        lins = {"fp8": LinearFp8(K, N, device="cuda"), "bf16": Linear(K, N, bias=False, device="cuda")}
        with torch.no_grad():
            lins["bf16"].weight.copy_(lins["fp8"].weight)
        for T in TOKENS:
            x = torch.randn(T, K, device="cuda").bfloat16().requires_grad_(True)
            dy = torch.randn(T, N, device="cuda").bfloat16()
            st = _alternate({n: _linear_step(lin, x, dy) for n, lin in lins.items()}, a.rounds, a.iters)
            grads = {}
            for n, lin in lins.items():
                _linear_step(lin, x, dy)()
                grads[n] = (x.grad.float().clone(), lin.weight.grad.float().clone())
            rel = [((f - b).norm() / b.norm()).item() for f, b in zip(grads["fp8"], grads["bf16"])]
            flop = 6.0 * T * K * N
            print(json.dumps({"op": "linear", "proj": name, "T": T, "K": K, "N": N, "rounds": a.rounds,
                              "fp8": st["fp8"], "bf16": st["bf16"],
                              "fp8_tflops": round(flop / st["fp8"]["ms"] / 1e9, 1),
                              "bf16_tflops": round(flop / st["bf16"]["ms"] / 1e9, 1),
                              "speedup": round(st["bf16"]["ms"] / st["fp8"]["ms"], 3),
                              "spread": _spread(st.values()), "dx_rel_fro": round(rel[0], 4),
                              "dw_rel_fro": round(rel[1], 4)}), flush=True)
            del x, dy, grads
        del lins
        torch.cuda.empty_cache()


def _kernel_cases(x, ra, ca, ta, y, yt, one):
    """name -> (call, bytes it must move): the matrix read as bf16, each image written as one byte per element"""
    from kgs.ops import fp8_amax, fp8_quantize

    elems = x.numel()
    return {
        "amax rows+tensor": (lambda: fp8_amax(x, rows=True, tensor=True), 2 * elems),
        "amax rows+cols": (lambda: fp8_amax(x, rows=True, cols=True), 2 * elems),
        "amax tensor": (lambda: fp8_amax(x, tensor=True), 2 * elems),
        "quant y(row)+yt(tensor)": (lambda: fp8_quantize(x, row_amax=ra, tensor_amax=ta, y=y, yt=yt, y_fold=one),
                                    4 * elems),
        "quant y(row)+yt(col)": (lambda: fp8_quantize(x, row_amax=ra, col_amax=ca, y=y, yt=yt, y_fold=one,
                                                      yt_fold=one), 4 * elems),
        "quant y(tensor)": (lambda: fp8_quantize(x, tensor_amax=ta, y=y), 3 * elems),
        "quant yt(tensor)": (lambda: fp8_quantize(x, tensor_amax=ta, y=False, yt=yt), 3 * elems),
    }


def bench_kernels(a):
    import torch

    from kgs.ops import fp8_amax

    one = torch.ones(1, device="cuda")
    for rows, cols in ((8192, 4096), (16384, 4096), (8192, 14336), (16384, 28672), (28672, 4096)):
        x = torch.randn(rows, cols, device="cuda").bfloat16()
        ra, ca, ta = fp8_amax(x, rows=True, cols=True, tensor=True)
        y, yt = (torch.empty(s, dtype=torch.float8_e4m3fn, device="cuda") for s in ((rows, cols), (cols, rows)))
        cases = _kernel_cases(x, ra, ca, ta, y, yt, one)
        per = 10  # calls per graph replay
        st = _alternate({n: _graphed(f, per) for n, (f, _) in cases.items()}, a.rounds, a.iters)
        for n, (_, nbytes) in cases.items():
            us = {k: 1e3 * v / per for k, v in st[n].items()}
            print(json.dumps({"op": "kernel", "what": n, "rows": rows, "cols": cols, "rounds": a.rounds,
                              "us": round(us["ms"], 1), "min_us": round(us["min"], 1), "max_us": round(us["max"], 1),
                              "bytes": nbytes, "tbps": round(nbytes / us["ms"] / 1e6, 2)}), flush=True)
        del x, y, yt, st
        torch.cuda.empty_cache()


def bench_layer(a):
    import torch

    from kgs.models.decoder import DecoderLayer

    dim, nh, nkv, inter, b, s = 4096, 32, 8, 14336, 4, 2048
    layers = {"fp8": DecoderLayer(dim, nh, nkv, inter, backend="kgs", device="cuda", linear="fp8"),
              "bf16": DecoderLayer(dim, nh, nkv, inter, backend="kgs", device="cuda")}
    x, d, dy1, dy2 = (torch.randn(b, s, dim, device="cuda").bfloat16() for _ in range(4))
    xs, ds = x.clone().requires_grad_(True), d.clone().requires_grad_(True)

    def step(layer):
        def run():
            xs.grad = ds.grad = None
            layer.zero_grad(set_to_none=True)
            res, out = layer(xs, ds)
            torch.autograd.backward([res, out], [dy1, dy2])
        return run

    st = _alternate({n: step(layer) for n, layer in layers.items()}, a.rounds, max(1, a.iters // 2))
    grads = {}
    for n, layer in layers.items():  # the same seeded weights on both sides
        step(layer)()
        grads[n] = xs.grad.float().clone()
    diff = ((grads["fp8"] - grads["bf16"]).norm() / grads["bf16"].norm()).item()
    print(json.dumps({"op": "layer", "dim": dim, "heads": nh, "kv_heads": nkv, "inter": inter, "batch": b, "seq": s,
                      "rounds": a.rounds, "fp8": st["fp8"], "bf16": st["bf16"],
                      "speedup": round(st["bf16"]["ms"] / st["fp8"]["ms"], 3), "spread": _spread(st.values()),
                      "dx_rel_fro": round(diff, 4)}), flush=True)


BENCHES = {"linear": bench_linear, "kernels": bench_kernels, "layer": bench_layer}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=sorted(BENCHES))
    a = ap.parse_args(argv)
    if a.rounds < 1 or a.iters < 1:
        raise SystemExit("rounds and iters must be positive")
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("fp8_linear_bench needs a GPU")
    torch.manual_seed(0)
    for name in a.only or list(BENCHES):
        BENCHES[name](a)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
