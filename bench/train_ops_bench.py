"""Training-glue timings on one MI355X: the train_ops kernels against the torch
bf16 autograd composites they replace, and one DecoderLayer step.

    python bench/train_ops_bench.py [--rounds 5 --iters 10] [--only norm swiglu rope loss layer]

One JSON line per op, forward + backward:

* ``norm``   -- ``rmsnorm_residual`` (delta added, residual gradient folded in), 16384 x 4096
* ``swiglu`` -- ``swiglu``, 16384 x 14336 (gate|up 28672 wide)
* ``rope``   -- ``rope_qkv`` on a QKV projection output, 16384 x (32 + 2*8) heads of 128
* ``loss``   -- ``softmax_cross_entropy``, 8192 x 128256
* ``layer``  -- one ``DecoderLayer`` step (dim 4096, heads 32/8, inter 14336, batch 4,
  seq 2048) against the same layer with kgs ``Linear`` and attention and torch glue
  (``glue="torch"``): the layer as it could be built before these kernels

The two sides alternate inside every round (same process, same tensors, device
events after a warm-up); medians and the min-max spread of the rounds are
reported. ``gbps`` is the traffic the op needs, computed here from the shapes
(each tensor read or written once, the small vectors ignored), over the time.
Random (gaussian) data.
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


def _alternate(fns: dict, rounds: int, iters: int) -> dict:
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            times[n].append(_time(f, iters))
    return {n: _stat(x) for n, x in times.items()}


def _report(op: str, shape: dict, nbytes: int, st: dict, rounds: int, extra: dict | None = None) -> None:
    kgs, ref = st["kgs"], st["torch"]
    spread = max((s["max"] - s["min"]) / s["ms"] for s in (kgs, ref))
    print(json.dumps({"op": op, **shape, "rounds": rounds, "kgs": kgs, "torch": ref, "bytes": nbytes,
                      "kgs_gbps": round(nbytes / kgs["ms"] / 1e6, 1), "torch_gbps": round(nbytes / ref["ms"] / 1e6, 1),
                      "speedup": round(ref["ms"] / kgs["ms"], 3), "spread": round(spread, 4), **(extra or {})}),
          flush=True)


def bench_norm(a):
    import torch

    from kgs.models.decoder import _torch_rmsnorm
    from kgs.ops.transformer import rmsnorm_residual

    rows, cols = 16384, 4096
    x, d, dres, dy = (torch.randn(rows, cols, device="cuda").bfloat16() for _ in range(4))
    w = (1 + 0.1 * torch.randn(cols, device="cuda")).bfloat16()
    xs, ds, ws = (t.clone().requires_grad_(True) for t in (x, d, w))

    def kgs():
        xs.grad = ds.grad = ws.grad = None
        res, y = rmsnorm_residual(xs, ds, ws)
        torch.autograd.backward([res, y], [dres, dy])

    def ref():
        xs.grad = ds.grad = ws.grad = None
        res = xs + ds
        torch.autograd.backward([res, _torch_rmsnorm(res, ws, 1e-5)], [dres, dy])

    # forward: read x, d, write res, y; backward: read res, dy, dres, write dx
    _report("norm", {"rows": rows, "cols": cols}, 8 * rows * cols * 2, _alternate({"kgs": kgs, "torch": ref},
                                                                                  a.rounds, a.iters), a.rounds)


def bench_swiglu(a):
    import torch

    from kgs.models.decoder import _torch_swiglu
    from kgs.ops.transformer import swiglu

    rows, inter = 16384, 14336
    gu = torch.randn(rows, 2 * inter, device="cuda").bfloat16().requires_grad_(True)
    dh = torch.randn(rows, inter, device="cuda").bfloat16()

    def kgs():
        gu.grad = None
        swiglu(gu).backward(dh)

    def ref():
        gu.grad = None
        _torch_swiglu(gu).backward(dh)

    # forward: read 2I, write I; backward: read 2I + I, write 2I
    _report("swiglu", {"rows": rows, "inter": inter}, 8 * rows * inter * 2,
            _alternate({"kgs": kgs, "torch": ref}, a.rounds, a.iters), a.rounds)


def bench_rope(a):
    import torch

    from kgs.models.attn_block import _rope
    from kgs.ops.transformer import rope_qkv, rope_tables

    b, s, nh, nkv, hd = 8, 2048, 32, 8, 128
    rows, width, rot = b * s, (nh + 2 * nkv) * hd, (nh + nkv) * hd
    qkv = torch.randn(rows, width, device="cuda").bfloat16().requires_grad_(True)
    dout = torch.randn(rows, width, device="cuda").bfloat16()
    cos, sin = rope_tables(s, hd, 10000.0, "cuda")

    def kgs():  # a leaf: rotated on a copy, as a caller that keeps qkv would have it
        qkv.grad = None
        rope_qkv(qkv, cos, sin, nh + nkv, hd, s).backward(dout)

    def ref():
        qkv.grad = None
        _rope(qkv, b, s, nh + nkv, hd, 10000.0).backward(dout)

    # each direction: one copy of the whole row (read + write) and the rotation in place (read + write)
    _report("rope", {"rows": rows, "width": width, "rotated": rot}, 2 * (2 * rows * width + 2 * rows * rot) * 2,
            _alternate({"kgs": kgs, "torch": ref}, a.rounds, a.iters), a.rounds)


def bench_loss(a):
    import torch

    from kgs.ops.transformer import softmax_cross_entropy

    rows, cols = 8192, 128256
    logits = torch.randn(rows, cols, device="cuda").bfloat16().requires_grad_(True)
    target = torch.randint(0, cols, (rows,), device="cuda")
    grow = torch.full((rows,), 1.0 / rows, device="cuda")

    def kgs():
        logits.grad = None
        softmax_cross_entropy(logits, target).backward(grow)

    def ref():
        logits.grad = None
        torch.nn.functional.cross_entropy(logits.float(), target, reduction="none").backward(grow)

    # forward: read the logits; backward: read them, write dlogits (its second read of a row is served by L2)
    _report("loss", {"rows": rows, "cols": cols}, 3 * rows * cols * 2,
            _alternate({"kgs": kgs, "torch": ref}, a.rounds, max(1, a.iters // 2)), a.rounds)


def bench_layer(a):
    import torch

    from kgs.models.decoder import DecoderLayer

    dim, nh, nkv, inter, b, s = 4096, 32, 8, 14336, 4, 2048
    layers = {"kgs": DecoderLayer(dim, nh, nkv, inter, backend="kgs", device="cuda"),
              "torch": DecoderLayer(dim, nh, nkv, inter, backend="kgs", glue="torch", device="cuda")}
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
    # same weights on both sides: how far apart the two layers' input gradients are
    grads = {}
    for n, layer in layers.items():
        step(layer)()
        grads[n] = xs.grad.float().clone()
    diff = ((grads["kgs"] - grads["torch"]).abs().max() / grads["torch"].abs().max()).item()
    kgs, ref = st["kgs"], st["torch"]
    spread = max((v["max"] - v["min"]) / v["ms"] for v in (kgs, ref))
    print(json.dumps({"op": "layer", "dim": dim, "heads": nh, "kv_heads": nkv, "inter": inter, "batch": b, "seq": s,
                      "rounds": a.rounds, "kgs": kgs, "torch_glue": ref, "speedup": round(ref["ms"] / kgs["ms"], 3),
                      "spread": round(spread, 4), "dx_rel_diff": round(diff, 5)}), flush=True)


BENCHES = {"norm": bench_norm, "swiglu": bench_swiglu, "rope": bench_rope, "loss": bench_loss, "layer": bench_layer}


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=sorted(BENCHES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_ops_bench needs a GPU")
    torch.manual_seed(0)
    for name in a.only or list(BENCHES):
        BENCHES[name](a)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
