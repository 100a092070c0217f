"""Mixture-of-experts routing timings on one MI355X: the kernels of
``native/kernels/moe_route.hip`` against the same steps as torch composites.

    python bench/moe_bench.py [--rounds 7 --iters 20] [--no-ffn]

16384 tokens of 4096 columns, 8 experts / top-2 and 64 experts / top-8, capacity
factor 1.25. One JSON line per configuration: for route, dispatch and combine,
forward and backward, the median and min-max of the rounds for each side, which
alternate inside every round (same process, same tensors, device events after a
warm-up), the bytes the step must move and the rate that makes for the kernels.
The torch side is ``sort`` + ``softmax`` + a stable ``sort`` / ``bincount`` / ``cumsum``
for the slots (``ref_moe_route`` in fp32), ``index_select`` for the dispatch, and a
gather, a weighted fp32 sum and autograd for the rest. Bytes: route, the logits in
and the four tables out; dispatch, the filled rows in and every slot row out;
combine (and the dispatch's backward), the filled rows in and the token rows out;
the combine's backward, ``dy`` twice, the filled rows of ``ye`` in and every slot row
of ``dye`` out. A last line times one :class:`kgs.models.moe.MoEFFN` step, forward
and backward, against the same module with the routing done by those torch
composites around the same GEMM and SwiGLU kernels.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENS, DIM, FACTOR = 16384, 4096, 1.25
CONFIGS = ((8, 2), (64, 8))
FFN = {"experts": 8, "top_k": 2, "inter": 2048}


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


def _torch_combine(ye, slot, weights):
    import torch

    picked = ye[slot.long().clamp(min=0)].float()
    w = torch.where(slot >= 0, weights, 0.0)
    return (picked * w[..., None]).sum(1).to(torch.bfloat16)


def _routing(num, k, rounds, iters):
    import torch

    from kgs.ops import moe

    gen = torch.Generator(device="cuda").manual_seed(num)
    cap = -(-int(FACTOR * TOKENS * k) // num)
    cap = (cap + 255) // 256 * 256
    logits = torch.randn(TOKENS, num, device="cuda", generator=gen).bfloat16()
    x, dy = (torch.randn(TOKENS, DIM, device="cuda", generator=gen).bfloat16() for _ in range(2))
    ye, dxe = (torch.randn(num * cap, DIM, device="cuda", generator=gen).bfloat16() for _ in range(2))
    r = moe.moe_route(logits, k, cap)
    dw = torch.randn(TOKENS, k, device="cuda", generator=gen)
    filled, ones = int((r.src >= 0).sum()), torch.ones_like(r.weights)
    rows = (r.src.long().clamp(min=0) // k)
    lleaf, yleaf, wleaf = logits.clone().requires_grad_(True), ye.clone().requires_grad_(True), \
        r.weights.clone().requires_grad_(True)

    def torch_route_bwd():
        lleaf.grad = None
        torch.softmax(lleaf.float().gather(1, r.experts.long()), 1).backward(dw)

    def torch_combine_bwd():
        yleaf.grad = wleaf.grad = None
        _torch_combine(yleaf, r.slot, wleaf).backward(dy)

    def no_grad(f):
        def run():
            with torch.no_grad():
                f()
        return run

    row = 2 * DIM
    groups = {
        "route_fwd": ({"kgs": lambda: moe.moe_route(logits, k, cap),
                       "torch": no_grad(lambda: moe.ref_moe_route(logits, k, cap, dtype=torch.float32))},
                      TOKENS * num * 2 + TOKENS * k * 12 + num * cap * 4),
        "route_bwd": ({"kgs": lambda: moe.moe_route_backward(dw, r.weights, r.experts, num), "torch": torch_route_bwd},
                      TOKENS * k * 12 + TOKENS * num * 2),
        "dispatch_fwd": ({"kgs": lambda: moe.moe_gather(x, r.src, k),
                          "torch": lambda: x.index_select(0, rows) * (r.src >= 0)[:, None]},
                         (filled + num * cap) * row),
        "dispatch_bwd": ({"kgs": lambda: moe.moe_combine(dxe, r.slot),
                          "torch": lambda: _torch_combine(dxe, r.slot, ones)}, (filled + TOKENS) * row),
        "combine_fwd": ({"kgs": lambda: moe.moe_combine(ye, r.slot, r.weights),
                         "torch": no_grad(lambda: _torch_combine(ye, r.slot, r.weights))}, (filled + TOKENS) * row),
        "combine_bwd": ({"kgs": lambda: moe.moe_combine_backward(dy, ye, r.slot, r.src, r.weights),
                         "torch": torch_combine_bwd}, (2 * TOKENS + filled + num * cap) * row),
    }
    out = {"tokens": TOKENS, "dim": DIM, "experts": num, "top_k": k, "capacity": cap, "filled": filled,
           "dropped": TOKENS * k - filled, "rounds": rounds, "iters": iters}
    for what, (fns, nbytes) in groups.items():
        st = _alternate(fns, rounds, iters)
        out[what] = {**st, "bytes": nbytes, "kgs_gbps": round(nbytes / st["kgs"]["ms"] / 1e6, 1),
                     "speedup_vs_torch": round(st["torch"]["ms"] / st["kgs"]["ms"], 2)}
    return out


def _ffn_step(rounds, iters):
    import torch

    from kgs.models.moe import MoEFFN
    from kgs.ops import moe
    from kgs.ops.transformer import swiglu

    m = MoEFFN(DIM, FFN["inter"], FFN["experts"], FFN["top_k"], capacity_factor=FACTOR, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    h = torch.randn(TOKENS, DIM, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    dy = torch.randn(TOKENS, DIM, device="cuda", generator=gen).bfloat16()
    n, k, cap = m.num_experts, m.top_k, m.capacity(TOKENS)

    def torch_glue(hh):  # the module's forward with the routing in torch ops, the same GEMMs and SwiGLU
        route = moe.ref_moe_route(m.router(hh), k, cap, dtype=torch.float32)
        xe = moe.ref_moe_gather(hh, route.src, k)
        ye = torch.cat([b.down(swiglu(b.gate_up(xs))) for b, xs in zip(m.experts, xe.view(n, cap, DIM).unbind(0))])
        return moe.ref_moe_combine(ye, route.slot, route.weights, dtype=torch.float32).to(torch.bfloat16)

    def step(fwd):
        def run():
            h.grad = None
            for p in m.parameters():
                p.grad = None
            fwd(h).backward(dy)
        return run

    st = _alternate({"kgs": step(m), "torch_glue": step(torch_glue)}, rounds, iters)
    return {"moe_ffn_step": {**FFN, "tokens": TOKENS, "dim": DIM, "capacity": cap, **st,
                             "speedup_vs_torch_glue": round(st["torch_glue"]["ms"] / st["kgs"]["ms"], 2)}}


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-ffn", action="store_true", help="skip the MoEFFN step")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench needs a GPU")
    for num, k in CONFIGS:
        print(json.dumps(_routing(num, k, a.rounds, a.iters)), flush=True)
    if not a.no_ffn:
        print(json.dumps(_ffn_step(a.rounds, max(2, a.iters // 4))), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
