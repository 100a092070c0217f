"""QK-norm + RoPE timings on one MI355X: ``kgs.ops.qknorm_rope``'s two kernels against
(a) the same step as a torch bf16 autograd composite and (b) the plain RoPE pair
they replace, ``rope_qkv_`` forward and its backward (a clone and the same kernel).

    python bench/qknorm_rope_bench.py [--rounds 7 --iters 40] [--sweep]

16384 tokens, 32 q heads, 8 k / v heads of 128: a fused row of 6144 bf16. One JSON
line: per direction the median and min-max of the rounds for each side, which
alternate inside every round (same process, same tensors, device events after a
warm-up), the bytes the direction must move and the rate that makes. Forward: the
q and k columns read once and written twice (the result, and the pre-norm copy the
backward needs). Backward: the ``dy`` row and the saved q and k columns in, the
``dx`` row out. The plain RoPE pair does less work (no norm, nothing saved, no
weight gradient) and moves fewer bytes; it is the yardstick for what a pass over
these rows costs, not an equal. ``--sweep`` times the two kernels over grid caps
(the default is the kernels' own).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENS, HEADS, KV_HEADS, SEQ, HD = 16384, 32, 8, 4096, 128


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


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sweep", action="store_true", help="also time the kernels over grid caps")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("qknorm_rope_bench needs a GPU")
    from kgs.ops.qknorm_rope import qknorm_rope_, qknorm_rope_backward, ref_qknorm_rope
    from kgs.ops.transformer import rope_qkv_, rope_tables

    gen = torch.Generator(device="cuda").manual_seed(0)
    nqk, width = (HEADS + KV_HEADS) * HD, (HEADS + 2 * KV_HEADS) * HD
    qkv0 = torch.randn(TOKENS, width, device="cuda", generator=gen).bfloat16()
    dy = torch.randn(TOKENS, width, device="cuda", generator=gen).bfloat16()
    wq, wk = ((1 + 0.1 * torch.randn(HD, device="cuda", generator=gen)).bfloat16() for _ in range(2))
    cos, sin = rope_tables(SEQ, HD, 10000.0, "cuda")
    buf, save = qkv0.clone(), torch.empty(TOKENS, nqk, dtype=torch.bfloat16, device="cuda")
    args = (wq, wk, cos, sin, HEADS, KV_HEADS, SEQ)
    qknorm_rope_(buf, *args, save=save)
    leaf = qkv0.clone().requires_grad_(True)
    lq, lk = wq.clone().requires_grad_(True), wk.clone().requires_grad_(True)

    def torch_fwd():  # the composite the torch glue runs: fp32 inside, bf16 in and out
        return ref_qknorm_rope(leaf, lq, lk, cos, sin, HEADS, KV_HEADS, SEQ, dtype=torch.float32).to(torch.bfloat16)

    def torch_step():
        leaf.grad = lq.grad = lk.grad = None
        torch_fwd().backward(dy)

    def torch_fwd_only():
        with torch.no_grad():
            torch_fwd()

    fns = {
        "fwd": {"kgs": lambda: qknorm_rope_(buf, *args, save=save), "torch": torch_fwd_only,
                "rope": lambda: rope_qkv_(buf, cos, sin, HEADS + KV_HEADS, HD, SEQ)},
        "step": {"kgs": lambda: (qknorm_rope_(buf, *args, save=save), qknorm_rope_backward(dy, save, *args)),
                 "torch": torch_step,
                 "rope": lambda: (rope_qkv_(buf, cos, sin, HEADS + KV_HEADS, HD, SEQ),
                                  rope_qkv_(dy.clone(), cos, -sin, HEADS + KV_HEADS, HD, SEQ))},
        "bwd": {"kgs": lambda: qknorm_rope_backward(dy, save, *args),
                "rope": lambda: rope_qkv_(dy.clone(), cos, -sin, HEADS + KV_HEADS, HD, SEQ)},
    }
    nbytes = {"fwd": 3 * TOKENS * nqk * 2, "bwd": (2 * TOKENS * width + TOKENS * nqk) * 2}
    nbytes["step"] = nbytes["fwd"] + nbytes["bwd"]
    rope_bytes = {"fwd": 2 * TOKENS * nqk * 2, "bwd": (2 * TOKENS * width + 2 * TOKENS * nqk) * 2}
    rope_bytes["step"] = rope_bytes["fwd"] + rope_bytes["bwd"]
    out = {"tokens": TOKENS, "heads": HEADS, "kv_heads": KV_HEADS, "rounds": a.rounds, "iters": a.iters}
    for what, group in fns.items():
        st = _alternate(group, a.rounds, a.iters)
        out[what] = {**st, "bytes": nbytes[what], "kgs_tbps": round(nbytes[what] / st["kgs"]["ms"] / 1e9, 3),
                     "rope_bytes": rope_bytes[what],
                     "rope_tbps": round(rope_bytes[what] / st["rope"]["ms"] / 1e9, 3)}
        if "torch" in st:
            out[what]["speedup_vs_torch"] = round(st["torch"]["ms"] / st["kgs"]["ms"], 2)
    print(json.dumps(out), flush=True)
    if a.sweep:
        caps = (512, 1024, 2048, 4096, 8192)
        sw = {"fwd": _alternate({str(c): (lambda c=c: qknorm_rope_(buf, *args, save=save, _wgs=c)) for c in caps},
                                a.rounds, a.iters),
              "bwd": _alternate({str(c): (lambda c=c: qknorm_rope_backward(dy, save, *args, _wgs=c)) for c in caps},
                                a.rounds, a.iters)}
        print(json.dumps({"sweep": sw}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
