"""Token-embedding timings on one MI355X: ``kgs.ops.embedding`` against
``torch.nn.functional.embedding`` with bf16 autograd and a dense gradient.

    python bench/embedding_bench.py [--rounds 7 --iters 10] [--only uniform zipf same]

16384 tokens x 4096 columns, vocabulary 128256, three token distributions:

* ``uniform`` -- every id equally likely: almost every run has length 0 or 1
* ``zipf``    -- P(id = k) ~ 1 / (k + 1) (exponent 1): the small ids come in runs of
  hundreds to a thousand rows
* ``same``    -- every token the same id: one run of 16384 rows. Reported, not
  compared: it shows what a long run costs next to the length-1 runs above

One JSON line per distribution. ``step`` is forward + backward through autograd
(the table's ``.grad`` reset to ``None`` first, so both sides write a fresh dense
gradient); ``fwd`` and ``bwd`` are the two raw ops alone (for kgs the backward
includes its device sort; for torch it is ``aten.embedding_dense_backward``). The
two sides alternate inside every round (same process, same tensors, device events
after a warm-up); medians and the min-max spread of the rounds are reported.
``gbps`` is the traffic the op must move over the time: ``2 T dim 2`` bytes
forward (read the rows, write them), ``T dim 2 + vocab dim 2`` backward (read dy,
write the dense dw).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENS, DIM, VOCAB = 16384, 4096, 128256


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


def tokens(dist: str, gen):
    import torch

    if dist == "uniform":
        return torch.randint(0, VOCAB, (TOKENS,), device="cuda", generator=gen)
    if dist == "zipf":
        u = torch.rand(TOKENS, device="cuda", generator=gen, dtype=torch.float64)
        span = torch.log(torch.tensor(VOCAB + 1.0, dtype=torch.float64))
        return (torch.exp(u * span) - 1).long().clamp_(0, VOCAB - 1)
    return torch.full((TOKENS,), 1234, device="cuda")


def bench(dist: str, w, dy, a, gen) -> None:
    import torch

    from kgs.ops.embedding import embedding, embedding_rows, embedding_rows_backward

    tok = tokens(dist, gen)
    runs = torch.bincount(tok, minlength=VOCAB)
    dense = torch.ops.aten.embedding_dense_backward

    def kgs_step():
        w.grad = None
        embedding(w, tok).backward(dy)

    def torch_step():
        w.grad = None
        torch.nn.functional.embedding(tok, w).backward(dy)

    wd = w.detach()
    fns = {"step": {"kgs": kgs_step, "torch": torch_step},
           "fwd": {"kgs": lambda: embedding_rows(wd, tok), "torch": lambda: torch.nn.functional.embedding(tok, wd)},
           "bwd": {"kgs": lambda: embedding_rows_backward(dy, tok, VOCAB),
                   "torch": lambda: dense(dy, tok, VOCAB, -1, False)}}
    nbytes = {"fwd": 2 * TOKENS * DIM * 2, "bwd": TOKENS * DIM * 2 + VOCAB * DIM * 2}
    nbytes["step"] = nbytes["fwd"] + nbytes["bwd"]
    out = {"dist": dist, "tokens": TOKENS, "dim": DIM, "vocab": VOCAB, "rounds": a.rounds,
           "rows_used": int((runs > 0).sum()), "longest_run": int(runs.max())}
    for what, pair in fns.items():
        st = _alternate(pair, a.rounds, a.iters)
        k, r = st["kgs"], st["torch"]
        out[what] = {"kgs": k, "torch": r, "bytes": nbytes[what],
                     "kgs_gbps": round(nbytes[what] / k["ms"] / 1e6, 1),
                     "torch_gbps": round(nbytes[what] / r["ms"] / 1e6, 1), "speedup": round(r["ms"] / k["ms"], 3),
                     "spread": round(max((s["max"] - s["min"]) / s["ms"] for s in (k, r)), 4)}
    # the two dense gradients: bit-equal or not, and how far apart
    kgs_step()
    gk = w.grad
    torch_step()
    diff = (gk.float() - w.grad.float()).abs().max().item()
    out["grad_max_abs_diff_vs_torch"] = diff
    w.grad = None
    print(json.dumps(out), flush=True)


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None, choices=["uniform", "zipf", "same"])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("embedding_bench needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(VOCAB, DIM, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    dy = torch.randn(TOKENS, DIM, device="cuda", generator=gen).bfloat16()
    for dist in a.only or ["uniform", "zipf", "same"]:
        bench(dist, w, dy, a, gen)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
