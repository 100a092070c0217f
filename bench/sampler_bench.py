"""Per-step sampler time: the engine's torch route against the device sampler
(``sample_rows``), same logits, same process.

Both routes are the engine's own code: ``Sampler.sample``
(``kgs.serve.sampling``) is called on a sampler (no model, no scheduler) over
the step's requests, once with ``device_sampler`` off (the chain of torch ops:
cast, divide, topk, sort, softmax, cumsum, scatter, multinomial, where) and
once with it on (the packed parameter buffer, one copy, one launch); either
ends in the launch of the tokens' read-back. So the figures include the host's
share: the small tensors the torch route builds from Python lists, the
parameter staging of the device route.

Rounds interleave the routes; each round times ``--iters`` back-to-back calls
with a host clock around work that ends in a device synchronise. Figures are
medians over rounds, microseconds per step. ``kernel_us`` is ``sample_rows`` alone
between two device events (the GPU's share of ``device_us``; at one row the
host's validation and launch can outlast the kernel). Rows {1, 32, 256} at vocabulary
128 256; cases: temperature only, top-k 50, top-p 0.9, both, and a batch whose
other half is greedy. One JSON document.

    python bench/sampler_bench.py --out sampler.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

VOCAB = 128256
ROWS = (1, 32, 256)
# name -> (top_k, top_p, every other row greedy)
CASES = {"temperature": (0, 1.0, False), "top_k 50": (50, 1.0, False), "top_p 0.9": (0, 0.9, False),
         "top_k 50 + top_p 0.9": (50, 0.9, False), "top_p 0.9, half greedy": (0, 0.9, True)}


def sampler(rows: int, top_k: int, top_p: float, half_greedy: bool, device_sampler: bool, temperature=0.8):
    """A Sampler over the requests of one step."""
    from kgs.serve.engine import EngineConfig, Request, SamplingParams
    from kgs.serve.sampling import Sampler

    requests = {}
    s = Sampler(EngineConfig(max_batch=max(ROWS), device_sampler=device_sampler), "cuda", "kgs", VOCAB, requests)
    for rid in range(rows):
        greedy = half_greedy and rid % 2 == 1
        p = SamplingParams(temperature=0.0 if greedy else temperature, top_k=top_k, top_p=top_p)
        requests[rid] = Request(rid, [1], p)
        s.track(requests[rid])
    return s


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def timed_events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def kernel_only(s, ids, logits):
    """sample_rows alone on the parameters the device route staged (device events
    around back-to-back launches): the GPU's share of device_us."""
    from kgs.ops.transformer import sample_rows

    n, v = len(ids), s.params.dev
    args = [v[k][:n] for k in ("temperature", "top_k", "top_p", "seed", "counter")]
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    return lambda: sample_rows(logits, *args, out=out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=2.0, help="standard deviation of the random logits")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np

    res = []
    for rows in ROWS:
        logits = (torch.randn(rows, VOCAB, device="cuda", generator=torch.Generator(device="cuda").manual_seed(rows))
                  * a.scale).bfloat16()
        ids = np.arange(rows)
        for name, (k, p, half) in CASES.items():
            engs = {"torch_us": sampler(rows, k, p, half, False), "device_us": sampler(rows, k, p, half, True)}
            routes = {r: (lambda e=e: e.sample(ids, logits).tokens) for r, e in engs.items()}
            toks = {r: fn() for r, fn in routes.items()}  # warm-up
            torch.cuda.synchronize()
            assert all(((t >= 0) & (t < VOCAB)).all() for t in toks.values())
            if half:  # the greedy rows of both routes are the same argmax
                assert torch.equal(toks["torch_us"][1::2], toks["device_us"][1::2])
            routes["kernel_us"] = kernel_only(engs["device_us"], ids, logits)
            times = {r: [] for r in routes}
            for _ in range(a.rounds):
                for r, fn in routes.items():
                    times[r].append((timed_events if r == "kernel_us" else timed)(fn, a.iters))
            rec = {"rows": rows, "vocab": VOCAB, "case": name}
            rec.update({r: round(statistics.median(v), 1) for r, v in times.items()})
            rec.update({r.replace("_us", "_min_max_us"): [round(min(v), 1), round(max(v), 1)]
                        for r, v in times.items()})
            rec["device_over_torch"] = round(rec["device_us"] / rec["torch_us"], 4)
            res.append(rec)
            print(json.dumps(rec), flush=True)
        del logits
        torch.cuda.empty_cache()
    doc = {"bench": "sampler per step: Sampler.sample, torch route vs device_sampler",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "logit_scale": a.scale,
           "cases": res}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
