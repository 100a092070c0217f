"""Per-step time of penalties and logprobs: the engine's per-request torch routes
against ``EngineConfig.device_logit_ops`` (``penalize_rows``, ``token_counts_add``,
``logprob_rows``), same logits, same process, ``device_sampler`` on both sides.

Both routes are the engine's own code: ``Sampler.sample``
(``kgs.serve.sampling``) on two samplers (no model, no scheduler) over the
step's requests, the flag differing. Off: the per-request penalties on the host,
the clone, ``sample_rows`` and the blocking ``log_softmax`` route. On: the three
launches around the sampler and ``logprob_rows``; each step then reads the
result of the step before, as overlapped engine steps do. Both end in the
read-back launch. So the figures include the host's share of both.

Rounds interleave the routes; each round times ``--iters`` back-to-back steps
with a host clock around work that ends in a device synchronise. Figures are
medians over rounds, microseconds per step. ``kernel_us``: each new kernel alone
between two device events on the parameters the route staged. Rows {1, 32, 256}
at vocabulary 128 256; every request has a 512-token prompt and 256 tokens of
output history. One JSON document.

    python bench/logit_ops_bench.py --out logit_ops.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path[:0] = [str(Path(__file__).resolve().parents[1]), str(Path(__file__).resolve().parent)]

from sampler_bench import ROWS, VOCAB, timed, timed_events  # noqa: E402

# name -> (rows with penalties, rows with logprobs): "all" or "one"
CASES = {"penalties, every row": ("all", None), "penalties, one row": ("one", None),
         "logprobs 5, every row": (None, "all"), "logprobs 5, one row": (None, "one"),
         "penalties + logprobs 5, every row": ("all", "all")}
HISTORY, PROMPT_LEN, TOP = 256, 512, 5


def sampler(rows: int, pen, lp, device_logit_ops: bool):
    """A Sampler over the requests of one step."""
    from kgs.serve.engine import EngineConfig, Request, SamplingParams
    from kgs.serve.sampling import Sampler

    requests = {}
    s = Sampler(EngineConfig(max_batch=max(ROWS), device_sampler=True, device_logit_ops=device_logit_ops), "cuda",
                "kgs", VOCAB, requests)
    rng = np.random.default_rng(rows)
    for rid in range(rows):
        kw = {}
        if pen == "all" or (pen == "one" and rid == 0):
            kw.update(frequency_penalty=0.5, presence_penalty=0.3, repetition_penalty=1.2)
        if lp == "all" or (lp == "one" and rid == 0):
            kw.update(logprobs=TOP)
        requests[rid] = Request(rid, rng.integers(3, VOCAB, PROMPT_LEN).tolist(), SamplingParams(temperature=0.8, **kw),
                                output=rng.integers(3, VOCAB, HISTORY).tolist())
        s.track(requests[rid])
    return s


def step_on(s, ids, logits, state):
    """One overlapped step: launch, then complete the step before."""
    prev, state["cur"] = state.get("cur"), s.sample(ids, logits)
    return prev.result() if prev is not None else None


def kernels_only(s, ids, logits, lp) -> dict:
    """Each new kernel alone on what the device route staged."""
    from kgs.ops.transformer import logprob_rows, penalize_rows, token_counts_add

    n, v = len(ids), s.params.dev
    out = {}
    toks = torch.zeros(n, dtype=torch.int64, device="cuda")
    if s.counts is not None:
        table, buf = s.counts.table, torch.empty_like(logits)
        out["penalize_rows"] = lambda: penalize_rows(logits, v["freq"][:n], v["pres"][:n], v["rep"][:n],
                                                     v["slot"][:n], table, out=buf)
        out["token_counts_add"] = lambda: token_counts_add(table, toks, v["slot"][:n])
    if lp is not None:
        lp, tv, ti = (s.lp.dev[k] for k in ("lp", "top_val", "top_idx"))
        out["logprob_rows"] = lambda: logprob_rows(logits, toks, v["want"][:n], lp[:n], tv[:n], ti[:n])
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=2.0, help="standard deviation of the random logits")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    res = []
    for rows in ROWS:
        logits = (torch.randn(rows, VOCAB, device="cuda", generator=torch.Generator(device="cuda").manual_seed(rows))
                  * a.scale).bfloat16()
        ids = np.arange(rows)
        for name, (pen, lp) in CASES.items():
            off, on = sampler(rows, pen, lp, False), sampler(rows, pen, lp, True)
            state = {}
            routes = {"off_us": lambda: off.sample(ids, logits), "on_us": lambda: step_on(on, ids, logits, state)}
            for fn in routes.values():  # warm-up: buffers, the count-table rows, code objects
                fn()
                fn()
            torch.cuda.synchronize()
            times = {r: [] for r in routes}
            for _ in range(a.rounds):
                for r, fn in routes.items():
                    times[r].append(timed(fn, a.iters))
            rec = {"rows": rows, "vocab": VOCAB, "case": name}
            rec.update({r: round(statistics.median(v), 1) for r, v in times.items()})
            rec.update({r.replace("_us", "_min_max_us"): [round(min(v), 1), round(max(v), 1)]
                        for r, v in times.items()})
            rec["on_over_off"] = round(rec["on_us"] / rec["off_us"], 4)
            rec["kernel_us"] = {k: round(statistics.median(timed_events(fn, a.iters) for _ in range(a.rounds)), 1)
                                for k, fn in kernels_only(on, ids, logits, lp).items()}
            res.append(rec)
            print(json.dumps(rec), flush=True)
            del off, on, state, routes
        del logits
        torch.cuda.empty_cache()
    doc = {"bench": "penalties and logprobs per step: device_logit_ops off vs on (device_sampler on both sides)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "logit_scale": a.scale,
           "history_tokens": HISTORY, "prompt_tokens": PROMPT_LEN, "cases": res}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
