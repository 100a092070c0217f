"""Per-step time of penalties and logprobs: the engine's per-request torch routes
against ``EngineConfig.device_logit_ops`` (``penalize_rows``, ``token_counts_add``,
``logprob_rows``), same logits, same process, ``device_sampler`` on both sides.

Both routes are the engine's own code on a bare engine object (no model, no
scheduler) holding the step's requests. Off: ``_sample`` (``_penalized_rows``, the
clone, ``sample_rows``) then the blocking ``_logprobs``. On: ``_sample`` (the three
launches around the sampler), ``_logprobs_device`` and the read-back launch; each
step then turns the step before's pinned results into tuples, as overlapped
engine steps do. So the figures include the host's share of both.

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


def bare_engine(rows: int, pen, lp, device_logit_ops: bool):
    """An LLMEngine with just what the sampling and logprob steps read."""
    from kgs.serve.engine import EngineConfig, LLMEngine, Request, SamplingParams

    eng = object.__new__(LLMEngine)
    eng.cfg = EngineConfig(max_batch=max(ROWS), device_sampler=True, device_logit_ops=device_logit_ops)
    eng.device, eng.backend = torch.device("cuda"), "kgs"
    eng.device_sampler, eng._draw = True, None
    eng.device_logit_ops, eng._lp_big = device_logit_ops, set()
    eng._want_pen, eng._seeded, eng._want_lp = set(), set(), set()
    eng._pinned, eng._flip = None, 0
    eng.requests = {}
    rng = np.random.default_rng(rows)
    for rid in range(rows):
        kw = {}
        if pen == "all" or (pen == "one" and rid == 0):
            kw.update(frequency_penalty=0.5, presence_penalty=0.3, repetition_penalty=1.2)
            eng._want_pen.add(rid)
        if lp == "all" or (lp == "one" and rid == 0):
            kw.update(logprobs=TOP)
            eng._want_lp.add(rid)
        p = SamplingParams(temperature=0.8, **kw)
        eng.requests[rid] = Request(rid, rng.integers(3, VOCAB, PROMPT_LEN).tolist(), p,
                                    output=rng.integers(3, VOCAB, HISTORY).tolist(), draw=(0.8, 0, 1.0, rid + 1))
    return eng


def step_off(eng, ids, logits):
    toks = eng._sample(ids, logits)
    return toks, eng._logprobs(ids, logits, toks)


def step_on(eng, ids, logits, state):
    """One overlapped step: launch, then complete the step before."""
    toks = eng._sample(ids, logits)
    cur = eng._launch_readback(ids, toks, 0, eng._logprobs_device(ids, logits, toks))
    prev, state["cur"] = state.get("cur"), cur
    lps = None
    if prev is not None:
        prev["event"].synchronize()
        if prev["lp_host"] is not None:
            lps = eng._lp_tuples(prev["lp_rows"], prev["lp_host"].numpy())
    return toks, lps


def kernels_only(eng, ids, logits) -> dict:
    """Each new kernel alone on what the device route staged."""
    from kgs.ops.transformer import logprob_rows, penalize_rows, token_counts_add

    n, v = len(ids), eng._draw["views"]
    out = {}
    toks = torch.zeros(n, dtype=torch.int64, device="cuda")
    if eng._counts is not None:
        table, buf = eng._counts.table, eng._pen_buf[:n]
        out["penalize_rows"] = lambda: penalize_rows(logits, v["freq"][:n], v["pres"][:n], v["rep"][:n],
                                                     v["slot"][:n], table, out=buf)
        out["token_counts_add"] = lambda: token_counts_add(table, toks, v["slot"][:n])
    if eng._lp is not None:
        lp, tv, ti = eng._lp_views(eng._lp["dev"])
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
            off, on = bare_engine(rows, pen, lp, False), bare_engine(rows, pen, lp, True)
            state = {}
            routes = {"off_us": lambda: step_off(off, ids, logits), "on_us": lambda: step_on(on, ids, logits, state)}
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
                                for k, fn in kernels_only(on, ids, logits).items()}
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
