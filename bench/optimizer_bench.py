"""Optimizer-step timings on one MI355X: ``kgs.optim.AdamW`` (fp32 masters, clipped,
three launches) against the torch route with the same semantics.

    python bench/optimizer_bench.py [--rounds 7 --iters 5 --layers 4] [--only step variants]

The tensor set is Llama-3-8B's: per layer qkv 6144 x 4096, o 4096 x 4096, gate|up
28672 x 4096, down 4096 x 14336 and two 4096 norms; ``--layers`` of them (default 4)
plus embedding and head at 128256 x 4096, about 1.9 G elements.

* ``step``     -- one ``AdamW.step()`` with ``max_grad_norm`` against: bf16 gradients
  cast to fp32 (``_foreach_copy_``), ``clip_grad_norm_(foreach=True)``,
  ``torch.optim.AdamW(fused=True)`` on fp32 masters, ``_foreach_copy_`` back to the
  bf16 weights. Also ``AdamW.step()`` without clipping (two launches).
* ``variants`` -- the update kernel alone and the norm pass alone in each streaming
  variant (plain or non-temporal accesses, one or two 16-byte groups per thread and
  trip, non-temporal loads or stores only): the A/B behind the library's defaults.

The sides alternate inside every round (same process, device events after a
warm-up); medians and the min-max spread of the rounds are reported. ``tbps`` is
the traffic the step needs over the time: per element 14 B read and 14 B written
by the update (bf16 gradient, fp32 p, m, v in; p, m, v, bf16 weight out) plus 2 B
for the norm pass, 30 B with clipping and 28 B without. Gaussian data.
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


def shapes(layers: int) -> list[tuple[int, ...]]:
    per_layer = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (4096,), (4096,)]
    return [(128256, 4096)] + per_layer * layers + [(4096,), (128256, 4096)]


def _tbps(nbytes: float, st: dict) -> float:
    return round(nbytes / st["ms"] / 1e9, 3)


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--only", nargs="*", default=None, choices=["step", "variants"])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench needs a GPU")
    from kgs.ops import optim as ops
    from kgs.optim import AdamW

    torch.manual_seed(0)
    dev = "cuda"
    shp = shapes(a.layers)
    weights = [(0.02 * torch.randn(s, device=dev)).bfloat16().requires_grad_(True) for s in shp]
    grads = [(0.01 * torch.randn(s, device=dev)).bfloat16() for s in shp]
    n = sum(w.numel() for w in weights)
    for w, g in zip(weights, grads):
        w.grad = g
    hyper = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    info = {"tensors": len(shp), "elements": n, "layers": a.layers, "rounds": a.rounds, "iters": a.iters,
            "chunk": ops.adamw_chunk()}
    only = a.only or ["step", "variants"]

    if "step" in only:
        clipped = AdamW(weights, max_grad_norm=a.max_grad_norm, **hyper)
        # the torch route: fp32 masters that own fp32 gradients, the bf16 weights written back
        w16 = [w.detach().clone() for w in weights]
        masters = [w.detach().float().requires_grad_(True) for w in weights]
        for m in masters:
            m.grad = torch.empty_like(m)
        g32 = [m.grad for m in masters]
        with torch.no_grad():
            torch._foreach_copy_(g32, grads)
        try:
            topt, impl = torch.optim.AdamW(masters, fused=True, **hyper), "fused"
            topt.step()
        except RuntimeError as e:  # said in the result line, not hidden
            topt, impl = torch.optim.AdamW(masters, foreach=True, **hyper), f"foreach ({str(e).splitlines()[0]})"
        # both sides start from the same state again
        with torch.no_grad():
            torch._foreach_copy_(masters, w16)
        topt.state.clear()

        def kgs_step():
            clipped.step()

        def torch_step():
            with torch.no_grad():
                torch._foreach_copy_(g32, grads)
                torch.nn.utils.clip_grad_norm_(masters, a.max_grad_norm, foreach=True)
                topt.step()
                torch._foreach_copy_(w16, masters)

        st = _alternate({"kgs": kgs_step, "torch": torch_step}, a.rounds, a.iters)
        torch.cuda.synchronize()
        # same gradients, same number of steps on both sides: how far apart the masters are
        diff = max(((clipped.state[w]["master"] - m.detach()).abs().max() / m.detach().abs().max()).item()
                   for w, m in zip(weights, masters))
        spread = max((s["max"] - s["min"]) / s["ms"] for s in st.values())
        print(json.dumps({"op": "step", **info, "kgs": st["kgs"], "torch": st["torch"], "torch_impl": impl,
                          "bytes_per_element": 30, "kgs_tbps": _tbps(30.0 * n, st["kgs"]),
                          "torch_tbps": _tbps(30.0 * n, st["torch"]),
                          "speedup": round(st["torch"]["ms"] / st["kgs"]["ms"], 3), "spread": round(spread, 4),
                          "steps": clipped.step_count, "skipped": clipped.skipped_steps,
                          "grad_norm": clipped.grad_norm, "master_rel_diff": diff}), flush=True)
        del topt, masters, g32, w16
        torch.cuda.empty_cache()
        plain = AdamW(weights, **hyper)
        st = _alternate({"kgs": plain.step}, a.rounds, a.iters)
        print(json.dumps({"op": "step_noclip", **info, "kgs": st["kgs"], "bytes_per_element": 28,
                          "kgs_tbps": _tbps(28.0 * n, st["kgs"])}), flush=True)
        del plain, clipped
        torch.cuda.empty_cache()

    if "variants" in only:
        opt = AdamW(weights, max_grad_norm=a.max_grad_norm, **hyper)
        opt.step()  # builds the table, the group block and a state with clip and bias corrections
        tbl, nch = opt._table, opt._nchunks

        def upd(v):
            return lambda: ops.adamw_step_(tbl, nch, opt._groups, opt._state, opt.betas, opt.eps, variant=v)

        def norm(v):
            return lambda: ops.grad_norm(tbl, nch, opt._state, opt.betas, partials=opt._partials,
                                         max_norm=a.max_grad_norm, variant=v)

        names = {0: "plain", 1: "nt", 2: "plain_x2", 3: "nt_x2", 4: "ntload_x2", 5: "ntstore_x2"}
        st = _alternate({f"update_{names[v]}": upd(v) for v in names}, a.rounds, a.iters)
        for k, s in st.items():
            print(json.dumps({"op": k, **info, "kgs": s, "bytes_per_element": 28, "kgs_tbps": _tbps(28.0 * n, s)}),
                  flush=True)
        st = _alternate({f"norm_{names[v]}": norm(v) for v in (0, 1)}, a.rounds, a.iters)
        for k, s in st.items():
            print(json.dumps({"op": k, **info, "kgs": s, "bytes_per_element": 2, "kgs_tbps": _tbps(2.0 * n, s)}),
                  flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
