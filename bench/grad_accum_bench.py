"""Gradient-accumulation timings on one MI355X: ``kgs.optim.AdamW(main_grads=True)``
against torch expressions of the same semantics, and its step against the
bf16-gradient step of the same build.

    python bench/grad_accum_bench.py [--rounds 7 --iters 5 --layers 4] [--only accumulate step]

The tensor set is bench/optimizer_bench.py's: Llama-3-8B's tensors with ``--layers``
layers (default 4) plus embedding and head, about 1.9 G elements.

* ``accumulate`` -- one ``accumulate()`` that adds (a later micro-batch of a cycle:
  2 B + 4 B read, 4 B + 2 B written per element, 12 B) and one that overwrites (the
  first micro-batch: 2 B read, 4 B + 2 B written, 8 B; the count word is reset by a
  one-element copy in front of the launch, inside the timed region), against two
  torch routes that leave fp32 sums of the bf16 gradients and zeroed gradients:
  ``torch._foreach_add_(mains, grads)`` + ``torch._foreach_zero_(grads)``, and the
  same per tensor (``a.add_(g); g.zero_()``).
* ``step`` -- the clipped step from main gradients (norm pass, finalize, update: 4 B
  + 16 B read, 14 B written per element, 34 B; the count word is set to 2 by a
  one-element copy in front, inside the timed region) against the clipped
  bf16-gradient step of the same optimizer class (2 B + 14 B read, 14 B written, 30 B);
  then each step's norm pass (with finalize) and update alone (``step_parts``).

The sides alternate inside every round (same process, device events after a
warm-up); medians and the min-max spread of the rounds are reported. ``tbps`` is
the traffic the operation needs over the time. Gaussian data.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from optimizer_bench import _alternate, _tbps, shapes  # noqa: E402  (this folder's: same tensor set, same timing)


def main(argv=None) -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7, help="interleaved timing rounds (medians reported)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--only", nargs="*", default=None, choices=["accumulate", "step"])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("grad_accum_bench needs a GPU")
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
    only = a.only or ["accumulate", "step"]
    opt = AdamW(weights, max_grad_norm=a.max_grad_norm, main_grads=True, **hyper)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    two = torch.full((1,), 2, dtype=torch.int32, device=dev)
    micro = opt._state[ops.STATE_MICRO:ops.STATE_MICRO + 1]

    if "accumulate" in only:
        mains = [torch.zeros(s, device=dev) for s in shp]

        def kgs_add():  # the count is > 0 after the first call: every timed call adds
            opt.accumulate()

        def kgs_first():
            micro.copy_(zero)
            opt.accumulate()

        def torch_foreach():
            with torch.no_grad():
                torch._foreach_add_(mains, grads)
                torch._foreach_zero_(grads)

        def torch_loop():
            with torch.no_grad():
                for m, g in zip(mains, grads):
                    m.add_(g)
                    g.zero_()

        opt.accumulate()
        st = _alternate({"kgs_add": kgs_add, "kgs_first": kgs_first, "torch_foreach": torch_foreach,
                         "torch_loop": torch_loop}, a.rounds, a.iters)
        best = min(("torch_foreach", "torch_loop"), key=lambda k: st[k]["ms"])
        print(json.dumps({"op": "accumulate", **info, **st, "bytes_per_element": 12,
                          "kgs_add_tbps": _tbps(12.0 * n, st["kgs_add"]),
                          "kgs_first_tbps": _tbps(8.0 * n, st["kgs_first"]),
                          "torch_foreach_tbps": _tbps(12.0 * n, st["torch_foreach"]),
                          "torch_loop_tbps": _tbps(12.0 * n, st["torch_loop"]), "torch_best": best,
                          "speedup": round(st[best]["ms"] / st["kgs_add"]["ms"], 3)}), flush=True)
        del mains
        torch.cuda.empty_cache()

    if "step" in only:
        for g in grads:  # the timed accumulates zeroed them
            g.copy_(0.01 * torch.randn(g.shape, device=dev))
        micro.copy_(zero)
        opt.accumulate(zero_grads=False)
        opt.accumulate(zero_grads=False)
        opt.step()  # builds the step's table; the main gradients stay as they are
        old = AdamW(weights, max_grad_norm=a.max_grad_norm, **hyper)

        def main_step():
            micro.copy_(two)
            ops.grad_norm(opt._main_live, opt._nchunks, opt._state, opt.betas, partials=opt._partials,
                          max_norm=a.max_grad_norm, main=True, average=True)
            ops.adamw_step_(opt._main_live, opt._nchunks, opt._groups, opt._state, opt.betas, opt.eps, main=True,
                            average=True)

        st = _alternate({"main": main_step, "bf16": old.step}, a.rounds, a.iters)
        torch.cuda.synchronize()
        print(json.dumps({"op": "step", **info, **st, "main_bytes_per_element": 34, "bf16_bytes_per_element": 30,
                          "main_tbps": _tbps(34.0 * n, st["main"]), "bf16_tbps": _tbps(30.0 * n, st["bf16"]),
                          "ratio": round(st["main"]["ms"] / st["bf16"]["ms"], 3), "steps": opt.step_count,
                          "skipped": opt.skipped_steps, "grad_norm": opt.grad_norm,
                          "bf16_grad_norm": old.grad_norm}), flush=True)

        # the two halves of each step alone: the state blocks hold an applied step's clip and count

        def main_norm():
            micro.copy_(two)
            ops.grad_norm(opt._main_live, opt._nchunks, opt._state, opt.betas, partials=opt._partials,
                          max_norm=a.max_grad_norm, main=True, average=True)

        def main_update():
            ops.adamw_step_(opt._main_live, opt._nchunks, opt._groups, opt._state, opt.betas, opt.eps, main=True,
                            average=True)

        def bf16_norm():
            ops.grad_norm(old._table, old._nchunks, old._state, old.betas, partials=old._partials,
                          max_norm=a.max_grad_norm)

        def bf16_update():
            ops.adamw_step_(old._table, old._nchunks, old._groups, old._state, old.betas, old.eps)

        main_step()
        st = _alternate({"main_norm": main_norm, "bf16_norm": bf16_norm}, a.rounds, a.iters)
        main_step()
        st.update(_alternate({"main_update": main_update, "bf16_update": bf16_update}, a.rounds, a.iters))
        print(json.dumps({"op": "step_parts", **info, **st,
                          "main_norm_tbps": _tbps(4.0 * n, st["main_norm"]),
                          "bf16_norm_tbps": _tbps(2.0 * n, st["bf16_norm"]),
                          "main_update_tbps": _tbps(30.0 * n, st["main_update"]),
                          "bf16_update_tbps": _tbps(28.0 * n, st["bf16_update"])}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
