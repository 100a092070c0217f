"""Per-layer attention of a chunked-prefill step: the gather route against the
paged prefill kernel, same inputs, same process.

Parent route, as ``ServingModel.mixed`` runs it without ``paged_prefill``: per
chunk, ``gather_kv`` (the cached context copied out of the pages) then
``attention_chunk``; a first chunk (no cached context) is ``attention_qkv`` on
the fused rows, first chunks of equal padded length sharing a launch. New
route: one ``paged_prefill_attention`` launch for all chunks over the pages in
place (the plan is built once per step and is not in the timed region, as it
is shared by all layers).

Rounds interleave the routes (parent, gather alone, paged, parent, ...), each
round timing ``--iters`` back-to-back calls between two events; the figures are
medians over rounds, in microseconds per layer. One JSON document.

    python bench/paged_prefill_bench.py --out paged_prefill.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

H, HKV, HD, PAGE = 32, 8, 128, 32

# name -> chunks (n, ctx0); padded = n rounded up to 128
CASES = {
    "1x2048 ctx0": [(2048, 0)],
    "1x2048 ctx2048": [(2048, 2048)],
    "1x2048 ctx6144": [(2048, 6144)],
    "8x256 ctx512": [(256, 512)] * 8,
    "8 first chunks, mixed lengths": [(100, 0), (200, 0), (256, 0), (300, 0), (384, 0), (150, 0), (500, 0), (60, 0)],
}


def build(chunks, seed=0):
    """(qkv, cache layer, plan, parent-route chunk list): a cache holding every
    chunk's context and own rows (the own rows are the k / v of its qkv rows)."""
    from kgs.ops.decode import ref_cache_write
    from kgs.ops.transformer import paged_prefill_plan

    g = torch.Generator(device="cuda").manual_seed(seed)
    need = [-(-(ctx0 + n) // PAGE) for n, ctx0 in chunks]
    pages = sum(need) + 1
    perm = torch.randperm(pages - 1, generator=torch.Generator().manual_seed(seed)) + 1  # page 0: the null page
    width = max(need) + (max(need) & 1)
    table = torch.zeros((len(chunks), width), dtype=torch.int32)
    cache = torch.zeros((pages, HKV, 2, PAGE * HD), dtype=torch.bfloat16, device="cuda")
    rows = sum(-(-n // 128) * 128 for n, _ in chunks)
    qkv = torch.randn(rows, (H + 2 * HKV) * HD, device="cuda", generator=g).bfloat16()
    desc, row, used = [], 0, 0
    for ci, (n, ctx0) in enumerate(chunks):
        padded = -(-n // 128) * 128
        table[ci, :need[ci]] = perm[used:used + need[ci]].int()
        used += need[ci]
        k = torch.randn(ctx0 + n, HKV, HD, device="cuda", generator=g).bfloat16()
        v = torch.randn(ctx0 + n, HKV, HD, device="cuda", generator=g).bfloat16()
        k[ctx0:] = qkv[row:row + n, H * HD:(H + HKV) * HD].reshape(n, HKV, HD)
        v[ctx0:] = qkv[row:row + n, (H + HKV) * HD:].reshape(n, HKV, HD)
        pos = torch.arange(ctx0 + n)
        ref_cache_write(cache, k, v, (table[ci].long()[pos // PAGE] * PAGE + pos % PAGE).int().cuda())
        desc.append((row, n, padded, ctx0))
        row += padded
    plan = paged_prefill_plan(desc, table, "cuda")
    tbl = table.cuda()
    return qkv, cache, plan, [(*d, tbl[i]) for i, d in enumerate(desc)]


def parent_route(qkv, cache, chunks, out, gather_only=False):
    from kgs.ops.decode import gather_kv
    from kgs.ops.transformer import attention_chunk, attention_qkv

    j = 0
    while j < len(chunks):
        row0, n, p, ctx0, pages = chunks[j]
        k = j + 1
        if ctx0 == 0:
            while k < len(chunks) and chunks[k][3] == 0 and chunks[k][2] == p:
                k += 1
            if not gather_only:
                attention_qkv(qkv[row0:row0 + p * (k - j)], k - j, p, H, HKV, head_dim=HD, causal=True,
                              out=out[row0:row0 + p * (k - j)])
        else:
            kk, vv = gather_kv(cache, pages, ctx0 + n, rows=ctx0 + p)
            if not gather_only:
                attention_chunk(qkv[row0:row0 + p], kk, vv, H, HKV, HD, out=out[row0:row0 + p])
        j = k


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from kgs.ops.transformer import paged_prefill_attention

    res = []
    for name, chunks in CASES.items():
        qkv, cache, plan, pchunks = build(chunks)
        o_par = torch.zeros((qkv.shape[0], H * HD), dtype=torch.bfloat16, device="cuda")
        o_new = torch.zeros_like(o_par)
        routes = {
            "parent_us": lambda: parent_route(qkv, cache, pchunks, o_par),
            "gather_us": lambda: parent_route(qkv, cache, pchunks, o_par, gather_only=True),
            "paged_us": lambda: paged_prefill_attention(qkv, cache, plan, H, HKV, out=o_new),
        }
        for fn in routes.values():  # warm-up, and the two routes' outputs for the sanity check
            fn()
        routes["parent_us"]()
        torch.cuda.synchronize()
        err = 0.0
        for row0, n, _, _ in plan.chunks:
            d = (o_par[row0:row0 + n].float() - o_new[row0:row0 + n].float()).abs().max()
            err = max(err, (d / o_par[row0:row0 + n].float().abs().max()).item())
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        rec = {"case": name, "heads": H, "kv_heads": HKV, "chunks": [list(c) for c in chunks],
               "q_rows": int(qkv.shape[0]), "q_blocks": int(plan.qmap.shape[0]), "routes_max_rel_diff": round(err, 5)}
        rec.update({k: round(statistics.median(v), 1) for k, v in times.items()})
        rec["paged_over_parent"] = round(rec["paged_us"] / rec["parent_us"], 3)
        res.append(rec)
        print(json.dumps(rec), flush=True)
        del qkv, cache, plan, pchunks, o_par, o_new
        torch.cuda.empty_cache()
    doc = {"bench": "paged_prefill per-layer attention", "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "iters": a.iters, "cases": res}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
