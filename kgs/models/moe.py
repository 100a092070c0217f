"""A trainable mixture-of-experts FFN (Mixtral, Qwen3-MoE, gpt-oss) on fixed-capacity
slabs: ``router Linear -> top-k route -> dispatch -> per-expert SwiGLU FFN -> combine``.

Every expert owns ``capacity`` rows of the dispatched matrix, so all shapes are
static: the expert FFNs are the ordinary Linears on row slices, and a token that
finds its expert full is dropped from that expert (its other picks still count).
``capacity = ceil(capacity_factor * T * top_k / experts)`` rounded up to a multiple
of 256, the GEMM tile. ``backend="kgs"``: :class:`kgs.ops.Linear` for the router and
the experts, :func:`kgs.ops.swiglu`, and the routing kernels of
``native/kernels/moe_route.hip`` through :func:`kgs.ops.moe_router`,
:func:`kgs.ops.moe_dispatch` and :func:`kgs.ops.moe_combine`. ``backend="torch"`` is the
same module on ``nn.Linear`` and the ``ref_moe_*`` formulas (weights and the combine's
sum in fp32 or wider, results in the module's dtype), on any device. Both start
from the same seeded weights. ``expert_gemm="batched"`` (kgs backend; ``dim`` and ``inter``
multiples of 128) runs all experts' FFNs as two :func:`kgs.ops.moe_linear` around one
:func:`kgs.ops.swiglu` -- three launches forward whatever E, empty slab rows skipped -- on
weights that are views of two stacked buffers: same parameter names, same seeded values, but
``Module.to`` restacks them; ``load_state_dict(assign=True)`` does not (``moe_linear`` then raises). The default
``"loop"`` is one Linear pair per expert; the torch backend accepts the option and ignores it.
There is no auxiliary load-balancing loss;
``last_counts`` holds the latest ``counts`` tensor (tokens per expert before
dropping), never read back by the module itself.
"""
from __future__ import annotations

import math

import torch

from .decoder import _torch_swiglu

TILE = 256


def slab_capacity(tokens: int, top_k: int, experts: int, capacity_factor: float) -> int:
    """Rows per expert: ``capacity_factor`` times the even share, rounded up to a multiple of TILE."""
    c = math.ceil(capacity_factor * tokens * top_k / experts)
    return (max(c, 1) + TILE - 1) // TILE * TILE


class _ExpertFFN(torch.nn.Module):
    def __init__(self, lin, dim: int, inter: int):
        super().__init__()
        self.gate_up, self.down = lin(dim, 2 * inter), lin(inter, dim)


class MoEFFN(torch.nn.Module):
    def __init__(self, dim: int, inter: int, experts: int, top_k: int = 2, capacity_factor: float = 1.25,
                 backend: str = "kgs", device=None, dtype=torch.bfloat16, seed: int = 0, expert_gemm: str = "loop"):
        super().__init__()
        if backend not in ("kgs", "torch"):
            raise ValueError(f"backend must be 'kgs' or 'torch', not {backend!r}")
        if expert_gemm not in ("loop", "batched"):
            raise ValueError(f"expert_gemm must be 'loop' or 'batched', not {expert_gemm!r}")
        if expert_gemm == "batched" and backend == "kgs" and (dim % 128 or inter % 128):
            raise ValueError("expert_gemm='batched' takes dim and inter multiples of 128")
        if experts < 1 or not 1 <= top_k <= experts:
            raise ValueError(f"experts must be at least 1 and top_k in 1 .. experts, got {experts}, {top_k}")
        if backend == "kgs" and (experts % 8 or not 8 <= experts <= 128 or top_k > 8):
            raise ValueError("the kgs backend takes experts a multiple of 8 in 8 .. 128 and top_k up to 8")
        if capacity_factor <= 0:
            raise ValueError("capacity_factor must be positive")
        if backend == "kgs" and (dtype != torch.bfloat16 or dim % 8 or inter % 8):
            raise ValueError("the kgs backend takes bf16 and dim, inter multiples of 8")
        self.dim, self.inter, self.num_experts, self.top_k = dim, inter, experts, top_k
        self.capacity_factor, self.backend, self.expert_gemm = capacity_factor, backend, expert_gemm
        if backend == "kgs":
            from kgs.ops.gemm import Linear

            def lin(i, o):
                return Linear(i, o, bias=False, device=device)
        else:
            def lin(i, o):
                return torch.nn.Linear(i, o, bias=False, device=device, dtype=dtype)
        self.router = lin(dim, experts)
        self.experts = torch.nn.ModuleList(_ExpertFFN(lin, dim, inter) for _ in range(experts))
        g = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():  # identical init for both backends
            for m in (self.router, *(m for blk in self.experts for m in (blk.gate_up, blk.down))):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * m.weight.shape[1] ** -0.5)
        self._restack()
        self.last_counts = None

    def _restack(self) -> None:
        """"batched" on the kgs backend: every expert's weight views its slice of one [E, out, in]
        buffer per projection. The same Parameters with the same values, names, order and count."""
        if self.backend != "kgs" or self.expert_gemm != "batched":
            return
        for name in ("gate_up", "down"):
            ws = [getattr(blk, name).weight for blk in self.experts]
            for w, s in zip(ws, torch.stack([w.detach() for w in ws]).unbind(0)):
                w.data = s

    def _apply(self, fn, *args, **kwargs):
        # Module.to and the dtype casts replace every Parameter's data one by one: stack them again
        super()._apply(fn, *args, **kwargs)
        self._restack()
        return self

    def capacity(self, tokens: int) -> int:
        return slab_capacity(tokens, self.top_k, self.num_experts, self.capacity_factor)

    def forward(self, h: torch.Tensor) -> torch.Tensor:
        """``h``: ``[..., dim]`` -> the same shape."""
        shp = h.shape
        h2 = h.reshape(-1, self.dim)
        n, cap = self.num_experts, self.capacity(h2.shape[0])
        logits = self.router(h2)
        if self.backend == "kgs":
            from kgs.ops.moe import moe_combine, moe_dispatch, moe_router
            from kgs.ops.transformer import swiglu

            route = moe_router(logits, self.top_k, cap)
            xe = moe_dispatch(h2, route)
            if self.expert_gemm == "batched":
                from kgs.ops.moe import moe_linear

                gu = moe_linear(xe, [blk.gate_up.weight for blk in self.experts], route.counts)
                ye = moe_linear(swiglu(gu), [blk.down.weight for blk in self.experts], route.counts)
            else:
                ye = torch.cat([blk.down(swiglu(blk.gate_up(xs)))
                                for blk, xs in zip(self.experts, xe.view(n, cap, self.dim).unbind(0))])
            y = moe_combine(ye, route)
        else:
            from kgs.ops.moe import ref_moe_combine, ref_moe_gather, ref_moe_route

            up = torch.promote_types(h2.dtype, torch.float32)
            route = ref_moe_route(logits, self.top_k, cap, dtype=up)
            xe = ref_moe_gather(h2, route.src, self.top_k)
            ye = torch.cat([blk.down(_torch_swiglu(blk.gate_up(xs)))
                            for blk, xs in zip(self.experts, xe.view(n, cap, self.dim).unbind(0))])
            y = ref_moe_combine(ye, route.slot, route.weights, dtype=up).to(h2.dtype)
        self.last_counts = route.counts
        return y.reshape(shp)
