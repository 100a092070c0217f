"""CPU tests of the mixture-of-experts routing (kgs/ops/moe.py, kgs/models/moe.py): the
float64 references against a per-token loop, the argument checks, the torch-backend
MoE layer, and the compile-time resources of native/kernels/moe_route.hip."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.ops import moe

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
SRC = ROOT / "native" / "kernels" / "moe_route.hip"


@pytest.mark.parametrize("k", [1, 3])
def test_references_against_a_per_token_loop(k):
    """T 12, E 8, C 2: drops occur, expert 5 is never chosen; forward and, through
    torch.autograd.grad on the loop, every backward, at 1e-9 in float64."""
    t, e, c, d = 12, 8, 2, 8
    g = torch.Generator().manual_seed(k)
    logits = ((torch.randn(t, e, generator=g) * 4).round() / 4).double()
    logits[:, 5] -= 50
    logits.requires_grad_(True)
    x = torch.randn(t, d, generator=g, dtype=torch.float64, requires_grad=True)
    ye = torch.randn(e * c, d, generator=g, dtype=torch.float64, requires_grad=True)
    dw_in, dy, dxe = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((t, k), (t, d), (e * c, d)))
    filled, experts, slot, weights = [0] * e, [], [], []
    xe_rows, src = [torch.zeros(d, dtype=torch.float64)] * (e * c), [-1] * (e * c)
    for ti in range(t):
        pick = sorted(range(e), key=lambda i: (-logits[ti, i].item(), i))[:k]
        weights.append(torch.softmax(logits[ti, pick], 0))
        experts.append(pick)
        slot.append([])
        for j, ex in enumerate(pick):
            s = ex * c + filled[ex] if filled[ex] < c else -1
            filled[ex] += 1
            slot[-1].append(s)
            if s >= 0:
                xe_rows[s], src[s] = x[ti], ti * k + j
    w_loop, xe_loop = torch.stack(weights), torch.stack(xe_rows)
    w_leaf = w_loop.detach().requires_grad_(True)
    y_loop = torch.stack([sum((w_leaf[ti, j] * ye[s] for j, s in enumerate(slot[ti]) if s >= 0), torch.zeros(d).double())
                          for ti in range(t)])
    assert max(filled) > c and filled[5] == 0

    r = moe.ref_moe_route(logits, k, c)
    assert r.experts.tolist() == experts and r.slot.tolist() == slot and r.src.tolist() == src
    assert r.counts.tolist() == filled and r.experts.dtype == r.slot.dtype == r.src.dtype == r.counts.dtype == torch.int32
    same = lambda a, b: torch.allclose(a, b, rtol=0, atol=1e-9)  # noqa: E731
    assert same(r.weights, w_loop)
    assert torch.equal(moe.ref_moe_gather(x, r.src, k), xe_loop)
    assert same(moe.ref_moe_combine(ye, r.slot, w_leaf), y_loop)
    (dl,) = torch.autograd.grad(w_loop, logits, dw_in)
    assert same(moe.ref_moe_route_backward(dw_in, w_loop.detach(), r.experts, e), dl)
    assert (dl[:, 5] == 0).all()
    (dx,) = torch.autograd.grad(xe_loop, x, dxe)
    assert same(moe.ref_moe_dispatch_backward(dxe, r.slot), dx)
    dye, dw = torch.autograd.grad(y_loop, (ye, w_leaf), dy, allow_unused=True)
    rdye, rdw = moe.ref_moe_combine_backward(dy, ye, r.slot, r.src, w_leaf.detach())
    assert same(rdye, dye) and same(rdw, torch.zeros_like(rdw) if dw is None else dw)
    assert (rdye[torch.tensor(src) < 0] == 0).all()


def test_bad_arguments_are_rejected_before_the_device_check():
    ok = torch.zeros(16, 8, dtype=torch.bfloat16)
    for fn in (moe.moe_route, moe.moe_router):
        with pytest.raises(ValueError, match="GPU"):
            fn(ok, 2, 4)
        for e in (12, 136):
            with pytest.raises(ValueError, match="multiple of 8"):
                fn(torch.zeros(16, e, dtype=torch.bfloat16), 2, 4)
        for k in (0, 9):
            with pytest.raises(ValueError, match="top_k"):
                fn(torch.zeros(16, 16, dtype=torch.bfloat16), k, 4)
        with pytest.raises(ValueError, match="top_k"):
            fn(ok, 9, 4)  # k > E
        with pytest.raises(ValueError, match="capacity"):
            fn(ok, 2, 0)
        with pytest.raises(TypeError):
            fn(ok.float(), 2, 4)
    r = moe.ref_moe_route(ok, 2, 4)
    route = moe.Route(r.weights.float(), r.experts, r.slot, r.src, r.counts)
    x, bad = torch.zeros(16, 24, dtype=torch.bfloat16), torch.zeros(16, 12, dtype=torch.bfloat16)
    ye = torch.zeros(32, 24, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        moe.moe_dispatch(x, route)
    with pytest.raises(ValueError, match="GPU"):
        moe.moe_combine(ye, route)
    with pytest.raises(ValueError, match="GPU"):
        moe.moe_combine_backward(x, ye, route.slot, route.src, route.weights)
    with pytest.raises(ValueError, match="GPU"):
        moe.moe_route_backward(route.weights, route.weights, route.experts, 8)
    with pytest.raises(ValueError, match="multiple of 8"):
        moe.moe_dispatch(bad, route)
    with pytest.raises(ValueError, match="multiple of 8"):
        moe.moe_combine(torch.zeros(32, 12, dtype=torch.bfloat16), route)
    with pytest.raises(ValueError, match="multiple of 8"):
        moe.moe_combine_backward(bad, torch.zeros(32, 12, dtype=torch.bfloat16), route.slot, route.src, route.weights)


def routing_input(t, dim, e, device):
    """Rows whose first ``e`` columns are a permutation of 0, 0.5, ..: with the router
    weight ``[I | 0]`` the logits are those columns exactly, in bf16 and in fp32."""
    g = torch.Generator().manual_seed(5)
    h = torch.randn(t, dim, generator=g)
    h[:, :e] = torch.stack([torch.randperm(e, generator=g) for _ in range(t)]) * 0.5
    return h.bfloat16().to(device)


def test_torch_backend_layer_and_the_dense_layers_names():
    from kgs.models.decoder import DecoderLayer
    from kgs.models.moe import MoEFFN

    layer = DecoderLayer(64, 2, 1, 48, backend="torch", dtype=torch.float32, experts=4, top_k=2)
    x = torch.randn(2, 16, 64, requires_grad=True)
    res, delta = layer(x)
    (res + delta).pow(2).mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.parameters())
    assert x.grad.abs().sum() > 0 and layer.moe.router.weight.grad.abs().sum() > 0
    assert int(layer.moe.last_counts.sum()) == 2 * 32 and layer.moe.capacity(32) == 256
    dense = DecoderLayer(64, 2, 1, 48, backend="torch", experts=0)
    assert [n for n, _ in dense.named_parameters()] == ["attn_norm", "mlp_norm", "qkv.weight", "o.weight",
                                                        "gate_up.weight", "down.weight"]
    # the input of the GPU gradient test routes identically in bf16 and in fp32
    counts = []
    for dtype in (torch.bfloat16, torch.float32):
        m = MoEFFN(512, 64, 8, backend="torch", dtype=dtype)
        with torch.no_grad():
            m.router.weight.copy_(torch.eye(8, 512))
            m(routing_input(512, 512, 8, "cpu").to(dtype))
        counts.append(m.last_counts)
    assert torch.equal(*counts) and int(counts[0].sum()) == 1024


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_kernels_have_no_spills_and_no_scratch(tmp_path):
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(SRC.parent), str(SRC), "-o", str(tmp_path / "moe_route.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=800, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"\s([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+) \[-Rpass", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    for short in ("moe_select", "moe_hist", "moe_scan", "moe_slots", "moe_gather", "moe_combine", "moe_dw",
                  "moe_route_bwd"):
        (r,) = [r for n, r in res.items() if re.search(rf"3moe\d+{short}E", n)]
        print(short, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (short, r)
