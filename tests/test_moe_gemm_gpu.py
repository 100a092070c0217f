"""GPU tests of the batched expert GEMM (native/kernels/moe_gemm.hip) against the float64 reference
of kgs/ops/moe.py. The per-element bound against the float64 product of the bf16 inputs is
``2^-8 |ref| + K 2^-23 (|A| |B|^T)``: one bf16 rounding plus a loose fp32 accumulation term."""
import pytest
import torch

from forward_refs import POISON
from kgs.ops import moe
from test_moe import routing_input

pytestmark = pytest.mark.gpu

DEV, NUM, M, NAN = "cuda", 5, 256, float("nan")
COUNTS = [0, 1, 129, 256, 300]
# (M, tile, counts): 2 to 4 tile rows on either kernel but for the first; counts inside the first tile and a later one
SLABS = [(256, -1, COUNTS), (256, 0, COUNTS), (384, -1, [0, 1, 129, 257, 384, 500]),
         (512, -1, [0, 1, 129, 257, 512, 600]), (512, 0, [0, 1, 129, 257, 512, 600])]


def _wide(shape, gen=None, fill=POISON):  # a column block of a wider, taller poisoned buffer: (view, buffer)
    num, rows, cols = shape
    buf = torch.full((num, rows + 2, cols + 64), fill, dtype=torch.bfloat16, device=DEV)
    view = buf[:, :rows, 8:8 + cols]
    if gen is not None:
        view.copy_(torch.randn(shape, device=DEV, generator=gen))
    return view, buf


def _check(out, ref, mag, k, what):
    err = (out.double() - ref).abs()
    slack = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * mag - err
    print(f"{what}: max err {err.max().item():.3e}, least margin {slack.min().item():.3e}")
    assert torch.isfinite(out.float()).all() and slack.min().item() >= 0, (what, err.max().item())


@pytest.mark.parametrize("m,tile,cs,mode,n,k", [(*s, mode, n, k) for s in SLABS for mode in (None, "rows")
                                                for n in (128, 256) for k in (64, 128, 192)] +
                         [(*s, "reduce", n, 256) for s in SLABS[:2] for n in (128, 256)])
def test_raw_entry_against_the_reference(m, tile, cs, mode, n, k):
    g = torch.Generator(device=DEV).manual_seed(n + k)
    (a, _), (b, _) = _wide((len(cs), m, k), g), _wide((len(cs), n, k), g)
    out, buf = _wide((len(cs), m, n))
    counts = None if mode is None else torch.tensor(cs, dtype=torch.int32, device=DEV)
    for e, c in enumerate(cs):
        if mode == "rows":
            a[e, c:] = NAN
        if mode == "reduce":
            for t in (a, b):
                t[e, :, min(c, k):] = 0
                t[e, :, -(-min(c, k) // moe.GEMM_BK) * moe.GEMM_BK:] = NAN
    assert moe.moe_gemm(a, b, counts, mode, out=out, tile=tile) is out
    _check(out, moe.ref_moe_gemm(a, b, counts, mode), moe.ref_moe_gemm(a.abs(), b.abs(), counts, mode), k, f"{mode}")
    assert (mode is None or (out[0] == 0).all()) and (mode != "rows" or all((out[e, c:] == 0).all() for e, c in enumerate(cs)))
    assert torch.equal(moe.moe_gemm(a, b, counts, mode), out)  # a contiguous output, the default tile: the same bits
    out.fill_(POISON)
    assert (buf == POISON).all()  # the surroundings of C kept their poison


def _linear_case(n, k):
    g = torch.Generator(device=DEV).manual_seed(n + k + 1)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    live = (torch.arange(M, device=DEV)[None, :] < counts.clamp(max=M)[:, None]).reshape(-1, 1)
    xe = (torch.randn(NUM * M, k, device=DEV, generator=g) * live).bfloat16()
    dy = (torch.randn(NUM * M, n, device=DEV, generator=g) * live).bfloat16()
    w3 = (torch.randn(NUM, n, k, device=DEV, generator=g) * k ** -0.5).bfloat16()
    return xe, dy, w3, counts, xe.clone().requires_grad_(True), [w.detach().requires_grad_(True) for w in w3.unbind(0)]


@pytest.mark.parametrize("n,k", [(128, 128), (256, 384)])
def test_moe_linear_forward_and_backward(n, k):
    xe, dy, w3, counts, x, ws = _linear_case(n, k)
    y = moe.moe_linear(x, ws, counts)
    dx, *dw = torch.autograd.grad(y, (x, *ws), dy)
    x64, w64 = xe.double().requires_grad_(True), w3.double().requires_grad_(True)
    ref = moe.ref_moe_gemm(x64.view(NUM, M, k), w64, counts, "rows").view(-1, n)
    ref.backward(dy.double())
    xa, da, wa = xe.double().abs().view(NUM, M, k), dy.double().abs().view(NUM, M, n), w3.double().abs()
    _check(y, ref.detach(), (xa @ wa.transpose(1, 2)).view(-1, n), k, "y")
    _check(dx, x64.grad, (da @ wa).view(-1, k), n, "dx")
    _check(torch.stack(dw), w64.grad, da.transpose(1, 2) @ xa, M, "dw")
    assert all(g.data_ptr() == dw[0].data_ptr() + 2 * i * n * k for i, g in enumerate(dw))  # views of one buffer
    assert (dw[0] == 0).all() and (dx[:M] == 0).all() and (y[M + 1:2 * M] == 0).all()
    plain = moe.moe_linear(xe, list(w3.unbind(0)), counts)  # no gradient wanted: the raw forward, nothing saved
    assert plain.grad_fn is None and torch.equal(plain, y)


def test_moe_ffn_batched_gradients_against_an_fp32_copy():
    """test_moe_ffn_gradients_against_an_fp32_copy's rule and inputs; names, order, seeded values and
    routes equal the loop module's."""
    from kgs.models.moe import MoEFFN

    dim, inter, e, k, t = 512, 768, 8, 2, 512
    h = routing_input(t, dim, e, DEV)
    dy = torch.randn(t, dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).bfloat16()
    mods = {"batched": MoEFFN(dim, inter, e, k, backend="kgs", device=DEV, expert_gemm="batched"),
            "loop": MoEFFN(dim, inter, e, k, backend="kgs", device=DEV),
            "torch": MoEFFN(dim, inter, e, k, backend="torch", device=DEV, expert_gemm="batched"),
            "fp32": MoEFFN(dim, inter, e, k, backend="torch", device=DEV, dtype=torch.float32)}
    assert all(n1 == n2 and torch.equal(p1, p2) for (n1, p1), (n2, p2) in
               zip(mods["batched"].named_parameters(), mods["loop"].named_parameters()))
    grads = {}
    for name, m in mods.items():
        with torch.no_grad():
            m.router.weight.copy_(torch.eye(e, dim))
            for p, q in zip(m.parameters(), mods["batched"].parameters()):
                p.copy_(q.to(p.dtype))
        cast = (lambda z: z.float()) if name == "fp32" else (lambda z: z)
        hi = cast(h).clone().requires_grad_(True)
        m(hi).backward(cast(dy))
        grads[name] = {"h": hi.grad.float(), **{n: p.grad.float() for n, p in m.named_parameters()}}
    assert all(torch.equal(m.last_counts, mods["loop"].last_counts) for m in mods.values())
    assert int(mods["batched"].last_counts.sum()) == t * k and len(grads["batched"]) == 2 + 2 * e
    for n, ref in grads["fp32"].items():
        e_kgs, e_base = ((grads[s][n] - ref).abs().max().item() / ref.abs().max().item() for s in ("batched", "torch"))
        print(f"{n}: batched {e_kgs:.4f} torch {e_base:.4f}")
        assert e_base < 2e-2 and e_kgs <= 2 * e_base, (n, e_kgs, e_base)


def test_a_captured_step_replays_bitwise_and_holds_no_memset():
    from kgs.utils.graph_audit import audit

    _, dy, _, counts, x, ws = _linear_case(256, 384)

    def step():
        y = moe.moe_linear(x, ws, counts)
        return (y, *torch.autograd.grad(y, (x, *ws), dy))

    # detached: a live eager autograd graph would make the captured backward wait on the stream it was built on
    eager = tuple(t.detach() for t in step())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        got = tuple(t.detach() for t in step())
    found = audit(graph)
    assert found["memsets"] == [] and "memset" not in found["types"], found
    for _ in range(2):
        for out in got:
            out.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
