"""GPU tests of the mixture-of-experts routing kernels (native/kernels/moe_route.hip)
against the float64 references of kgs/ops/moe.py."""
import ctypes
import functools

import pytest
import torch

from forward_refs import POISON, poison_intact, wide, within
from kgs.ops import moe
from test_moe import routing_input

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (T, E, k, C). No T is a multiple of a wave, of the 512 / E rows a wave selects per trip or of
# the 1024 flat indices a workgroup of the rank passes owns: T k = 2000, 8000 and 16532 span 2,
# 8 and 17 of those workgroups. (777, 8, 2, 8): every token's first pick is expert 3.
CASES = [(5, 8, 1, 4), (1000, 8, 2, 300), (1000, 64, 8, 96), (4133, 128, 4, 160), (777, 8, 2, 8)]
DIMS = [8, 520, 4096]
ULP = 2.0 ** -20


def _raw(fn, *args):
    from kgs.ops import _lib

    conv = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else ctypes.c_void_p(0) if a is None else a
            for a in args]
    return getattr(_lib.lib(), fn)(*conv, _lib.stream_handle(torch.device(DEV)))


@functools.lru_cache(maxsize=None)
def _case(t, e, k, c, d=0):
    """d = 0: the logits (a wide view), the kernels' route and the reference's. d > 0: wide
    inputs of that width and the raw entries' outputs in poisoned wide buffers. Computed once
    and shared by the tests (nothing below modifies them)."""
    g = torch.Generator(device=DEV).manual_seed(t + e + k + d)
    if d == 0:
        lg = ((torch.randn(t, e, device=DEV, generator=g) * 4).round() / 4).bfloat16()
        if (t, c) == (777, 8):
            lg[:, 3] = 16.0
        logits, buf = wide(lg)
        return {"logits": logits, "buf": buf, "route": moe.moe_route(logits, k, c), "ref": moe.ref_moe_route(logits, k, c)}
    r = _case(t, e, k, c)["route"]
    o = {"d": d, "dw_in": torch.randn(t, k, device=DEV, generator=g)}
    for name, rows in (("x", t), ("ye", e * c), ("dy", t), ("dxe", e * c)):
        o[name], _ = wide(torch.randn(rows, d, device=DEV, generator=g).bfloat16(), pad=72)
    for name, rows in (("xe", e * c), ("y", t), ("dx", t), ("dye", e * c)):
        o[name], o[name + "_buf"] = wide(torch.zeros(rows, d, dtype=torch.bfloat16, device=DEV), pad=136)
        o[name].fill_(POISON)
    o["dl"], o["dl_buf"] = wide(torch.full((t, e), POISON, dtype=torch.bfloat16, device=DEV))
    o["dw"] = torch.full((t * k + 2,), POISON, device=DEV)
    ld = lambda m: m.stride(0)  # noqa: E731
    assert _raw("kgs_moe_gather_bf16", o["x"], r.src, None, o["xe"], t, e * c, k, d, ld(o["x"]), ld(o["xe"])) == 0
    assert _raw("kgs_moe_combine_bf16", o["ye"], r.slot, r.weights, o["y"], t, e * c, k, d, ld(o["ye"]), ld(o["y"])) == 0
    assert _raw("kgs_moe_combine_bf16", o["dxe"], r.slot, None, o["dx"], t, e * c, k, d, ld(o["dxe"]), ld(o["dx"])) == 0
    assert _raw("kgs_moe_combine_bwd_bf16", o["dy"], o["ye"], r.slot, r.src, r.weights, o["dye"], o["dw"], t, e * c, k,
                d, ld(o["dy"]), ld(o["ye"]), ld(o["dye"])) == 0
    assert _raw("kgs_moe_route_bwd_bf16", o["dw_in"], r.weights, r.experts, o["dl"], t, e, k, ld(o["dl"])) == 0
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("t,e,k,c", CASES)
def test_route_equals_the_reference(t, e, k, c):
    """Indices equal, ties included; weights within 1e-6 of float64 (they are at most 1, and
    fp32 exp, a k-term sum and a quotient are a few 2^-24)."""
    o = _case(t, e, k, c)
    r, ref = o["route"], o["ref"]
    for name in ("experts", "slot", "src", "counts"):
        assert getattr(r, name).dtype == torch.int32 and torch.equal(getattr(r, name), getattr(ref, name)), name
    err = (r.weights.double() - ref.weights).abs().max().item()
    print(f"weights: max err {err:.3e}; dropped {int((r.slot < 0).sum())} of {t * k}, counts max {int(r.counts.max())}")
    assert r.weights.dtype == torch.float32 and err <= 1e-6
    assert poison_intact(o["buf"], t, e)
    if (t, c) == (777, 8):
        assert int(r.counts[3]) == t and int((r.slot < 0).sum()) >= t - c


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t,e,k,c", CASES)
def test_dispatch_and_combine_forward_and_backward(t, e, k, c, d):
    r, o = _case(t, e, k, c)["route"], _case(t, e, k, c, d)
    w = r.weights
    assert torch.equal(o["xe"], moe.ref_moe_gather(o["x"], r.src, k)), "xe"
    within(o["y"], moe.ref_moe_combine(o["ye"], r.slot, w), ULP * moe.ref_moe_combine(o["ye"].abs(), r.slot, w), "y")
    within(o["dx"], moe.ref_moe_combine(o["dxe"], r.slot), ULP * moe.ref_moe_combine(o["dxe"].abs(), r.slot), "dx")
    rdye, rdw = moe.ref_moe_combine_backward(o["dy"], o["ye"], r.slot, r.src, w)
    within(o["dye"], rdye, 0.0, "dye")
    assert (o["dye"][r.src < 0] == 0).all() and (o["xe"][r.src < 0] == 0).all()
    dw = o["dw"][:t * k].view(t, k)
    bound = ULP * moe.ref_moe_combine_backward(o["dy"].abs(), o["ye"].abs(), r.slot, r.src, w)[1]
    print(f"dweights: least margin {(bound - (dw.double() - rdw).abs()).min().item():.3e}")
    assert bool(((dw.double() - rdw).abs() <= bound).all()) and (o["dw"][t * k:] == POISON).all()
    wd, ad = w.double(), o["dw_in"].double().abs()
    atol = torch.zeros(t, e, dtype=torch.float64, device=DEV).scatter_(
        1, r.experts.long(), ULP * wd * (ad + (wd * ad).sum(1, keepdim=True)))
    within(o["dl"], moe.ref_moe_route_backward(o["dw_in"], w, r.experts, e), atol, "dlogits")
    assert int((o["dl"] != 0).sum(1).max()) <= k
    assert all(poison_intact(o[n + "_buf"], o[n].shape[0], o[n].shape[1]) for n in ("xe", "y", "dx", "dye", "dl"))


@pytest.mark.parametrize("t,e,k,c,d", [(5, 8, 1, 4, 8), (4133, 128, 4, 160, 520)])
def test_repeatable_and_capturable(t, e, k, c, d):
    from kgs.utils.graph_audit import audit

    base, o = _case(t, e, k, c), _case(t, e, k, c, d)

    def step():
        r = moe.moe_route(base["logits"], k, c)
        dye, dw = moe.moe_combine_backward(o["dy"], o["ye"], r.slot, r.src, r.weights)
        return (*r, moe.moe_gather(o["x"], r.src, k), moe.moe_combine(o["ye"], r.slot, r.weights),
                moe.moe_combine(o["dxe"], r.slot), dye, dw, moe.moe_route_backward(o["dw_in"], r.weights, r.experts, e))

    eager = step()
    want = (*base["route"], o["xe"], o["y"], o["dx"], o["dye"], o["dw"][:t * k].view(t, k), o["dl"])
    assert all(torch.equal(a, b) for a, b in zip(eager, want))  # the wrappers give the raw entries' bits, again
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        got = step()
    found = audit(graph)
    assert found["memsets"] == [] and "memset" not in found["types"], found
    for _ in range(3):
        for out in got:
            out.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, eager))


def test_autograd_ops_give_the_raw_entries_bits():
    t, e, k, c, d = 1000, 8, 2, 300, 520
    base, o = _case(t, e, k, c), _case(t, e, k, c, d)
    logits, x, ye = (z.clone().requires_grad_(True) for z in (base["logits"], o["x"], o["ye"]))
    route = moe.moe_router(logits, k, c)
    xe, y = moe.moe_dispatch(x, route), moe.moe_combine(ye, route)
    torch.autograd.backward([xe, y], [o["dxe"], o["dy"]])
    assert all(torch.equal(a, b) for a, b in zip(route, base["route"]))
    assert torch.equal(xe, o["xe"]) and torch.equal(y, o["y"])
    assert torch.equal(x.grad, o["dx"]) and torch.equal(ye.grad, o["dye"])
    dw = o["dw"][:t * k].view(t, k).contiguous()
    assert torch.equal(logits.grad, moe.moe_route_backward(dw, route.weights.detach(), route.experts, e))
    plain = moe.moe_router(base["logits"], k, c)  # no gradient wanted: the raw forwards, nothing saved
    outs = (plain.weights, moe.moe_dispatch(o["x"], plain), moe.moe_combine(o["ye"], plain))
    assert all(z.grad_fn is None and not z.requires_grad for z in outs)
    assert torch.equal(outs[1], o["xe"]) and torch.equal(outs[2], o["y"])


def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    from kgs.ops import _lib

    t, e, k, c = 5, 8, 1, 4
    logits = _case(t, e, k, c)["logits"]
    w = torch.full((t, k), POISON, device=DEV)
    ex, sl, src, cnt = (torch.full((n,), 1234, dtype=torch.int32, device=DEV) for n in (t * k, t * k, e * c, e))
    ws = torch.full((_lib.lib().kgs_moe_workspace(t, e, k) // 4,), 1234, dtype=torch.int32, device=DEV)
    out, _ = wide(torch.full((t, 16), POISON, dtype=torch.bfloat16, device=DEV))
    ld = logits.stride(0)
    assert _raw("kgs_moe_route_bf16", logits.data_ptr() + 2, w, ex, sl, src, cnt, ws, t, e, k, c, ld) == -2
    assert _raw("kgs_moe_route_bf16", logits, w, ex, sl, src, cnt, None, t, e, k, c, ld) == -2
    assert _raw("kgs_moe_route_bf16", logits, w, ex, sl, src, cnt, ws, t, 12, k, c, ld) == -1
    assert _lib.lib().kgs_moe_workspace(t, 12, k) == -1
    assert _raw("kgs_moe_route_bwd_bf16", w, w, ex, out.data_ptr() + 2, t, 16, k, out.stride(0)) == -2
    assert _raw("kgs_moe_route_bwd_bf16", w, w, ex, out, t, 12, k, out.stride(0)) == -1
    assert _raw("kgs_moe_gather_bf16", logits.data_ptr() + 2, src, None, out, t, t, k, 8, ld, out.stride(0)) == -2
    assert _raw("kgs_moe_gather_bf16", logits, src, None, out, t, t, k, 12, ld, out.stride(0)) == -1
    assert _raw("kgs_moe_combine_bf16", logits, sl, None, out.data_ptr() + 2, t, t, k, 8, ld, out.stride(0)) == -2
    assert _raw("kgs_moe_combine_bwd_bf16", logits, logits, sl, src, w, out, None, t, t, k, 8, ld, ld, out.stride(0)) == -2
    torch.cuda.synchronize()
    assert (w == POISON).all() and (out == POISON).all() and all((z == 1234).all() for z in (ex, sl, src, cnt, ws))


def test_a_nan_logit_keeps_every_index_in_range():
    """The NaN sits in the last row, the lowest priority, so no other row's slot depends on it."""
    t, e, k, c = 1000, 64, 8, 96
    base = _case(t, e, k, c)
    lg = base["logits"].clone()
    lg[-1, 37] = float("nan")
    r, want = moe.moe_route(lg, k, c), base["route"]
    assert torch.isnan(r.weights[-1]).all() and not torch.isnan(r.weights[:-1]).any()
    assert int(r.experts.min()) >= 0 and int(r.experts.max()) < e and int(r.slot.min()) >= -1
    assert int(r.slot.max()) < e * c and int(r.src.min()) >= -1 and int(r.src.max()) < t * k
    for name in ("weights", "experts", "slot"):
        assert torch.equal(getattr(r, name)[:-1], getattr(want, name)[:-1]), name


def test_moe_ffn_gradients_against_an_fp32_copy():
    """test_decoder_layer_gradients_against_an_fp32_copy's rule for every gradient, the router's
    included. Routing is discrete: the router weight [I | 0] and rows that start with a
    permutation of 0, 0.5, .. 3.5 make the logits exact, hence the routes equal, in every precision."""
    from kgs.models.moe import MoEFFN

    dim, inter, e, k, t = 512, 768, 8, 2, 512
    h = routing_input(t, dim, e, DEV)
    dy = torch.randn(t, dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).bfloat16()
    mods = {"kgs": MoEFFN(dim, inter, e, k, backend="kgs", device=DEV),
            "torch": MoEFFN(dim, inter, e, k, backend="torch", device=DEV),
            "fp32": MoEFFN(dim, inter, e, k, backend="torch", device=DEV, dtype=torch.float32)}
    grads = {}
    for name, m in mods.items():
        with torch.no_grad():
            m.router.weight.copy_(torch.eye(e, dim))
            for p, q in zip(m.parameters(), mods["kgs"].parameters()):
                p.copy_(q.to(p.dtype))
        cast = (lambda z: z.float()) if name == "fp32" else (lambda z: z)
        hi = cast(h).clone().requires_grad_(True)
        m(hi).backward(cast(dy))
        grads[name] = {"h": hi.grad.float(), **{n: p.grad.float() for n, p in m.named_parameters()}}
    assert all(torch.equal(m.last_counts, mods["fp32"].last_counts) for m in mods.values())
    assert int(mods["kgs"].last_counts.sum()) == t * k and len(grads["fp32"]) == 2 + 2 * e
    for n, ref in grads["fp32"].items():
        mag = ref.abs().max().item()
        e_kgs = (grads["kgs"][n] - ref).abs().max().item() / mag
        e_base = (grads["torch"][n] - ref).abs().max().item() / mag
        print(f"{n}: kgs {e_kgs:.4f} torch {e_base:.4f}")
        assert e_base < 2e-2, (n, e_base)
        assert e_kgs <= 2 * e_base, (n, e_kgs, e_base)
