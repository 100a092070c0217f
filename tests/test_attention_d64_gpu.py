"""GPU tests of the head_dim 64 training attention kernels
(native/kernels/attention_d64.hip): forward with and without log-sum-exp, the
dQ / dK / dV kernels, the autograd op and a DecoderLayer with 64-wide heads.

The reference is the attention math in float64 (the bf16 inputs upcast, plain
matmul / softmax / autograd). Accuracy follows tests/test_attention_bwd_gpu.py:
the baseline is the same math in plain torch bf16 ops on the same GPU (bf16
matmul, fp32 softmax, P cast to bf16, bf16 matmul, autograd); the kernels round
P and dS to bf16 where it does, so their max error over the reference's max
must be within 2x the baseline's, and the baseline itself under 2e-2."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 64

SHAPES = [(1, 128, 2, 2),   # one tile: diagonal masking and the per-sub-block skip only
          (2, 256, 4, 1),   # batch offsets, a 4-head group summed into one dK/dV, a skipped causal tile
          (1, 384, 2, 2)]   # an odd number of 128-row blocks: the double buffer wraps
CASES = [(*s, c) for s in SHAPES for c in (True, False)] + [(1, 1024, 4, 2, True)]  # several key blocks per sweep


def _groups(x, nh, nkv):
    return {"dq": x[:, :nh * HD], "dk": x[:, nh * HD:(nh + nkv) * HD], "dv": x[:, (nh + nkv) * HD:(nh + 2 * nkv) * HD]}


def _math(qkv, dout, b, s, nh, nkv, causal, low):
    """(out, lse, dqkv) of the attention math by autograd: in float64, or (low)
    the bf16 baseline, which rounds the scores' softmax to bf16 before P.V."""
    leaf = (qkv if low else qkv.double()).clone().requires_grad_(True)
    q = leaf[:, :nh * HD].reshape(b, s, nh, HD).transpose(1, 2)
    k = leaf[:, nh * HD:(nh + nkv) * HD].reshape(b, s, nkv, HD).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    v = leaf[:, (nh + nkv) * HD:].reshape(b, s, nkv, HD).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    sc = q @ k.transpose(-1, -2)
    sc = (sc.float() if low else sc) / math.sqrt(HD)
    if causal:
        sc = sc.masked_fill(torch.triu(torch.ones(s, s, dtype=torch.bool, device=DEV), 1), float("-inf"))
    o = (torch.softmax(sc, -1).to(leaf.dtype) @ v).transpose(1, 2).reshape(b * s, nh * HD)
    o.backward(dout.to(o.dtype))
    return o.detach(), torch.logsumexp(sc.detach(), -1).reshape(b * nh, s), leaf.grad


@functools.lru_cache(maxsize=None)
def _case(b, s, nh, nkv, causal, qscale=1.0):
    """One forward + backward of a case, its float64 reference and its bf16
    baseline, computed once and shared by the tests (nothing modifies them)."""
    from kgs.ops.transformer import attention_qkv_backward, attention_qkv_lse

    g = torch.Generator(device=DEV).manual_seed(b + s + nh)
    qkv = torch.randn(b * s, (nh + 2 * nkv) * HD, device=DEV, generator=g)
    qkv[:, :nh * HD] *= qscale
    qkv, dout = qkv.bfloat16(), torch.randn(b * s, nh * HD, device=DEV, generator=g).bfloat16()
    out, lse = attention_qkv_lse(qkv, b, s, nh, nkv, causal=causal, head_dim=HD)
    dqkv = attention_qkv_backward(qkv, out, dout, lse, b, s, nh, nkv, causal=causal, head_dim=HD)
    torch.cuda.synchronize()
    return {"qkv": qkv, "dout": dout, "out": out, "lse": lse, "dqkv": dqkv,
            "ref": _math(qkv, dout, b, s, nh, nkv, causal, False), "base": _math(qkv, dout, b, s, nh, nkv, causal, True)}


@pytest.mark.parametrize("b,s,nh,nkv,causal", CASES)
def test_forward_and_gradients_against_float64(b, s, nh, nkv, causal):
    """out, dq, dk, dv within 2x the bf16 baseline's error; lse within 1e-3 of
    the float64 logsumexp (exact fp32 score sums, a 2^-24 fma rounding and a few
    ulp of v_exp / v_log: of order 1e-5); the forward without lse gives the
    same output bits."""
    from kgs.ops.transformer import attention_qkv

    c = _case(b, s, nh, nkv, causal)
    (ro, rl, rg), (bo, _, bg) = c["ref"], c["base"]
    assert torch.equal(c["out"], attention_qkv(c["qkv"], b, s, nh, nkv, head_dim=HD, causal=causal))
    assert c["lse"].dtype == torch.float32 and c["lse"].shape == (b * nh, s)
    lse_err = (c["lse"].double() - rl).abs().max().item()
    got, bas, ref = {"out": c["out"], **_groups(c["dqkv"], nh, nkv)}, {"out": bo, **_groups(bg, nh, nkv)}, \
        {"out": ro, **_groups(rg, nh, nkv)}
    errs = {}
    for n, r in ref.items():
        mag = r.abs().max().item()
        errs[n] = ((got[n].double() - r).abs().max().item() / mag, (bas[n].double() - r).abs().max().item() / mag)
    print(f"lse err {lse_err:.3e}; err (kgs, baseline):", {n: (f"{e[0]:.4f}", f"{e[1]:.4f}") for n, e in errs.items()})
    assert lse_err < 1e-3, lse_err
    assert torch.isfinite(c["dqkv"].float()).all()
    for n, (e_kgs, e_base) in errs.items():
        assert e_base < 2e-2, (n, e_base)  # the rule below cannot hide a failure behind a bad baseline
        assert e_kgs <= 2 * e_base, (n, e_kgs, e_base)


@pytest.mark.parametrize("causal", [True, False])
def test_gradients_of_peaky_scores(causal):
    """q x 8: P is near one-hot and the deferred maximum trails the true one."""
    b, s, nh, nkv = 2, 256, 4, 1
    c = _case(b, s, nh, nkv, causal, 8.0)
    got, ref = _groups(c["dqkv"].double(), nh, nkv), _groups(c["ref"][2], nh, nkv)
    assert torch.isfinite(c["dqkv"].float()).all() and torch.isfinite(c["out"].float()).all()
    assert torch.isfinite(c["lse"]).all()
    for n in ("dq", "dk", "dv"):
        err, mag = (got[n] - ref[n]).abs().max().item(), ref[n].abs().max().item()
        print(f"{n}: err {err:.4f} mag {mag:.2f}")
        assert err < 4e-2 * max(1.0, mag), (n, err, mag)


@pytest.mark.parametrize("row", [5, 200])
def test_one_row_of_dout_reaches_only_its_own_query_and_earlier_keys(row):
    from kgs.ops.transformer import attention_qkv_backward

    b, s, nh, nkv = 1, 384, 2, 2
    c = _case(b, s, nh, nkv, True)
    dout = torch.zeros_like(c["dout"])
    dout[row] = c["dout"][row]
    g = _groups(attention_qkv_backward(c["qkv"], c["out"], dout, c["lse"], b, s, nh, nkv, causal=True, head_dim=HD)
                .view(torch.int16), nh, nkv)
    assert (g["dk"][row + 1:] == 0).all() and (g["dv"][row + 1:] == 0).all()
    assert (g["dq"][:row] == 0).all() and (g["dq"][row + 1:] == 0).all()
    assert g["dq"][row].count_nonzero() > 0 and g["dk"][:row + 1].count_nonzero() > 0
    assert g["dv"][:row + 1].count_nonzero() > 0


@pytest.mark.parametrize("causal", [True, False])
def test_strided_dout_and_a_wider_poisoned_dqkv(causal):
    from kgs.ops.transformer import attention_qkv_backward

    b, s, nh, nkv = 2, 256, 4, 1
    c = _case(b, s, nh, nkv, causal)
    t, qc, w = b * s, nh * HD, (nh + 2 * nkv) * HD
    wide = torch.full((t, qc + 128), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, 64:64 + qc] = c["dout"]
    poison = 1234.0
    buf = torch.full((t + 3, w + 256), poison, dtype=torch.bfloat16, device=DEV)
    got = attention_qkv_backward(c["qkv"], c["out"], wide[:, 64:64 + qc], c["lse"], b, s, nh, nkv, causal=causal,
                                 dqkv=buf[:, 128:128 + w + 64], head_dim=HD)
    assert got.data_ptr() == buf[:, 128:].data_ptr()
    assert torch.equal(buf[:t, 128:128 + w], c["dqkv"])
    assert (buf[:, :128] == poison).all() and (buf[:, 128 + w:] == poison).all() and (buf[t:] == poison).all()


@pytest.mark.parametrize("b,s,nh,nkv,causal", [(2, 256, 4, 1, True), (1, 384, 2, 2, False)])
def test_repeatable_and_graph_capturable(b, s, nh, nkv, causal):
    from kgs.ops.transformer import attention_qkv_backward, attention_qkv_lse

    c = _case(b, s, nh, nkv, causal)
    again = attention_qkv_backward(c["qkv"], c["out"], c["dout"], c["lse"], b, s, nh, nkv, causal=causal, head_dim=HD)
    assert torch.equal(again, c["dqkv"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = attention_qkv_lse(c["qkv"], b, s, nh, nkv, causal=causal, head_dim=HD)
        dqkv = attention_qkv_backward(c["qkv"], out, c["dout"], lse, b, s, nh, nkv, causal=causal, head_dim=HD)
    for _ in range(2):
        for x in (out, lse, dqkv):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, c["out"]) and torch.equal(lse, c["lse"]) and torch.equal(dqkv, c["dqkv"])


def test_autograd_op_runs_the_kernels_and_saves_nothing_without_a_gradient():
    from kgs.ops.transformer import attention_qkv, flash_attention_qkv

    b, s, nh, nkv = 2, 256, 4, 1
    c = _case(b, s, nh, nkv, True)
    leaf = c["qkv"].clone().requires_grad_(True)
    y = flash_attention_qkv(leaf, b, s, nh, nkv, causal=True, head_dim=HD)
    assert torch.equal(y, c["out"])
    y.backward(c["dout"])
    assert torch.equal(leaf.grad, c["dqkv"])
    y0 = flash_attention_qkv(c["qkv"], b, s, nh, nkv, causal=True, head_dim=HD)
    assert y0.grad_fn is None and not y0.requires_grad
    assert torch.equal(y0, attention_qkv(c["qkv"], b, s, nh, nkv, head_dim=HD, causal=True))


def test_decoder_layer_with_64_wide_heads_against_an_fp32_copy():
    """Input and parameter gradients of the kgs layer against an fp32 copy with
    the same rounded weights: within 2x the torch bf16 backend's error."""
    from kgs.models.decoder import DecoderLayer

    dim, nh, nkv, inter, b, s = 512, 8, 2, 1024, 2, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    x, d, dy1, dy2 = (torch.randn(b, s, dim, device=DEV, generator=g).bfloat16() for _ in range(4))
    layers = {"kgs": DecoderLayer(dim, nh, nkv, inter, backend="kgs", device=DEV),
              "torch": DecoderLayer(dim, nh, nkv, inter, backend="torch", device=DEV),
              "fp32": DecoderLayer(dim, nh, nkv, inter, backend="torch", device=DEV, dtype=torch.float32)}
    assert layers["kgs"].head_dim == HD
    grads = {}
    for name, layer in layers.items():
        cast = (lambda t: t.float()) if name == "fp32" else (lambda t: t)
        with torch.no_grad():
            for p, q in zip(layer.parameters(), layers["kgs"].parameters()):
                p.copy_(q.to(p.dtype))
        xi, di = cast(x).clone().requires_grad_(True), cast(d).clone().requires_grad_(True)
        torch.autograd.backward(list(layer(xi, di)), [cast(dy1), cast(dy2)])
        grads[name] = {"x": xi.grad.float(), "delta": di.grad.float(),
                       **{n: p.grad.float() for n, p in layer.named_parameters()}}
    assert len(grads["fp32"]) == 8
    for n, ref in grads["fp32"].items():
        mag = ref.abs().max().item()
        e_kgs = (grads["kgs"][n] - ref).abs().max().item() / mag
        e_base = (grads["torch"][n] - ref).abs().max().item() / mag
        print(f"{n}: kgs {e_kgs:.4f} torch {e_base:.4f}")
        assert e_base < 2e-2, (n, e_base)
        assert e_kgs <= 2 * e_base, (n, e_kgs, e_base)


def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    from kgs.ops import _lib

    b, s, nh, nkv = 1, 256, 2, 1
    c = _case(1, 384, 2, 2, True)  # any valid device buffers of at least this size
    qkv, out, dout, lse = c["qkv"], c["out"], c["dout"], c["lse"]
    poison = 1234.0
    dqkv, o2 = torch.full_like(qkv, poison), torch.full_like(out, poison)
    ws = torch.full((b * nh * s,), poison, device=DEV)
    ld, st = qkv.stride(0), _lib.stream_handle(qkv.device)
    ko, vo = nh * HD * 2, (nh + nkv) * HD * 2

    def bwd(S=s, q_off=0, ws_ptr=None):
        ws_ptr = ws.data_ptr() if ws_ptr is None else ws_ptr
        return _lib.lib().kgs_attn64_bwd_bf16(
            qkv.data_ptr() + q_off, qkv.data_ptr() + ko, qkv.data_ptr() + vo, out.data_ptr(), dout.data_ptr(),
            lse.data_ptr(), dqkv.data_ptr(), dqkv.data_ptr() + ko, dqkv.data_ptr() + vo, ctypes.c_void_p(ws_ptr),
            b, S, nh, nkv, ld, ld, ld, out.stride(0), dout.stride(0), ld, ld, ld, 0.125, 1, st)

    def fwd(S=s, q_off=0):
        return _lib.lib().kgs_attn64_fwd_bf16(qkv.data_ptr() + q_off, qkv.data_ptr() + ko, qkv.data_ptr() + vo,
                                              o2.data_ptr(), None, b, S, nh, nkv, ld, ld, ld, o2.stride(0), 0.125, 1, st)

    assert bwd(S=192) == -1 and fwd(S=192) == -1      # KGS_ERR_SHAPE: S % 128
    assert bwd(q_off=2) == -2 and fwd(q_off=2) == -2  # KGS_ERR_ALIGN: pointer not 16-byte aligned
    assert bwd(ws_ptr=0) == -2                        # KGS_ERR_ALIGN: null workspace
    torch.cuda.synchronize()
    assert (dqkv == poison).all() and (ws == poison).all() and (o2 == poison).all()
