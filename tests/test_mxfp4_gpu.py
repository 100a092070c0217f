"""MXFP4 weight-only decode (W4A16) on the GPU: the skinny GEMM's mxfp4
instantiations against the bf16 kernel on the dequantised weight (bitwise: the
in-register dequant is exact and the k order unchanged), the element map with
exact data, the fused epilogues, rejections, graph replay, and the serving
engine with ``decode_weights="mxfp4"`` against an oracle carrying the engine's
own rounded weights."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, K = 768, 2048


@pytest.fixture(scope="module", autouse=True)
def _native():
    from kgs.ops import _lib

    _lib.lib()
    torch.manual_seed(0)


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


@pytest.fixture(scope="module")
def weights():
    """One Gaussian [768, 2048] weight: its mxfp4 packing, the dequantised weight
    packed as bf16, and the dequantised weight in fp32 (never modified)."""
    from kgs.ops.decode import PackedWeight

    w = _bf(N, K, scale=K ** -0.5, seed=1)
    pw4 = PackedWeight(w, mxfp4=True)
    wd = pw4.unpacked()
    return pw4, PackedWeight(wd), wd.float()


def _variants(m):
    from kgs.ops.decode import KIN_VARIANTS, skinny_variants

    return [v for v in skinny_variants(m) if v <= 12 or v in KIN_VARIANTS]


def _ksplits(m, v):
    from kgs.ops.decode import skinny_geometry

    nchunks = K // skinny_geometry(m, v)[1]
    return [d for d in range(1, nchunks + 1) if nchunks % d == 0]


@pytest.mark.parametrize("k0", [0, 64, 1984])
def test_element_map_exact(k0):
    """Random codes, random exponents in a narrow range, one-hot x: row m of y
    is column k0 + m of the dequantised weight, bit for bit. Pins the nibble,
    byte, lane and scale-byte order of the packed layout in one go."""
    from kgs.ops.decode import PackedWeight, mxfp4_dequantize, pack_mxfp4, skinny_gemm

    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    exps = torch.randint(120, 128, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    dq = mxfp4_dequantize(codes, exps)
    pw = PackedWeight.__new__(PackedWeight)
    pw.n, pw.k, pw.swiglu, pw.fp8, pw.rope, pw.mxfp4 = N, K, False, False, None, True
    pw.data, pw.wscale = (t.to(DEV) for t in pack_mxfp4(codes, exps))
    assert torch.equal(pw.unpacked().cpu(), dq)
    for m in (64, 16):  # 16: the variants whose waves split K inside the workgroup too
        x = torch.zeros(m, K, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(m), k0 + torch.arange(m)] = 1
        want = dq[:, k0:k0 + m].T.contiguous()
        want = torch.where(want == 0, torch.zeros_like(want), want)  # a -0 product plus +0 products is +0
        for v in _variants(m):
            for ks in (1, _ksplits(m, v)[-1]):
                y = skinny_gemm(x, pw, ksplit=ks, variant=v)
                torch.cuda.synchronize()
                assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), (m, v, ks)


@pytest.mark.parametrize("m", [1, 16, 17, 30, 33, 64])
def test_same_arithmetic_as_bf16(m, weights):
    from kgs.ops.decode import skinny_config, skinny_gemm

    pw4, pwd, wd = weights
    x = _bf(m, K, seed=10 + m)
    ref = x.float() @ wd.T
    bound = 2e-2 * ref.abs().max().item() + 1e-3
    for v in _variants(m):
        for ks in _ksplits(m, v):
            y4 = skinny_gemm(x, pw4, ksplit=ks, variant=v)
            yd = skinny_gemm(x, pwd, ksplit=ks, variant=v)
            torch.cuda.synchronize()
            assert torch.equal(y4.view(torch.int16), yd.view(torch.int16)), (v, ks)
            assert (y4.float() - ref).abs().max().item() <= bound, (v, ks)
    # the route skinny_config picks for mxfp4
    v0, ks0 = skinny_config(m, N, K, mxfp4=True)
    y4, yd = skinny_gemm(x, pw4), skinny_gemm(x, pwd, variant=v0, ksplit=ks0)
    torch.cuda.synchronize()
    assert torch.equal(y4.view(torch.int16), yd.view(torch.int16))


def test_strided_x(weights):
    from kgs.ops.decode import skinny_gemm

    pw4, pwd, wd = weights
    m = 12
    big = _bf(m, K + 64, seed=3)
    x = big[:, 32:32 + K]
    assert x.stride(0) > K
    out_big = torch.zeros(m, N + 128, dtype=torch.bfloat16, device=DEV)
    ref = x.float() @ wd.T
    for v in _variants(m):
        for ks in _ksplits(m, v):
            out = out_big[:, 64:64 + N]
            skinny_gemm(x, pw4, out=out, ksplit=ks, variant=v)
            yd = skinny_gemm(x, pwd, ksplit=ks, variant=v)
            torch.cuda.synchronize()
            assert torch.equal(out.contiguous().view(torch.int16), yd.view(torch.int16)), (v, ks)
            assert (out.float() - ref).abs().max().item() <= 2e-2 * ref.abs().max().item() + 1e-3
    assert out_big[:, :64].abs().max().item() == 0 and out_big[:, 64 + N:].abs().max().item() == 0


@pytest.mark.parametrize("m", [3, 32, 64])
def test_epilogues(m):
    """RMS + SWIGLU on a folded gate|up weight, and RESID with resid_ss and
    zero: y bitwise the bf16 kernel's on the unpacked weight."""
    from kgs.ops.decode import PackedWeight, skinny_config, skinny_gemm

    h, n = 1024, 1536
    x = _bf(m, h, seed=20)
    lnw = (_bf(h, scale=0.2, seed=21) + 1).contiguous()
    ss = x.float().pow(2).sum(-1)
    wgu = _bf(2 * n, h, scale=h ** -0.5, seed=22)
    p4 = PackedWeight(wgu, swiglu=True, fold=lnw, mxfp4=True)
    pd = PackedWeight(p4.unpacked(), swiglu=True)
    for v in _variants(m):
        got = skinny_gemm(x, p4, rms=ss, eps=1e-5, variant=v, ksplit=1)
        want = skinny_gemm(x, pd, rms=ss, eps=1e-5, variant=v, ksplit=1)
        torch.cuda.synchronize()
        assert got.shape == (m, n) and torch.equal(got.view(torch.int16), want.view(torch.int16)), v
    # fp32 math on the dequantised weight
    wd = p4.unpacked().float()
    yn = x.float() * torch.rsqrt(ss / h + 1e-5)[:, None]
    g, u = yn @ wd[:n].T, yn @ wd[n:].T
    ref = g * torch.sigmoid(g) * u
    assert (got.float() - ref).abs().max().item() <= 3e-2 * ref.abs().max().item()
    # residual
    wo = _bf(h, n, scale=n ** -0.5, seed=23)
    o4 = PackedWeight(wo, mxfp4=True)
    od = PackedWeight(o4.unpacked())
    a = _bf(m, n, seed=24)
    res0 = _bf(m, h, seed=25)
    for v, ks in ((0, 1), skinny_config(m, h, n, mxfp4=True)):
        outs = []
        for pw in (o4, od):
            res = res0.clone()
            ss_out = torch.zeros(m, device=DEV)
            junk = torch.full((m,), 7.0, device=DEV)
            skinny_gemm(a, pw, out=res, resid_ss=ss_out, zero=junk, variant=v, ksplit=ks)
            torch.cuda.synchronize()
            assert junk.abs().max().item() == 0
            assert torch.allclose(ss_out, res.float().pow(2).sum(-1), rtol=1e-4, atol=1e-3)
            outs.append((res, ss_out))
        assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)), ks
        assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-3)


def test_rejections_before_launch(weights):
    from kgs.ops import _lib
    from kgs.ops.decode import EPI_RMS, _workspace, skinny_gemm

    pw4, _, _ = weights
    with pytest.raises(ValueError, match="mxfp4.*<= 64"):
        skinny_gemm(_bf(65, K), pw4)
    m = 8
    x = _bf(m, K + 64)
    y = torch.full((m, N), 3.0, dtype=torch.bfloat16, device=DEV)
    ws, cnt = _workspace(x.device, 16 * N * 4, N // 16)
    so = _lib.lib()

    def call(k=K, scales=pw4.wscale.data_ptr(), variant=1, epi=0, rows=m):
        return so.kgs_skinny_gemm_mxfp4_fused(pw4.data.data_ptr(), scales, x.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                              cnt.data_ptr(), rows, N, k, x.stride(0), y.stride(0), 1, variant, epi,
                                              None, None, None, 1.0 / K, 1e-5, None)

    SHAPE, ALIGN, ARG = -1, -2, -3
    assert call(k=K + 64) == SHAPE          # K % 128
    assert call(scales=None) == ARG         # null scales
    assert call(scales=pw4.wscale.data_ptr() + 4) == ALIGN
    assert call(variant=13, rows=100) == ARG
    assert call(variant=13) == ARG
    assert call(epi=8) == ARG               # EPI_ROPE
    assert call(epi=8 | EPI_RMS) == ARG
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())           # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, skinny_gemm(x[:, :K], pw4, variant=1, ksplit=1))


@pytest.mark.parametrize("m,v,ks", [(5, 20, 2), (5, 1, 4), (40, 9, 8)])
def test_graph_replay_is_bitwise_eager(m, v, ks, weights):
    from kgs.ops.decode import skinny_gemm

    pw4, _, _ = weights
    x = _bf(m, K, seed=30)
    want = skinny_gemm(x, pw4, ksplit=ks, variant=v)
    out = torch.zeros_like(want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        skinny_gemm(x, pw4, out=out, ksplit=ks, variant=v)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# ---------------------------------------------------------------- engine

def _cfg():
    from kgs.models.llama import LlamaConfig

    return LlamaConfig(hidden=512, intermediate=1024, heads=4, kv_heads=1, layers=2, vocab=1024)


def _engine(**kw):
    from kgs.serve import EngineConfig, LLMEngine

    ec = EngineConfig(num_pages=kw.pop("num_pages", 256), max_batch=kw.pop("max_batch", 8), max_model_len=1024,
                      cuda_graphs=True, decode_weights="mxfp4", **kw)
    return LLMEngine(_cfg(), ec, device="cuda", backend="kgs")


def _oracle_check(eng, prompts, outs, tol=3e-2):
    """Against a torch-backend model that carries the engine's own rounded weights."""
    from kgs.ops.decode import mxfp4_dequantize, mxfp4_quantize

    oracle = eng.model.oracle
    ref = type(oracle)(oracle.cfg, device="cuda", backend="torch", seed=0)
    for i, lw in enumerate(eng.model.w):
        for name, w in lw.items():
            assert torch.equal(w, mxfp4_dequantize(*mxfp4_quantize(w))), (i, name)
            assert not torch.equal(ref.layers[i][name].w, w)
            ref.layers[i][name].w.copy_(w)
    ref.lm_head.w.copy_(eng.model.w_lm)
    for prompt, req in zip(prompts, outs):
        seq = list(prompt)
        for tok in req.output:
            logits = ref.forward(torch.tensor([seq], device="cuda"))[0, -1].float()
            assert logits[tok] >= logits.max() - tol * logits.abs().max(), (len(seq), tok, int(logits.argmax()))
            seq.append(tok)


@pytest.mark.parametrize("fused_max_batch", [48, 0])
def test_engine_mxfp4_matches_oracle(fused_max_batch):
    from kgs.serve import SamplingParams

    eng = _engine(fused_max_batch=fused_max_batch)
    assert eng.model.packed[0]["o"].mxfp4 and eng.model.packed_lm.mxfp4 and not eng.model.packed[0]["qkv"].rope
    rng = np.random.default_rng(0)
    prompts = [rng.integers(3, 1024, size=n).tolist() for n in (40, 70)]
    outs = eng.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))
    assert all(len(r.output) == 6 for r in outs)
    assert eng.stats["graph_replays"] > 0
    _oracle_check(eng, prompts, outs)
    assert eng.sched.check_invariants() == ""


def test_engine_mxfp4_wide_batch_runs_on_the_rounded_bf16_copies():
    from kgs.serve import SamplingParams

    eng = _engine(max_batch=128, num_pages=512, fused_max_batch=128)
    assert eng.model.fused_max_batch == 64
    rng = np.random.default_rng(2)
    prompts = [rng.integers(3, 1024, size=int(n)).tolist() for n in rng.integers(20, 60, size=72)]
    outs = eng.generate(prompts, SamplingParams(max_tokens=4, ignore_eos=True))
    assert all(len(r.output) == 4 for r in outs)
    _oracle_check(eng, prompts[:6] + prompts[-2:], outs[:6] + outs[-2:])
    assert eng.sched.check_invariants() == ""


def test_engine_mxfp4_needs_the_packed_copies():
    from kgs.serve import EngineConfig, LLMEngine

    with pytest.raises(ValueError, match="mxfp4"):
        LLMEngine(_cfg(), EngineConfig(num_pages=64, decode_weights="mxfp4", packed_decode=False), device="cuda",
                  backend="kgs")
