"""MXFP4 weight-only decode (W4A16) on the CPU: the quantiser against an
independent float64 numpy reference, the facts the in-register dequant relies
on, the packed layout's round trip, the serving engine on the reference backend
with ``decode_weights="mxfp4"``, and the cross-compiled kernels' resources."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _ref_quantize(w64: np.ndarray):
    """OCP MX v1.0 MXFP4 in float64 numpy, element by block: nearest grid point
    by explicit distances, ties to the even code; -> (codes [N, K], exps [N, K/32])."""
    n, k = w64.shape
    v = w64.reshape(n, k // 32, 32)
    amax = np.abs(v).max(-1)
    with np.errstate(divide="ignore"):
        ex = np.floor(np.log2(amax)) - 2
    # code * X normal in bf16: 0.5 X >= 2^-126, 6 X < 2^128
    ex = np.where(amax > 0, np.clip(ex, -125, 125), 0).astype(np.int64)
    a = np.abs(v) / np.exp2(ex.astype(np.float64))[..., None]
    d = np.abs(a[..., None] - GRID)  # [..., 8]
    best = d.min(-1, keepdims=True)
    cand = d == best  # one or (at a tie) two adjacent codes
    lo = cand.argmax(-1)
    hi = 7 - cand[..., ::-1].argmax(-1)
    code = np.where(lo % 2 == 0, lo, hi)
    code = np.where(a > 6, 7, code)
    code = code + 8 * np.signbit(v)
    return code.reshape(n, k).astype(np.uint8), (ex + 127).astype(np.uint8)


def _unpack_codes(codes: torch.Tensor) -> np.ndarray:
    c = codes.numpy()
    return np.stack((c & 15, c >> 4), -1).reshape(c.shape[0], -1)


def _gauss(n=768, k=2048, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16)


def _edge_rows():
    """One block per row around X = 2^-3 (amax 0.5 .. < 1), plus scaled copies."""
    x = 0.125
    rows = []

    def row(vals, fill=0.0):
        r = np.full(32, fill)
        r[:len(vals)] = vals
        rows.append(r)

    row([])                                              # zero block -> e 127, codes 0
    row([0.5])                                           # amax a power of two: 4 X
    row([4 * x, 2.5 * x, 5 * x, 0.25 * x, 0.75 * x, 1.25 * x, 1.75 * x, 3.5 * x])   # exact ties
    row([4 * x, -2.5 * x, -5 * x, -0.25 * x, -0.75 * x, -1.25 * x, -1.75 * x, -3.5 * x])
    row([7 * x, 7.5 * x, 6.5 * x, -7 * x, 5.5 * x])      # saturation: 7 X -> 6 X
    row([-0.0, 0.5, -0.0, -0.001])                       # -0 keeps its sign bit
    row([-0.75], fill=-0.0)
    row([2.0 ** -126, 2.0 ** -127, 2.0 ** -130])         # exponent clamp (small)
    row([2.0 ** 127, 2.0 ** 120, -(2.0 ** 126)])         # exponent clamp (large)
    row([3.0, 1.0, 1.1, 2.6, 2.4, 0.9])                  # amax not a power of two
    return np.stack(rows)


def _cases():
    return {"gauss": _gauss().double().numpy(), "edges": torch.tensor(_edge_rows()).to(torch.bfloat16).double().numpy()}


@pytest.mark.parametrize("name", ["gauss", "edges"])
def test_quantiser_matches_float64_reference(name):
    from kgs.ops.decode import mxfp4_quantize

    w64 = _cases()[name]
    codes, exps = mxfp4_quantize(torch.tensor(w64).to(torch.bfloat16))
    assert codes.dtype == torch.uint8 and exps.dtype == torch.uint8
    n, k = w64.shape
    assert tuple(codes.shape) == (n, k // 2) and tuple(exps.shape) == (n, k // 32)
    rc, re_ = _ref_quantize(w64)
    assert np.array_equal(exps.numpy(), re_)
    assert np.array_equal(_unpack_codes(codes), rc)
    assert int(exps.max()) < 255


def test_quantiser_edge_values():
    """The cases spelled out: zero block, ties to even (2.5 X -> 2 X, 5 X -> 4 X),
    saturation (7 X -> 6 X), signs."""
    from kgs.ops.decode import mxfp4_dequantize, mxfp4_quantize

    w = torch.tensor(_edge_rows()).to(torch.bfloat16)
    codes, exps = mxfp4_quantize(w)
    c = _unpack_codes(codes)
    dq = mxfp4_dequantize(codes, exps).double().numpy()
    x = 0.125
    assert exps[0, 0] == 127 and not c[0].any()
    assert exps[1, 0] == 127 - 3 and c[1, 0] == 6                      # 0.5 = 4 X
    assert list(dq[2, :8] / x) == [4, 2, 4, 0, 1, 1, 2, 4]
    assert list(dq[3, :8] / x) == [4, -2, -4, 0, -1, -1, -2, -4]
    assert list(dq[4, :5] / x) == [6, 6, 6, -6, 6]
    assert list(c[5, :4]) == [8, 6, 8, 8] and c[6, 1] == 8
    assert exps[7, 0] == 2 and exps[8, 0] == 252


def test_the_three_facts():
    from kgs.ops.decode import mxfp4_dequantize, mxfp4_quantize

    for w in (_gauss(), torch.tensor(_edge_rows()[:7]).to(torch.bfloat16)):
        codes, exps = mxfp4_quantize(w)
        dq = mxfp4_dequantize(codes, exps)
        assert dq.dtype == torch.bfloat16
        # dq is exactly representable in bf16: the float64 value of code x 2^(e - 127) survives the cast
        lut = np.concatenate([GRID, -GRID])
        exact = lut[_unpack_codes(codes)] * np.exp2(exps.numpy().astype(np.float64) - 127).repeat(32, 1)
        assert np.array_equal(dq.double().numpy(), exact)
        assert np.array_equal(torch.tensor(exact).to(torch.bfloat16).double().numpy(), exact)
        # |w - dq| <= 0.25 x block amax
        n, k = w.shape
        err = (w.double() - dq.double()).abs().reshape(n, k // 32, 32)
        amax = w.double().abs().reshape(n, k // 32, 32).amax(-1, keepdim=True)
        assert bool((err <= 0.25 * amax).all()), float((err / amax.clamp(min=1e-300)).max())
        # idempotent
        c2, e2 = mxfp4_quantize(dq)
        assert torch.equal(c2, codes) and torch.equal(e2, exps)


@pytest.mark.parametrize("swiglu,fold", [(False, False), (True, False), (False, True), (True, True)])
def test_packed_weight_round_trip(swiglu, fold):
    from kgs.ops.decode import PackedWeight, mxfp4_dequantize, mxfp4_quantize

    g = torch.Generator().manual_seed(3)
    n, k = 192, 384
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16)
    f = (1 + 0.25 * torch.randn(k, generator=g)).to(torch.bfloat16) if fold else None
    pw = PackedWeight(w, swiglu=swiglu, fold=f, mxfp4=True)
    assert pw.mxfp4 and not pw.fp8 and (pw.n, pw.k) == (n, k)
    assert pw.data.dtype == torch.uint8 and pw.data.numel() == n * k // 2
    assert pw.wscale.dtype == torch.uint8 and pw.wscale.numel() == n * k // 32
    wf = w.float() * f.float()[None, :] if fold else w
    assert torch.equal(pw.unpacked(), mxfp4_dequantize(*mxfp4_quantize(wf)))


def test_packed_layout_is_the_documented_one():
    """Dword s of lane (g, r) of super-fragment (nt, q) holds the codes of
    W[16 nt + r, 128 q + 32 s + 8 g .. + 8]; scale byte s of row r is k-step 4 q + s."""
    from kgs.ops.decode import mxfp4_quantize, pack_mxfp4

    w = _gauss(32, 256, seed=5)
    codes, exps = mxfp4_quantize(w)
    data, scales = pack_mxfp4(codes, exps)
    assert tuple(data.shape) == (2, 2, 64, 16) and tuple(scales.shape) == (2, 2, 16, 4)
    for nt, q, g, r, s in ((0, 0, 0, 0, 0), (1, 1, 3, 15, 3), (1, 0, 2, 7, 1), (0, 1, 1, 9, 2)):
        k0 = 128 * q + 32 * s + 8 * g
        assert torch.equal(data[nt, q, 16 * g + r, 4 * s:4 * s + 4], codes[16 * nt + r, k0 // 2:k0 // 2 + 4])
        assert scales[nt, q, r, s] == exps[16 * nt + r, 4 * q + s]


def test_packed_weight_rejections():
    from kgs.ops.decode import PackedWeight

    w = _gauss(6 * 128, 256, seed=2)
    with pytest.raises(ValueError, match="mxfp4"):
        PackedWeight(w, mxfp4=True, fp8=True)
    with pytest.raises(ValueError, match="mxfp4"):
        PackedWeight(w, mxfp4=True, rope=(4, 1))
    with pytest.raises(ValueError, match="128"):
        PackedWeight(_gauss(64, 192, seed=2), mxfp4=True)


def test_skinny_config_reads_the_mxfp4_tables():
    from kgs.ops import decode as D

    assert isinstance(D.TUNED_MXFP4, dict) and isinstance(D.TUNED_TINY_MXFP4, dict)
    for (mt, n, k), (v, ks) in D.TUNED_MXFP4.items():
        assert (v <= 12 or v in D.KIN_VARIANTS) and D.SKINNY_VARIANTS[v][1] == mt
        m = 16 * mt
        assert D.skinny_config(m, n, k, mxfp4=True) == (v, ks)
        assert (k // D.skinny_geometry(m, v)[1]) % ks == 0
    # an untuned shape takes the defaults, as bf16 does
    assert D.skinny_config(8, 768, 2048, mxfp4=True) == D.skinny_config(8, 768, 2048)


def _tiny():
    from kgs.models.llama import LlamaConfig

    return LlamaConfig(hidden=256, intermediate=512, heads=2, kv_heads=1, layers=2, vocab=512)


def test_engine_ref_mxfp4_matches_full_recompute():
    pytest.importorskip("kgs._native._serve")
    from kgs.ops.decode import mxfp4_dequantize, mxfp4_quantize
    from kgs.serve import EngineConfig, LLMEngine, SamplingParams

    eng = LLMEngine(_tiny(), EngineConfig(num_pages=64, max_batch=4, max_model_len=512, cuda_graphs=False,
                                          decode_weights="mxfp4"), device="cpu", backend="ref")
    base = LLMEngine(_tiny(), EngineConfig(num_pages=64, max_batch=4, max_model_len=512, cuda_graphs=False),
                     device="cpu", backend="ref")
    ws = [w for lw in eng.model.w for w in lw.values()] + [eng.model.w_lm]
    ws0 = [w for lw in base.model.w for w in lw.values()] + [base.model.w_lm]
    for w, w0 in zip(ws, ws0):
        assert torch.equal(w, mxfp4_dequantize(*mxfp4_quantize(w)))   # a fixed point of the round trip
        assert torch.equal(w, mxfp4_dequantize(*mxfp4_quantize(w0)))  # of the same model's weights
        assert not torch.equal(w, w0)
    assert eng.model.oracle.lm_head.w is eng.model.w_lm  # the oracle shares the rounded tensors
    rng = np.random.default_rng(1)
    prompts = [rng.integers(3, 512, size=n).tolist() for n in (5, 33, 64, 100, 17)]
    outs = eng.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))
    assert all(len(r.output) == 6 and r.finish_reason == "length" for r in outs)
    oracle = eng.model.oracle
    for prompt, req in zip(prompts, outs):
        seq = list(prompt)
        for tok in req.output:
            logits = oracle.forward(torch.tensor([seq]))[0, -1].float()
            assert logits[tok] >= logits.max() - 2e-2 * logits.abs().max(), (len(seq), tok, int(logits.argmax()))
            seq.append(tok)


def test_engine_rejects_unknown_decode_weights():
    pytest.importorskip("kgs._native._serve")
    from kgs.serve import EngineConfig, LLMEngine

    with pytest.raises(ValueError, match="bf16, fp8 or mxfp4"):
        LLMEngine(_tiny(), EngineConfig(num_pages=64, decode_weights="int4"), device="cpu", backend="ref")


def test_page_budget_counts_the_mxfp4_copies(monkeypatch):
    """_pages_from_memory: the decode copies cost 1/4 + 1/64 of the bf16 weights."""
    pytest.importorskip("kgs._native._serve")
    from kgs.models.llama import LlamaConfig
    from kgs.ops.decode import PagedKVCache
    from kgs.serve import EngineConfig, LLMEngine

    mc = LlamaConfig.named("llama3-8b")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (280 << 30, 288 << 30))
    pages = {}
    for dw in ("bf16", "mxfp4"):
        eng = object.__new__(LLMEngine)
        eng.device, eng.backend, eng.cfg = torch.device("cuda"), "kgs", EngineConfig(decode_weights=dw)
        pages[dw] = eng._pages_from_memory(mc)
    h, i, kvd = mc.hidden, mc.intermediate, mc.kv_heads * mc.head_dim
    weights = 2 * (mc.layers * (h * (h + 2 * kvd) + h * h + 3 * h * i) + 2 * mc.vocab * h)
    saved = weights * (1 - 0.25 - 1 / 64)
    per_page = PagedKVCache.bytes_per_page(mc.layers, mc.kv_heads, "bf16")
    assert abs((pages["mxfp4"] - pages["bf16"]) - saved * EngineConfig().kv_fraction / per_page) <= 1


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_mxfp4_kernels_have_no_scratch_and_dequantise_in_registers(tmp_path):
    """Every mxfp4 ``skinny`` instantiation (variants 1-12, 20, 21): no scratch,
    no spills, registers within its ``__launch_bounds__`` (512 per lane at one
    workgroup of 4 waves per CU, 256 at two), and the fp4 -> bf16 conversion
    instruction in its body -- read from the saved device assembly."""
    src = ROOT / "native" / "kernels" / "decode.hip"
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(ROOT / "native" / "kernels"), str(src), "-o", str(tmp_path / "d.o"), "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    (s_file,) = list(tmp_path.glob("decode-hip-amdgcn-amd-amdhsa-gfx950.s"))
    asm = s_file.read_text()
    meta = asm[asm.index(".amdgpu_metadata"):]
    # skinny<R, MT, KC, WF = 2 (mxfp4), EROPE, KIN>
    name = re.compile(r"_ZN3kgs3dec6skinnyILi(\d+)ELi(\d+)ELi(\d+)ELi2ELb0ELb([01])EEE\w+")
    seen = set()
    for entry in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", entry)
        nm = name.fullmatch(m.group(1)) if m else None
        if nm is None:
            continue
        r, mt, kc, kin = (int(t) for t in nm.groups())
        seen.add((r, mt, kc, kin))

        def field(f, entry=entry):
            (v,) = re.findall(rf"\.{f}:\s+(\d+)", entry)
            return int(v)

        assert field("private_segment_fixed_size") == 0, nm.group(0)
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, nm.group(0)
        occupancy = 1 if (mt * kc > 32 or r * mt >= 16) else 2  # the kernel's __launch_bounds__(256, occupancy)
        assert field("vgpr_count") + field("agpr_count") <= 512 // occupancy, nm.group(0)
        assert field("group_segment_fixed_size") <= 160 * 1024 // occupancy, nm.group(0)
        body = asm[asm.index(nm.group(0) + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert body.count("v_cvt_scalef32_pk_bf16_fp4") >= 4 * r, nm.group(0)
        assert "v_mfma_f32_16x16x32_bf16" in body
    from kgs.ops.decode import KIN_VARIANTS, SKINNY_VARIANTS

    want = {(r, mt, kc, int(v in KIN_VARIANTS)) for v, (r, mt, kc) in SKINNY_VARIANTS.items()
            if v <= 12 or v in KIN_VARIANTS}
    assert seen == want
