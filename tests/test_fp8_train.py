"""The fp8 training Linear without a GPU: the torch model of the recipe
(``ref_linear_fp8``) against the formulas and against fp32, what autograd saves,
the decoder's ``linear="fp8"`` option, argument checks that fire before the
native library is touched, and the new kernels' compile-time resources."""
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.ops import fp8_amax, fp8_quantize, linear_fp8, ref_linear_fp8
from kgs.ops.fp8_train import FP8_DTYPE, LinearFp8, RefLinearFp8, ref_quantize, ref_scale

# relative Frobenius error of the model against the fp32 products of the same
# bf16 inputs at (512, 512, 768), as first recorded on a CPU (the README of
# profiles/r14/fp8_linear); the test allows 1.5 x for another seed / matmul order
RECORDED = {"y": 0.0372, "dx": 0.0373, "dw": 0.0374}


def _bf(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16()


def _fro(got, ref):
    return ((got.float() - ref).norm() / ref.norm()).item()


def test_model_quantisers_follow_the_formula():
    x = _bf(64, 96, seed=1, scale=3.0)
    x[5] = 0  # an all-zero row
    xf = x.float()
    for amax, shape in ((xf.abs().amax(dim=1), (64, 1)), (xf.abs().amax(dim=0), (1, 96)), (xf.abs().amax(), (1, 1))):
        s = ref_scale(amax).reshape(shape)
        assert torch.equal(s, (amax.clamp(min=1e-12) / 448).reshape(shape))
        q = ref_quantize(xf, s)
        assert q.dtype == FP8_DTYPE
        deq = q.float() * s
        assert torch.all((deq - xf).abs() <= 2.0 ** -4 * xf.abs() + 2 * s * 2.0 ** -9)
    s = ref_scale(xf.abs().amax(dim=1))
    q = ref_quantize(xf, s[:, None])
    assert torch.isfinite(s).all() and s[5] > 0
    assert torch.all(q[5].view(torch.uint8) == 0)
    # a non-finite amax gives a non-finite scale (fmaxf would have hidden the NaN)
    assert torch.isnan(ref_scale(torch.tensor(float("nan"))))
    assert torch.isinf(ref_scale(torch.tensor(float("inf"))))


def test_model_against_fp32_products():
    T, K, N = 512, 512, 768
    x, w, dy = _bf(T, K, seed=2), _bf(N, K, seed=3, scale=K ** -0.5), _bf(T, N, seed=4)
    x.requires_grad_(True)
    w.requires_grad_(True)
    y = ref_linear_fp8(x, w)
    y.backward(dy)
    xf, wf, df = x.detach().float(), w.detach().float(), dy.float()
    err = {"y": _fro(y.detach(), xf @ wf.T), "dx": _fro(x.grad, df @ wf), "dw": _fro(w.grad, df.T @ xf)}
    print("ref_linear_fp8 against fp32, relative Frobenius error:", err)
    for k, e in err.items():
        assert e < 1.5 * RECORDED[k], (k, e)


def test_model_bias_and_its_gradient():
    x, w, b = _bf(32, 48, seed=5), _bf(64, 48, seed=6), _bf(64, seed=7)
    b.requires_grad_(True)
    y = ref_linear_fp8(x, w, b)
    y0 = ref_linear_fp8(x, w)
    assert _fro(y.detach(), y0.float() + b.detach().float()) < 2.0 ** -7
    dy = _bf(32, 64, seed=8)
    y.backward(dy)
    assert torch.equal(b.grad, dy.float().sum(0).bfloat16())


def test_autograd_saves_no_bf16_copy_of_x_and_honours_needs_input_grad():
    T, K, N = 32, 48, 64
    x, w = _bf(T, K, seed=9).requires_grad_(True), _bf(N, K, seed=10).requires_grad_(True)
    y = ref_linear_fp8(x, w)
    saved = y.grad_fn.saved_tensors
    assert not any(t.dtype == torch.bfloat16 and tuple(t.shape) in ((T, K), (K, T)) for t in saved)
    x8t = [t for t in saved if t.dtype == FP8_DTYPE]
    assert len(x8t) == 1 and tuple(x8t[0].shape) == (K, T)  # one byte per element of x
    assert any(t is w or t.data_ptr() == w.data_ptr() for t in saved)  # w itself: the version check guards it
    y.backward(_bf(T, N, seed=11))
    assert x.grad is not None and w.grad is not None

    # dX only: no transposed image of x is made or kept
    x1, w1 = x.detach().clone().requires_grad_(True), w.detach().clone()
    y1 = ref_linear_fp8(x1, w1)
    assert not any(t.dtype == FP8_DTYPE for t in y1.grad_fn.saved_tensors)
    y1.backward(_bf(T, N, seed=11))
    assert torch.equal(x1.grad, x.grad) and w1.grad is None

    # dW only
    x2, w2 = x.detach().clone(), w.detach().clone().requires_grad_(True)
    y2 = ref_linear_fp8(x2, w2)
    y2.backward(_bf(T, N, seed=11))
    assert torch.equal(w2.grad, w.grad) and x2.grad is None

    # a weight changed in place between forward and backward is caught
    y3 = ref_linear_fp8(x, w)
    with torch.no_grad():
        w.add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y3.backward(_bf(T, N, seed=11))


def test_nonfinite_values_stay_visible_in_the_model():
    T, K, N = 32, 48, 64
    x, w, dy = _bf(T, K, seed=12), _bf(N, K, seed=13), _bf(T, N, seed=14)
    xi = x.clone()
    xi[3, 7] = float("inf")
    assert not torch.isfinite(ref_linear_fp8(xi, w)[3]).all()
    x.requires_grad_(True)
    w.requires_grad_(True)
    dy[4, 9] = float("nan")
    ref_linear_fp8(x, w).backward(dy)
    assert not torch.isfinite(x.grad[4]).any()
    assert not torch.isfinite(w.grad[9]).any()


def test_decoder_layer_takes_linear_fp8():
    from kgs.models.decoder import DecoderLayer, DecoderLM

    assert DecoderLayer(64, 2, 1, 96, backend="torch").linear == "bf16"
    assert isinstance(DecoderLayer(64, 2, 1, 96, backend="torch").qkv, torch.nn.Linear)
    with pytest.raises(ValueError, match="linear"):
        DecoderLayer(64, 2, 1, 96, backend="torch", linear="fp4")
    layer = DecoderLayer(64, 2, 1, 96, backend="torch", linear="fp8")
    base = DecoderLayer(64, 2, 1, 96, backend="torch")
    for name in ("qkv", "o", "gate_up", "down"):
        assert isinstance(getattr(layer, name), RefLinearFp8)
        assert torch.equal(getattr(layer, name).weight, getattr(base, name).weight)  # the same seeded weights
    x = _bf(2, 16, 64, seed=15).requires_grad_(True)
    res, out = layer(x)
    (res.float().sum() + out.float().square().sum()).backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    for p in layer.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    o0 = base(x.detach())[1]
    assert _fro(out.detach(), o0.float()) < 0.2  # fp8 noise, not another function

    lm = DecoderLM(128, 64, 2, 2, 1, 96, backend="torch", linear="fp8")
    assert lm.linear == "fp8" and isinstance(lm.head, torch.nn.Linear)
    assert all(isinstance(layer.down, RefLinearFp8) for layer in lm.layers)
    tok = torch.randint(0, 128, (2, 16), generator=torch.Generator().manual_seed(0))
    loss = lm.loss(tok, tok.roll(-1, 1))
    loss.backward()
    assert torch.isfinite(loss)
    assert DecoderLM(128, 64, 1, 2, 1, 96, backend="torch").linear == "bf16"


@pytest.fixture
def no_native(monkeypatch):
    from kgs.ops import _lib

    def boom():
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(_lib, "lib", boom)


def test_raw_ops_check_their_arguments(no_native):
    x = _bf(32, 48)
    v = torch.zeros
    with pytest.raises(TypeError):
        fp8_amax(x.float(), rows=True)
    with pytest.raises(ValueError, match="16"):
        fp8_amax(_bf(24, 48), rows=True)
    with pytest.raises(ValueError, match="16"):
        fp8_amax(_bf(32, 40), rows=True)
    with pytest.raises(ValueError, match="row-major"):
        fp8_amax(_bf(48, 32).T, rows=True)
    with pytest.raises(ValueError, match="stride"):
        fp8_amax(_bf(32, 52)[:, :48], rows=True)  # ld % 8
    with pytest.raises(ValueError, match="at least one"):
        fp8_amax(x)
    with pytest.raises(ValueError, match="GPU"):
        fp8_amax(x, rows=True)

    with pytest.raises(TypeError):
        fp8_quantize(x.float(), tensor_amax=v(1))
    with pytest.raises(TypeError):
        fp8_quantize(x, tensor_amax=v(1).double())
    with pytest.raises(TypeError):
        fp8_quantize(x, tensor_amax=v(1), y=torch.zeros(32, 48, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least one"):
        fp8_quantize(x, tensor_amax=v(1), y=False, yt=False)
    with pytest.raises(ValueError, match="row_amax or tensor_amax"):
        fp8_quantize(x, col_amax=v(48))
    with pytest.raises(ValueError, match="col_amax or tensor_amax"):
        fp8_quantize(x, row_amax=v(32), y=False, yt=True)
    with pytest.raises(ValueError, match="32 floats"):
        fp8_quantize(x, row_amax=v(48))
    with pytest.raises(ValueError, match="1 floats"):
        fp8_quantize(x, tensor_amax=v(1), y_fold=v(2))
    with pytest.raises(ValueError):
        fp8_quantize(x, tensor_amax=v(1), y=torch.zeros(48, 32).to(FP8_DTYPE))  # y is [rows, cols]
    with pytest.raises(ValueError, match="multiple of 16"):
        fp8_quantize(x, tensor_amax=v(1), y=torch.zeros(32, 56).to(FP8_DTYPE)[:, :48])
    with pytest.raises(ValueError, match="GPU"):
        fp8_quantize(x, tensor_amax=v(1))


def test_linear_fp8_checks_its_arguments(no_native):
    x, w = _bf(32, 48), _bf(64, 48)
    with pytest.raises(TypeError):
        linear_fp8(x.float(), w)
    with pytest.raises(TypeError):
        linear_fp8(x, w.float())
    with pytest.raises(TypeError):
        linear_fp8(x, w, torch.zeros(64))
    with pytest.raises(ValueError, match="inner"):
        linear_fp8(x, _bf(64, 32))
    for bad in ((_bf(24, 48), w), (_bf(32, 40), _bf(64, 40)), (x, _bf(72, 48))):
        with pytest.raises(ValueError, match="no bf16 fallback"):
            linear_fp8(*bad)
    with pytest.raises(ValueError, match="length N"):
        linear_fp8(x, w, _bf(48))
    with pytest.raises(ValueError, match="GPU"):
        linear_fp8(x, w)
    lin = LinearFp8(48, 64, bias=True)
    assert lin.weight.dtype == torch.bfloat16 and tuple(lin.weight.shape) == (64, 48) and lin.bias is not None
    assert LinearFp8(48, 64).bias is None
    with pytest.raises(ValueError, match="GPU"):
        lin(_bf(2, 16, 48))


def test_names_are_reachable_from_kgs_ops():
    import kgs.ops

    for name in ("fp8_amax", "fp8_quantize", "linear_fp8", "LinearFp8", "ref_linear_fp8"):
        assert callable(getattr(kgs.ops, name))
    from kgs.ops import _lib

    assert {"kgs_fp8_amax_bf16", "kgs_fp8_quant_bf16"} <= set(_lib._SIGS)
    assert len(_lib._SIGS["kgs_fp8_amax_bf16"][0]) == 8 and len(_lib._SIGS["kgs_fp8_quant_bf16"][0]) == 16


def test_fp8_train_kernels_use_no_scratch(tmp_path):
    """Every kernel of fp8_train.hip, cross-compiled for gfx950: no scratch, no
    spilled VGPR (the quantise kernel holds a 128 x 128 tile's 8 chunks per thread)."""
    root = Path(__file__).resolve().parents[1]
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", str(root / "native/kernels"),
                          str(root / "native/kernels/fp8_train.hip"), "-o", str(tmp_path / "fp8_train.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600,
                         cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    # zero, amax (one tile per workgroup / looping), 3 x quantise
    assert len(res) == 6 and sum("quant_tile" in n for n in res) == 3 and sum("amax_tile" in n for n in res) == 2, res
    assert all("ScratchSize" in r and "VGPRs Spill" in r and "VGPRs" in r for r in res.values()), res
    bad = {n: r for n, r in res.items() if r["ScratchSize"] or r["VGPRs Spill"]}
    assert not bad, bad
    # one workgroup per tile: four waves per SIMD at least. The looping amax kernel's grid is capped at two
    # workgroups per CU (two waves per SIMD), which 256 VGPRs allow.
    assert all(r["VGPRs"] <= (256 if "amax_tileILb1" in n else 128) for n, r in res.items()), res
