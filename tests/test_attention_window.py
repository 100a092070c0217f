"""CPU tests of sliding-window attention: argument checks, the fp32 reference, the torch-backend decoder and the
compile-time resources of native/kernels/attention_window.hip (hipcc cross-compiles gfx950)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.models.decoder import DecoderLayer, DecoderLM
from kgs.ops.transformer import (attention_qkv, attention_qkv_backward, attention_qkv_lse, flash_attention_qkv,
                                 ref_attention_qkv, ref_attention_qkv_backward)

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
SRC = ROOT / "native" / "kernels" / "attention_window.hip"


def _args(hd=128, s=256, nh=2, nkv=1, dt=torch.bfloat16):
    return torch.zeros(s, (nh + 2 * nkv) * hd, dtype=dt), torch.zeros(s, nh * hd, dtype=dt), torch.zeros(nh, s)


def test_window_arguments_are_checked_before_the_device():
    qkv, out, lse = _args()
    calls = [lambda **kw: attention_qkv(qkv, 1, 256, 2, 1, **kw), lambda **kw: attention_qkv_lse(qkv, 1, 256, 2, 1, **kw),
             lambda **kw: flash_attention_qkv(qkv, 1, 256, 2, 1, **kw),
             lambda **kw: attention_qkv_backward(qkv, out, out, lse, 1, 256, 2, 1, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="at least 1"):
            call(window=0)
        with pytest.raises(ValueError, match="causal"):
            call(window=64, causal=False)
        for w in (64, 256, 300):  # the window kernels, and the causal ones for a window that covers seq
            with pytest.raises(ValueError, match="GPU"):
                call(window=w)
    q64, o64, l64 = _args(hd=64)
    for call in (lambda: flash_attention_qkv(q64, 1, 256, 2, 1, head_dim=64, window=64),
                 lambda: attention_qkv_backward(q64, o64, o64, l64, 1, 256, 2, 1, head_dim=64, window=64)):
        with pytest.raises(ValueError, match="128"):
            call()
    with pytest.raises(ValueError, match="GPU"):  # covers seq: the head_dim 64 causal kernels
        flash_attention_qkv(q64, 1, 256, 2, 1, head_dim=64, window=256)


@pytest.mark.parametrize("window", [1, 3, 8, 11])
def test_reference_against_a_brute_force_masked_softmax(window):
    b, s, nh, nkv, hd = 2, 8, 2, 1, 4
    g = torch.Generator().manual_seed(window)
    qkv, dout = (torch.randn(b * s, c * hd, generator=g, dtype=torch.float64) for c in (nh + 2 * nkv, nh))
    leaf = qkv.clone().requires_grad_(True)
    rows = []
    for t in range(b * s):
        bi, i = divmod(t, s)
        for h in range(nh):
            q = leaf[t, h * hd:(h + 1) * hd]
            js = range(max(0, i - window + 1), i + 1)
            sc = torch.stack([q @ leaf[bi * s + j, (nh + h // 2) * hd:(nh + h // 2 + 1) * hd] for j in js]) / hd ** 0.5
            vs = torch.stack([leaf[bi * s + j, (nh + nkv + h // 2) * hd:(nh + nkv + h // 2 + 1) * hd] for j in js])
            rows.append(torch.softmax(sc, 0) @ vs)
    want = torch.stack(rows).reshape(b * s, nh * hd)
    (wgrad,) = torch.autograd.grad(want, leaf, dout)
    assert torch.allclose(ref_attention_qkv(qkv, b, s, nh, nkv, head_dim=hd, window=window).double(), want.detach(), atol=1e-5)
    assert torch.allclose(ref_attention_qkv_backward(qkv, dout, b, s, nh, nkv, head_dim=hd, window=window).double(), wgrad,
                          atol=1e-5)


def test_torch_decoder_layer_applies_the_window_and_the_lm_places_it(monkeypatch):
    dim, nh, nkv, inter, b, s, w = 64, 4, 2, 96, 2, 16, 5
    x = torch.randn(b, s, dim, generator=torch.Generator().manual_seed(0))
    layer = DecoderLayer(dim, nh, nkv, inter, backend="torch", dtype=torch.float32, window=w)
    plain = DecoderLayer(dim, nh, nkv, inter, backend="torch", dtype=torch.float32)
    assert [n for n, _ in layer.named_parameters()] == [n for n, _ in plain.named_parameters()]
    res, out = layer(x)
    pres = plain(x)[0]
    assert not torch.equal(res, pres)
    assert torch.equal(DecoderLayer(dim, nh, nkv, inter, backend="torch", dtype=torch.float32, window=s)(x)[0], pres)
    # the layer without the option (same seeded weights), its attention given the mask densely
    ones = torch.ones(s, s, dtype=torch.bool)
    real = torch.nn.functional.scaled_dot_product_attention
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention",
                        lambda q, k, v, **kw: real(q, k, v, attn_mask=ones.tril() & ~ones.tril(-w)))
    dres, dout = plain(x)
    monkeypatch.undo()
    assert torch.equal(res, dres) and torch.equal(out, dout)

    lm = DecoderLM(32, dim, 6, nh, nkv, inter, backend="torch", dtype=torch.float32, window=w, global_every=3)
    assert [m.window for m in lm.layers] == [w, w, None, w, w, None]
    assert [m.window for m in DecoderLM(32, dim, 2, nh, nkv, inter, backend="torch", window=w).layers] == [w, w]
    assert [m.window for m in DecoderLM(32, dim, 2, nh, nkv, inter, backend="torch").layers] == [None, None]
    for msg, kw in (("causal=True", dict(causal=False, window=w)), ("at least 1", dict(window=0))):
        with pytest.raises(ValueError, match=msg):
            DecoderLayer(dim, nh, nkv, inter, backend="torch", **kw)
    with pytest.raises(ValueError, match="128"):
        DecoderLayer(512, 8, 2, 1024, backend="kgs", window=64)  # head_dim 64
    assert DecoderLayer(512, 4, 2, 1024, backend="kgs", window=64).window == 64


# kernel -> (workgroups per CU, waves per SIMD) its __launch_bounds__ declare
DESIGN = {"fwdILb0": (2, 2), "fwdILb1": (2, 2), "bwd_dkdv": (1, 1), "bwd_dq": (2, 2), "bwd_prep": (1, 1)}


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_kernels_have_no_spills_no_scratch_and_fit_their_declared_occupancy(tmp_path):
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(SRC.parent), str(SRC), "-o", str(tmp_path / "attention_window.o"),
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
    assert len(res) == len(DESIGN), sorted(res)
    for short, (wgs, waves) in DESIGN.items():
        (r,) = [r for n, r in res.items() if re.search(rf"attn_win\d+{short}E", n)]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (short, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512 // waves, (short, r)
        assert r["LDS Size"] <= 160 * 1024 // wgs, (short, r)
