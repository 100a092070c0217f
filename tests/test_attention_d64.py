"""CPU tests of head_dim 64 attention: the argument checks of the ops, the
models that now take 64-wide heads on the kgs backend, and the compile-time
resources of native/kernels/attention_d64.hip (hipcc cross-compiles gfx950)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.ops.transformer import attention_qkv_backward, attention_qkv_lse, flash_attention_qkv

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
SRC = ROOT / "native" / "kernels" / "attention_d64.hip"


def _args(b=1, s=128, nh=2, nkv=1, dtype=torch.bfloat16):
    return (torch.zeros(b * s, (nh + 2 * nkv) * 64, dtype=dtype), torch.zeros(b * s, nh * 64, dtype=dtype),
            torch.zeros(b * nh, s))


def test_well_formed_cpu_tensors_reach_the_device_check():
    qkv, out, lse = _args()
    with pytest.raises(ValueError, match="GPU"):
        flash_attention_qkv(qkv, 1, 128, 2, 1, head_dim=64)
    with pytest.raises(ValueError, match="GPU"):
        flash_attention_qkv(qkv.clone().requires_grad_(True), 1, 128, 2, 1, head_dim=64)
    with pytest.raises(ValueError, match="GPU"):
        attention_qkv_lse(qkv, 1, 128, 2, 1, head_dim=64)
    with pytest.raises(ValueError, match="GPU"):
        attention_qkv_backward(qkv, out, out, lse, 1, 128, 2, 1, head_dim=64)


def test_bad_arguments_are_rejected_at_head_dim_64():
    qkv, out, lse = _args()
    for fn in (flash_attention_qkv, attention_qkv_lse):
        with pytest.raises(TypeError):
            fn(qkv.float(), 1, 128, 2, 1, head_dim=64)
        with pytest.raises(ValueError, match="128"):
            fn(torch.zeros(192, 256, dtype=torch.bfloat16), 1, 192, 2, 1, head_dim=64)  # seq % 128
        with pytest.raises(ValueError, match="kv_heads"):
            fn(qkv, 1, 128, 3, 2, head_dim=64)
        with pytest.raises(ValueError, match="shape"):
            fn(qkv, 1, 128, 4, 1, head_dim=64)  # columns
        with pytest.raises(ValueError, match="64 or 128"):
            fn(qkv, 1, 128, 2, 1, head_dim=32)
    with pytest.raises(ValueError, match="out shape"):
        attention_qkv_backward(qkv, out[:, :64], out, lse, 1, 128, 2, 1, head_dim=64)
    with pytest.raises(ValueError, match="dqkv shape"):
        attention_qkv_backward(qkv, out, out, lse, 1, 128, 2, 1, dqkv=qkv[:, :192], head_dim=64)


def test_models_take_64_wide_heads_on_the_kgs_backend():
    from kgs.models.attn_block import AttentionBlock
    from kgs.models.decoder import DecoderLayer

    assert AttentionBlock(512, 8, 2, backend="kgs").head_dim == 64
    assert DecoderLayer(512, 8, 2, 1024, backend="kgs").head_dim == 64
    for make in (lambda **kw: AttentionBlock(512, 8, 2, backend="kgs", **kw),
                 lambda **kw: DecoderLayer(512, 8, 2, 1024, backend="kgs", **kw)):
        with pytest.raises(ValueError, match="qk_norm"):
            make(qk_norm=True)
    with pytest.raises(ValueError, match="64 or 128"):
        AttentionBlock(64, 4, 2, backend="kgs")  # head_dim 16
    with pytest.raises(ValueError, match="64 or 128"):
        DecoderLayer(64, 4, 2, 96, backend="kgs")


# kernel -> (workgroups per CU, waves per SIMD) its __launch_bounds__ declare
DESIGN = {"fwdILb0": (2, 2), "fwdILb1": (2, 2), "bwd_dkdv": (2, 2), "bwd_dq": (2, 2), "bwd_prep": (1, 1)}


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_kernels_have_no_spills_no_scratch_and_fit_their_declared_occupancy(tmp_path):
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(SRC.parent), str(SRC), "-o", str(tmp_path / "attention_d64.o"),
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
    for short, (wgs, waves) in DESIGN.items():
        (r,) = [r for n, r in res.items() if re.search(rf"attn64\d+{short}E", n)]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (short, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512 // waves, (short, r)
        assert r["LDS Size"] <= 160 * 1024 // wgs, (short, r)
