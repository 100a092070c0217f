"""CPU tests of the batched expert GEMM (kgs/ops/moe.py, native/kernels/moe_gemm.hip): the float64
reference against a per-expert loop, the argument checks, the kernels' compile-time resources."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.ops import moe

HIPCC = "/opt/rocm/bin/hipcc"
SRC = Path(__file__).resolve().parents[1] / "native" / "kernels" / "moe_gemm.hip"


@pytest.mark.parametrize("mode", [None, "rows", "reduce"])
def test_reference_against_a_per_expert_loop(mode):  # counts 0, 1, inside, the limit, past it; NaN where excluded
    num, m, n, k = 5, 6, 4, 7
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(num, m, k, generator=g, dtype=torch.float64), torch.randn(num, n, k, generator=g, dtype=torch.float64)
    counts = None if mode is None else torch.tensor([0, 1, 3, m if mode == "rows" else k, 50], dtype=torch.int32)
    want = []
    for e in range(num):
        c = None if mode is None else min(int(counts[e]), m if mode == "rows" else k)
        if mode == "rows":
            a[e, c:] = float("nan")
            want.append(torch.cat((a[e, :c] @ b[e].T, torch.zeros(m - c, n, dtype=torch.float64))))
        elif mode == "reduce":
            a[e, :, c:] = b[e, :, c:] = float("nan")
            want.append(a[e, :, :c] @ b[e, :, :c].T)
        else:
            want.append(a[e] @ b[e].T)
    assert torch.allclose(moe.ref_moe_gemm(a, b, counts, mode), torch.stack(want), rtol=0, atol=1e-12)


def test_bad_arguments_are_rejected_before_the_device_check():
    a, b = torch.zeros(2, 128, 64, dtype=torch.bfloat16), torch.zeros(2, 128, 64, dtype=torch.bfloat16)
    counts = torch.zeros(2, dtype=torch.int32)
    w, xe = torch.zeros(3, 128, 128, dtype=torch.bfloat16), torch.zeros(2 * 128, 128, dtype=torch.bfloat16)
    for exc, match, call in (
            (ValueError, "GPU", lambda: moe.moe_gemm(a, b)),
            (ValueError, "GPU", lambda: moe.moe_gemm(a, b, counts, "reduce")),
            (TypeError, "bf16", lambda: moe.moe_gemm(a.float(), b)),
            (TypeError, "int32", lambda: moe.moe_gemm(a, b, counts.long(), "rows")),
            (ValueError, "mode", lambda: moe.moe_gemm(a, b, counts, "cols")),
            (ValueError, "go together", lambda: moe.moe_gemm(a, b, counts)),
            (ValueError, "multiples", lambda: moe.moe_gemm(a[:, :64], b)),
            (ValueError, "agree", lambda: moe.moe_gemm(a, b[:, :, :32])),
            (ValueError, "agree", lambda: moe.moe_gemm(a[:1], b)),
            (ValueError, "unit column stride", lambda: moe.moe_gemm(a[:, :, ::2], b)),
            (ValueError, "unit column stride", lambda: moe.moe_gemm(a[0], b[0])),
            (ValueError, "out must be", lambda: moe.moe_gemm(a, b, out=torch.zeros(2, 128, 256, dtype=torch.bfloat16))),
            (ValueError, "batch stride", lambda: moe.moe_gemm(a, b, out=torch.zeros(128, 128, dtype=torch.bfloat16).expand(2, -1, -1))),
            (ValueError, "tile", lambda: moe.moe_gemm(a, b, tile=1)),
            (ValueError, "GPU", lambda: moe.moe_linear(xe, [w[0], w[1]], counts)),
            (ValueError, "consecutive", lambda: moe.moe_linear(xe, [w[0], w[2]], counts)),
            (ValueError, "consecutive", lambda: moe.moe_linear(xe, [w[0], w[1].clone()], counts)),
            (ValueError, "multiples", lambda: moe.moe_linear(xe[:192], [w[0], w[1]], counts))):
        with pytest.raises(exc, match=match):
            call()


def test_a_batched_module_restacks_its_weights_when_moved():
    from kgs.models.moe import MoEFFN

    m, loop = (MoEFFN(128, 128, 8, expert_gemm=g) for g in ("batched", "loop"))
    params = list(m.parameters())
    m.float().bfloat16()  # Module._apply replaces every Parameter's data on its own
    assert all(p is q for p, q in zip(m.parameters(), params))
    assert moe._stacked([blk.down.weight for blk in m.experts]).shape == (8, 128, 128)
    with pytest.raises(ValueError, match="batched"):
        moe._stacked([blk.down.weight for blk in loop.experts])


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_kernels_have_no_spills_and_no_scratch(tmp_path):
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(SRC.parent), str(SRC), "-o", str(tmp_path / "moe_gemm.o"),
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
    kernels = {n: r for n, r in res.items() if "moe_gemm_nt" in n}  # both tile shapes
    assert len(kernels) == 2 and all(r["VGPRs Spill"] == r["SGPRs Spill"] == r["ScratchSize"] == 0
                                     for r in kernels.values()), kernels
