"""Paged prefill attention, CPU tier: the fp32 reference against the gathered
chunk reference, the page-layout facts the kernel's fragment reads rest on, the
plan's host-side validation, the fp8 guard, and the compiled kernel's
resources (hipcc cross-compiles gfx950 without a GPU)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"


def _filled_cache(pages, hkv, table, ctx, seed):
    """A cache layer with ``ctx`` tokens written through ``table`` (ref_cache_write)."""
    from kgs.ops.decode import ref_cache_write

    g = torch.Generator().manual_seed(seed)
    cache = torch.zeros(pages, hkv, 2, 4096, dtype=torch.bfloat16)
    k = torch.randn(ctx, hkv, 128, generator=g).bfloat16()
    v = torch.randn(ctx, hkv, 128, generator=g).bfloat16()
    pos = torch.arange(ctx)
    slots = (table.long()[pos // 32] * 32 + pos % 32).int()
    ref_cache_write(cache, k, v, slots)
    return cache


@pytest.mark.parametrize("ctx0,n,padded", [(0, 100, 128), (64, 77, 128)])
def test_reference_matches_chunk_reference_over_gathered_context(ctx0, n, padded):
    from kgs.ops.decode import ref_gather_kv
    from kgs.ops.transformer import paged_prefill_plan, ref_attention_chunk, ref_paged_prefill_attention

    H, HKV, pages = 4, 2, 12
    g = torch.Generator().manual_seed(ctx0 + n)
    table = torch.randperm(pages, generator=g)[:8].int()  # shuffled: not monotonic
    assert (table[1:] < table[:-1]).any()
    cache = _filled_cache(pages, HKV, table, ctx0 + n, seed=n)
    row0 = 128  # rows in front of the chunk belong to nobody
    qkv = torch.randn(row0 + padded, (H + 2 * HKV) * 128, generator=g).bfloat16()
    plan = paged_prefill_plan([(row0, n, padded, ctx0)], table[None], "cpu")
    out = ref_paged_prefill_attention(qkv, cache, plan, H, HKV)
    assert out.dtype == torch.float32 and out.shape == (row0 + padded, H * 128)
    k, v = ref_gather_kv(cache, table, ctx0 + n)
    want = ref_attention_chunk(qkv[row0:row0 + n], k.reshape(ctx0 + n, -1), v.reshape(ctx0 + n, -1), H, HKV)
    assert (out[row0:row0 + n] - want).abs().max().item() < 1e-5
    assert out[row0:row0 + n].abs().max() > 0.1
    assert (out[row0 + n:] == 0).all() and (out[:row0] == 0).all()


def test_page_layout_feeds_the_kernels_fragments():
    """What attention_paged.hip reads straight out of a page: every 16-byte
    unit of the K region is 8 consecutive dims of one token (unit (tau, c) at
    256 (tau>>4) + 16 c + (tau&15)); V unit (dt, g, m) is dim 16 dt + m of
    tokens {4g..4g+3, 16+4g..16+4g+3}, which is k-step (sp, hh) of a 32-row S^T
    tile whose row i holds token swap34(i), with g = 2 sp + hh."""
    from kgs.ops.decode import kv_index_tables

    k_idx, v_idx = kv_index_tables()
    for tau in range(32):
        for c in range(16):
            unit = 256 * (tau >> 4) + 16 * c + (tau & 15)
            assert k_idx[tau, 8 * c:8 * c + 8].tolist() == list(range(8 * unit, 8 * unit + 8))

    def swap34(i):
        return (i & 7) | ((i & 8) << 1) | ((i & 16) >> 1)

    for dt in range(8):
        for g in range(4):
            for m in range(16):
                unit = 64 * dt + 16 * g + m
                sp, hh = g >> 1, g & 1
                for j in range(8):
                    i = 16 * sp + 8 * (j >> 2) + 4 * hh + (j & 3)  # S^T row of P-fragment slot j
                    tau = swap34(i)
                    assert tau == 4 * g + (j & 3) + 16 * (j >> 2)
                    assert int(v_idx[tau, 16 * dt + m]) == 8 * unit + j


def test_plan_orders_q_blocks_heaviest_first():
    from kgs.ops.transformer import paged_prefill_plan

    chunks = [(0, 128, 128, 0), (128, 40, 128, 0), (256, 300, 384, 128), (640, 5, 128, 640)]
    plan = paged_prefill_plan(chunks, torch.zeros(4, 21, dtype=torch.int32), "cpu")
    assert plan.desc.tolist() == [list(c) for c in chunks] and plan.rows == 768
    qmap = [tuple(r) for r in plan.qmap.tolist()]
    assert sorted(qmap) == [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (3, 0)]

    def tiles(ci, qb):
        _, n, _, ctx0 = chunks[ci]
        return 0 if qb * 128 >= n else min((ctx0 + 128 * (qb + 1)) // 64, -(-(ctx0 + n) // 64))

    w = [tiles(*r) for r in qmap]
    assert w == sorted(w, reverse=True) and w[0] == 11 and qmap[0] == (3, 0)


@pytest.mark.parametrize("chunk,width", [
    ((0, 100, 100, 0), 8),     # padded % 128
    ((0, 100, 128, 32), 8),    # ctx0 % 64
    ((0, 0, 128, 0), 8),       # n == 0
    ((0, 129, 128, 0), 8),     # n > padded
    ((0, 100, 128, 64), 5),    # 164 tokens need 6 pages
])
def test_plan_rejects_contract_violations(chunk, width):
    from kgs.ops.transformer import paged_prefill_plan

    with pytest.raises(ValueError, match=re.escape(str(chunk))):
        paged_prefill_plan([chunk], torch.zeros(1, width, dtype=torch.int32), "cpu")
    ok = (0, 100, 128, 64)
    assert paged_prefill_plan([ok], torch.zeros(1, 6, dtype=torch.int32), "cpu").max_page == 0


def test_engine_refuses_paged_prefill_over_fp8_pages():
    from kgs.models.llama import LlamaConfig
    from kgs.serve import EngineConfig, LLMEngine

    mc = LlamaConfig(hidden=512, intermediate=1024, heads=4, kv_heads=1, layers=1, vocab=256)
    with pytest.raises(ValueError, match="paged_prefill"):
        LLMEngine(mc, EngineConfig(paged_prefill=True, kv_cache_dtype="fp8"), device="cpu", backend="ref")
    assert EngineConfig().paged_prefill is False


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_kernel_resources_allow_two_workgroups_per_cu(tmp_path):
    """No scratch, no spills, and at most 256 registers per lane and 80 KiB of
    LDS per workgroup, so two workgroups (two waves per SIMD) share a CU -- read
    from the code object's metadata in the saved device assembly."""
    src = ROOT / "native" / "kernels" / "attention_paged.hip"
    cmd = [HIPCC if Path(HIPCC).exists() else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
           "-I", str(ROOT / "native" / "kernels"), str(src), "-o", str(tmp_path / "ap.o"), "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    (s_file,) = list(tmp_path.glob("attention_paged-hip-amdgcn-amd-amdhsa-gfx950.s"))
    asm = s_file.read_text()
    meta = asm[asm.index(".amdgpu_metadata"):]
    assert "fwd_paged" in meta

    def field(name):
        vals = re.findall(rf"\.{name}:\s+(\d+)", meta)
        assert len(vals) == 1, (name, vals)  # one kernel in the translation unit
        return int(vals[0])

    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("vgpr_count") + field("agpr_count") <= 256   # 2 waves / SIMD (512 registers per lane)
    assert field("group_segment_fixed_size") <= 80 * 1024     # 2 workgroups / CU (160 KiB)
    assert field("max_flat_workgroup_size") == 256
