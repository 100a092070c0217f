"""Paged prefill attention on the GPU (native/kernels/attention_paged.hip):
prompt chunks attend over the bf16 KV pages in place, all chunks of a step in
one launch. Against the fp32 reference at the project's tolerance for this
math (test_attention_chunk_matches_reference: max abs error / max abs
reference < 2e-2), with stale pages and slots poisoned, and through the engine
with the gather path made to raise."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TOL = 2e-2
POISON = 1e4


def _rel_err(out, ref):
    return ((out.float() - ref).abs().max() / ref.abs().max()).item()


def _setup(chunks, H, HKV, seed, extra=2):
    """``chunks``: (n, padded, ctx0) per chunk, packed from row 128 on. A cache
    that is POISON everywhere except the chunks' real tokens (so the unused
    slots of every last page are poison), each sequence on its own shuffled
    pages, every table entry past a sequence's pages pointing at one all-poison
    page. Returns (qkv, cache, plan, host chunk list, table)."""
    from kgs.ops.decode import ref_cache_write
    from kgs.ops.transformer import paged_prefill_plan

    g = torch.Generator(device="cuda").manual_seed(seed)
    need = [-(-(ctx0 + n) // 32) for n, _, ctx0 in chunks]
    pages = sum(need) + 3
    perm = torch.randperm(pages, generator=torch.Generator().manual_seed(seed)).tolist()
    poison, perm = perm[0], perm[1:]
    width = max(need) + extra
    table = torch.full((len(chunks), width), poison, dtype=torch.int32)
    cache = torch.full((pages, HKV, 2, 4096), POISON, dtype=torch.bfloat16, device="cuda")
    desc, row = [], 128
    for ci, (n, padded, ctx0) in enumerate(chunks):
        mine, perm = perm[:need[ci]], perm[need[ci]:]
        if need[ci] > 1 and mine == sorted(mine):
            mine = mine[::-1]
        table[ci, :need[ci]] = torch.tensor(mine, dtype=torch.int32)
        ctx = ctx0 + n
        k = torch.randn(ctx, HKV, 128, device="cuda", generator=g).bfloat16()
        v = torch.randn(ctx, HKV, 128, device="cuda", generator=g).bfloat16()
        pos = torch.arange(ctx)
        slots = (table[ci].long()[pos // 32] * 32 + pos % 32).int().cuda()
        ref_cache_write(cache, k, v, slots)
        desc.append((row, n, padded, ctx0))
        row += padded
    # q sits at the front of wider fused rows: row stride (H + 2 HKV) * 128
    qkv = torch.randn(row, (H + 2 * HKV) * 128, device="cuda", generator=g).bfloat16()
    return qkv, cache, paged_prefill_plan(desc, table, "cuda"), desc, table


def _check_rows(out, ref, desc):
    """Tolerance on every chunk's real rows, exact zeros after them, finite."""
    for row0, n, padded, _ in desc:
        assert torch.isfinite(out[row0:row0 + padded].float()).all()  # rows of no chunk are not the op's
        assert _rel_err(out[row0:row0 + n], ref[row0:row0 + n]) < TOL, (row0, n, _rel_err(out[row0:row0 + n],
                                                                                         ref[row0:row0 + n]))
        assert (out[row0 + n:row0 + padded] == 0).all()


SINGLE = [(128, 128, 0), (128, 77, 64), (256, 200, 192), (128, 1, 1024), (384, 300, 128)]


@pytest.mark.parametrize("H,HKV", [(4, 1), (8, 8), (32, 8)])
@pytest.mark.parametrize("padded,n,ctx0", SINGLE)
def test_single_chunk_matches_reference(padded, n, ctx0, H, HKV):
    from kgs.ops.transformer import paged_prefill_attention, ref_paged_prefill_attention

    qkv, cache, plan, desc, table = _setup([(n, padded, ctx0)], H, HKV, seed=padded + n + ctx0 + H)
    need = -(-(ctx0 + n) // 32)
    if need > 1:
        assert (table[0, 1:need] < table[0, :need - 1]).any()  # not monotonic
    out = torch.full((qkv.shape[0], H * 128), 7.0, dtype=torch.bfloat16, device="cuda")
    paged_prefill_attention(qkv, cache, plan, H, HKV, out=out)
    ref = ref_paged_prefill_attention(qkv, cache, plan, H, HKV)
    _check_rows(out, ref, desc)
    assert (out[:128] == 7.0).all()  # rows of no chunk are left alone
    again = paged_prefill_attention(qkv, cache, plan, H, HKV)
    assert torch.equal(again[128:], out[128:])


def test_table_no_wider_than_the_context_with_an_odd_page_count():
    """141 tokens = 5 pages = 3 key tiles: the last tile's second page lies
    past a 5-entry table and must not be looked up there."""
    from kgs.ops.transformer import paged_prefill_attention, ref_paged_prefill_attention

    qkv, cache, plan, desc, table = _setup([(77, 128, 64)], 4, 1, seed=5, extra=0)
    assert table.shape[1] == 5
    out = paged_prefill_attention(qkv, cache, plan, 4, 1)
    _check_rows(out, ref_paged_prefill_attention(qkv, cache, plan, 4, 1), desc)


@pytest.fixture(scope="module")
def step():
    """One step of four chunks (n, ctx0) = (128, 0), (40, 0), (300, 128),
    (5, 640) on disjoint pages of one cache, H/HKV 4/1, and its fp32 reference."""
    from kgs.ops.transformer import ref_paged_prefill_attention

    qkv, cache, plan, desc, table = _setup([(128, 128, 0), (40, 128, 0), (300, 384, 128), (5, 128, 640)], 4, 1, seed=9)
    return qkv, cache, plan, desc, table, ref_paged_prefill_attention(qkv, cache, plan, 4, 1)


def test_one_launch_for_several_chunks_equals_one_launch_each(step):
    from kgs.ops.transformer import paged_prefill_attention, paged_prefill_plan

    qkv, cache, plan, desc, table, ref = step
    assert plan.qmap.shape[0] == 6
    out = paged_prefill_attention(qkv, cache, plan, 4, 1)
    _check_rows(out, ref, desc)
    for ci, ch in enumerate(desc):
        alone = paged_prefill_attention(qkv, cache, paged_prefill_plan([ch], table[ci:ci + 1], "cuda"), 4, 1)
        assert torch.equal(alone[ch[0]:ch[0] + ch[2]], out[ch[0]:ch[0] + ch[2]]), ci


def test_parent_path_and_paged_path_both_within_tolerance(step):
    """gather_kv + attention_chunk on the same inputs. Not bitwise equal to the
    paged kernel: the key order inside a tile differs."""
    from kgs.ops.decode import gather_kv
    from kgs.ops.transformer import attention_chunk, paged_prefill_attention

    qkv, cache, plan, desc, table, ref = step
    out = paged_prefill_attention(qkv, cache, plan, 4, 1)
    tbl = table.cuda()
    for ci, (row0, n, padded, ctx0) in enumerate(desc):
        k, v = gather_kv(cache, tbl[ci], ctx0 + n, rows=ctx0 + padded)
        parent = attention_chunk(qkv[row0:row0 + padded], k, v, 4, 1)
        assert _rel_err(parent[:n], ref[row0:row0 + n]) < TOL
        assert _rel_err(out[row0:row0 + n], ref[row0:row0 + n]) < TOL


def test_graph_capture_replays_bitwise(step):
    from kgs.ops.transformer import paged_prefill_attention

    qkv, cache, plan, desc, _, _ = step
    eager = paged_prefill_attention(qkv, cache, plan, 4, 1)
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        paged_prefill_attention(qkv, cache, plan, 4, 1, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        paged_prefill_attention(qkv, cache, plan, 4, 1, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for row0, _, padded, _ in desc:
            assert torch.equal(out[row0:row0 + padded], eager[row0:row0 + padded])


def test_rejects_fp8_pages_and_bad_scalars(step):
    from kgs.ops import KernelError, _lib
    from kgs.ops.decode import FP8
    from kgs.ops.transformer import paged_prefill_attention

    qkv, cache, plan, _, _, _ = step
    with pytest.raises(TypeError):
        paged_prefill_attention(qkv, cache.to(FP8), plan, 4, 1)
    out = torch.empty((qkv.shape[0], 512), dtype=torch.bfloat16, device="cuda")
    args = [qkv.data_ptr(), cache.data_ptr(), plan.block_tables.data_ptr(), plan.desc.data_ptr(), plan.qmap.data_ptr(),
            out.data_ptr(), 4, 6, 4, 1, 128, plan.block_tables.shape[1], qkv.stride(0), 512, 0.1, 0]
    fn = _lib.lib().kgs_attn_prefill_paged_bf16
    # KGS_ERR_SHAPE: H % HKV, head_dim, ldq < H * 128; KGS_ERR_ALIGN: ldq % 8, a q pointer off 16 bytes.
    # Every one returns before the launch.
    for i, v, rc in ((9, 3, -1), (10, 64, -1), (12, 500, -1), (12, qkv.stride(0) + 4, -2), (0, qkv.data_ptr() + 2, -2)):
        bad = list(args)
        bad[i] = v
        assert fn(*bad) == rc, (i, v)
    with pytest.raises(KernelError):
        _lib.check(fn(*args[:9], 3, *args[10:]), "paged_prefill_attention")


# --- the engine on the paged route -----------------------------------------------
# (_cfg, _engine, _oracle_check as in test_serve_gpu.py)

def _cfg():
    from kgs.models.llama import LlamaConfig

    return LlamaConfig(hidden=512, intermediate=1024, heads=4, kv_heads=1, layers=2, vocab=1024)


def _engine(graphs, **kw):
    from kgs.serve import EngineConfig, LLMEngine

    ec = EngineConfig(num_pages=256, max_batch=kw.pop("max_batch", 8), max_model_len=1024, cuda_graphs=graphs, **kw)
    return LLMEngine(_cfg(), ec, device="cuda", backend="kgs")


def _oracle_check(eng, prompts, outs, tol=3e-2):
    oracle = eng.model.oracle
    oracle_ref = type(oracle)(oracle.cfg, device="cuda", backend="torch", seed=0)
    for prompt, req in zip(prompts, outs):
        seq = list(prompt)
        for tok in req.output:
            logits = oracle_ref.forward(torch.tensor([seq], device="cuda"))[0, -1].float()
            assert logits[tok] >= logits.max() - tol * logits.abs().max(), (len(seq), tok, int(logits.argmax()))
            seq.append(tok)


@pytest.fixture
def no_gather(monkeypatch):
    """The parent route's two ops raise: nothing on the paged route may call them."""
    import kgs.ops.decode
    import kgs.ops.transformer

    def boom(*a, **k):
        raise AssertionError("the paged prefill route called the gather path")

    monkeypatch.setattr(kgs.ops.decode, "gather_kv", boom)
    monkeypatch.setattr(kgs.ops.transformer, "attention_chunk", boom)


@pytest.mark.parametrize("graphs", [False, True])
def test_chunked_prefill_engine_on_paged_route_matches_oracle(graphs, no_gather):
    from kgs.serve import SamplingParams

    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, 1024, size=n).tolist() for n in (40, 700, 300, 129, 5)]
    p = SamplingParams(max_tokens=6, ignore_eos=True)
    eng = _engine(graphs, chunked_prefill=256, paged_prefill=True)
    assert eng.model.paged_prefill
    outs = eng.generate(prompts, p)
    assert eng.stats["mixed_steps"] >= 4 and all(len(r.output) == 6 for r in outs)
    _oracle_check(eng, prompts, outs)
    assert eng.sched.check_invariants() == ""


def test_prefix_caching_engine_on_paged_route_matches_oracle(no_gather):
    from kgs.serve import SamplingParams

    rng = np.random.default_rng(11)
    system = rng.integers(3, 1024, size=300).tolist()
    prompts = [system + rng.integers(3, 1024, size=n).tolist() for n in (5, 40, 77, 130)]
    eng = _engine(True, prefix_caching=True, chunked_prefill=512, paged_prefill=True)
    p = SamplingParams(max_tokens=5, ignore_eos=True)
    outs = eng.generate(prompts[:1], p) + eng.generate(prompts[1:], p)
    assert eng.sched.prefix_hit_tokens >= 3 * 256
    _oracle_check(eng, prompts, outs)
    assert eng.sched.check_invariants() == ""
