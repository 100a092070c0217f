"""The device sampler's CPU side: Philox4x32-10, the float64 reference that
states sample_rows' semantics (kept sets, distribution), the op's host-side
validation, and the engine / bench surface of EngineConfig.device_sampler."""
import argparse

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _ref(x, T=1.0, k=0, p=1.0, seed=0, counter=0):
    from kgs.ops.transformer import sample_rows_reference

    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = len(x)
    full = lambda v: np.broadcast_to(np.asarray(v), (n,))  # noqa: E731
    return sample_rows_reference(x, full(T), full(k), full(p), full(seed), full(counter))


def test_philox_known_answers():
    """Random123's known answers for Philox4x32-10: counter and key all zero,
    all ones, and the digits of pi."""
    from kgs.ops.transformer import philox4x32_10

    def run(ctr, key):
        return [f"{v:08x}" for v in philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))]

    assert run([0] * 4, [0] * 2) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert run([0xffffffff] * 4, [0xffffffff] * 2) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert run([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_uniforms_follow_the_documented_stream():
    """Element i is word i % 4 of the block with counter (i // 4, counter lo,
    counter hi, 0) and key (seed lo, seed hi); nothing else enters."""
    from kgs.ops.transformer import philox4x32_10, sample_uniforms

    seed, counter = -0x123456789abcdef, (5 << 32) | 7  # a negative seed: its two's-complement words
    u = sample_uniforms([seed, 3], [counter, 0], 10)
    assert u.shape == (2, 10) and (u > 0).all() and (u < 1).all()
    s = seed & (2**64 - 1)
    w = philox4x32_10(np.array([2, 7, 5, 0], np.uint32), np.array([s & 0xffffffff, s >> 32], np.uint32))
    assert u[0, 9] == ((int(w[1]) >> 8) + 0.5) * 2.0 ** -24
    assert not np.array_equal(u[0], u[1])
    assert np.array_equal(sample_uniforms([3], [0], 10)[0], u[1])  # a row's stream does not depend on its batch


def test_reference_top_k_keeps_ties_at_the_kth_value():
    x = [3.0, 1.0, 2.0, 2.0, 0.5, 2.0, -1.0, 0.0]
    assert _ref(x, k=2).kept[0].tolist() == [True, False, True, True, False, True, False, False]
    assert _ref(x, k=1).kept[0].tolist() == [True] + [False] * 7
    assert _ref(x, k=5).kept[0].sum() == 5
    # the filter is on only for 0 < k < cols
    for k in (0, -3, 8, 9, 1000):
        assert _ref(x, k=k).kept[0].all()
    assert _ref(x, k=7).kept[0].sum() == 7


def test_reference_top_p_keeps_ties_together():
    # probabilities 0.4, 0.2, 0.2, 0.1, 0.1 at T = 1
    x = np.log([0.4, 0.2, 0.2, 0.1, 0.1, 1e-300, 1e-300, 1e-300])
    kept = lambda p: _ref(x, p=p).kept[0, :5].tolist()  # noqa: E731
    assert kept(0.3) == [True, False, False, False, False]      # M(0.4) = 0 < p, M(0.2) = 0.4 >= p
    assert kept(0.5) == [True, True, True, False, False]        # the boundary falls between the tied 0.2s: both kept
    assert kept(0.7) == [True, True, True, False, False]        # M(0.1) = 0.8 >= p
    assert kept(0.85) == [True, True, True, True, True]         # both tied 0.1s
    assert kept(1e-9) == [True, False, False, False, False]
    # the token that crosses p is included, the one after it is not
    r = _ref(x, p=0.3)
    assert 0.09 < r.p_margin[0] < 0.11 + 1e-12  # |M(0.2) - 0.3| = 0.1, the closest boundary
    # p outside (0, 1): off
    for p in (1.0, 0.0, -0.5, 2.0):
        r = _ref(x, p=p)
        assert r.kept[0, :5].all() and np.isinf(r.p_margin[0])


def test_reference_top_p_runs_over_the_top_k_survivors_at_temperature():
    x = np.log([0.4, 0.2, 0.2, 0.1, 0.1, 1e-9, 1e-9, 1e-9])
    # survivors of k = 3 renormalise to 0.5, 0.25, 0.25: M(0.25) = 0.5
    assert _ref(x, k=3, p=0.45).kept[0].sum() == 1
    assert _ref(x, k=3, p=0.55).kept[0].sum() == 3
    # T = 0.5 squares the probabilities: 16, 4, 4, 1, 1 of 26 -> M(0.2) = 0.615
    assert _ref(x, T=0.5, p=0.6).kept[0].sum() == 1
    assert _ref(x, T=0.5, p=0.63).kept[0].sum() == 3


def test_reference_special_values():
    ninf = -np.inf
    r = _ref([[ninf, 1.0, ninf, 0.0, ninf, ninf, ninf, ninf]] * 200, counter=np.arange(200))
    assert r.kept[0].tolist() == [False, True, False, True] + [False] * 4
    assert set(r.tokens.tolist()) == {1, 3}  # -inf is never chosen
    assert _ref([ninf, 1.0, ninf, 0.0, ninf, ninf, ninf, ninf], k=3).kept[0].sum() == 2  # the 3rd largest is -inf
    # greedy, NaN and no finite maximum: the first index of the maximum, NaN counting as the maximum
    assert _ref([0.0, 2.0, 2.0, 1.0], T=0.0).tokens[0] == 1
    assert _ref([0.0, 2.0, 2.0, 1.0], T=-1.0).tokens[0] == 1
    assert _ref([0.0, np.nan, 5.0, np.nan], T=1.0).tokens[0] == 1
    assert _ref([ninf] * 4, T=1.0).tokens[0] == 0
    assert _ref([0.0, np.inf, 1.0, np.inf], T=1.0).tokens[0] == 1
    r = _ref([0.0, 2.0, 2.0, 1.0], T=0.0)
    assert r.kept[0].tolist() == [False, True, False, False] and np.isinf(r.gap[0])


def test_reference_token_is_the_gumbel_argmax():
    from kgs.ops.transformer import sample_uniforms

    rng = np.random.default_rng(0)
    x = rng.normal(size=(3, 16)) * 2
    r = _ref(x, T=0.7, k=5, seed=[1, 2, 3], counter=[4, 5, 6])
    u = sample_uniforms([1, 2, 3], [4, 5, 6], 16)
    score = np.where(r.kept, x / 0.7 - np.log(-np.log(u)), -np.inf)
    assert r.tokens.tolist() == score.argmax(1).tolist()
    top = np.sort(score, axis=1)
    assert np.allclose(r.gap, top[:, -1] - top[:, -2])
    assert r.kept[np.arange(3), r.tokens].all()


@pytest.mark.parametrize("k, p", [(0, 1.0), (8, 1.0), (0, 0.7)])
def test_reference_distribution(k, p):
    """65 536 draws (counters 0 .. 65 535) over 64 logits: every token's frequency
    within 5 sqrt(q (1 - q) / N) + 1 / N of its softmax probability q over the
    kept set."""
    n, T = 65536, 0.8
    x = torch.randn(64, generator=torch.Generator().manual_seed(3)).mul(2).bfloat16().double().numpy()
    r = _ref(np.broadcast_to(x, (n, 64)), T=T, k=k, p=p, seed=11, counter=np.arange(n))
    kept = r.kept[0]
    assert (r.kept == kept).all() and kept.sum() == ({8: 8}.get(k, 64) if p == 1.0 else kept.sum())
    assert 1 < kept.sum() < 64 or (k == 0 and p == 1.0)
    q = np.where(kept, np.exp((x - x.max()) / T), 0.0)
    q /= q.sum()
    f = np.bincount(r.tokens, minlength=64) / n
    assert (np.abs(f - q) <= 5 * np.sqrt(q * (1 - q) / n) + 1 / n).all()
    assert 2e-4 < (r.gap < 1e-3).mean() < 3e-3  # a near-tie of width g happens about g of the time


def _tiny():
    from kgs.models.llama import LlamaConfig

    return LlamaConfig(hidden=256, intermediate=512, heads=2, kv_heads=1, layers=2, vocab=512)


def test_engine_flag_is_ignored_by_the_ref_backend():
    """EngineConfig.device_sampler exists, defaults to off, and a backend without
    the kernel ignores it (as paged_prefill is ignored): same tokens, seeded
    requests still on their generators and still one step at a time."""
    pytest.importorskip("kgs._native._serve")
    from kgs.serve import EngineConfig, LLMEngine, SamplingParams

    assert EngineConfig().device_sampler is False
    prompts = [[5, 6, 7], [9, 10]]
    ps = [SamplingParams(max_tokens=5, temperature=1.0, top_p=0.9, seed=7, ignore_eos=True),
          SamplingParams(max_tokens=5, ignore_eos=True)]

    def run(flag):
        eng = LLMEngine(_tiny(), EngineConfig(num_pages=64, max_batch=4, max_model_len=256, cuda_graphs=False,
                                              device_sampler=flag), device="cpu", backend="ref")
        assert eng.device_sampler is False
        rid = eng.add_request(prompts[0], ps[0])
        assert not eng._overlap_now() and eng.requests[rid].draw is None
        eng.abort(rid)
        return [r.output for r in eng.generate(prompts, ps)]

    assert run(True) == run(False)


def test_engine_seed_mix_and_counter():
    from kgs.serve.engine import Request, SamplingParams, _i64, _mix64

    seeds = {_mix64(s, r) for s in range(4) for r in range(64)}
    assert len(seeds) == 256 and all(0 <= v < 2**64 for v in seeds)  # distinct per (engine seed, request)
    assert _mix64(0, 5) == _mix64(0, 5)
    assert _i64(2**64 - 1) == -1 and _i64(2**63) == -2**63 and _i64(5) == 5 and _i64(2**64 + 5) == 5
    assert Request(0, [1], SamplingParams()).sampled == 0


def test_bench_parser_and_online_run_without_the_new_arguments(monkeypatch):
    pytest.importorskip("kgs._native._serve")
    from kgs.serve import bench

    seen = {}
    monkeypatch.setattr(bench, "run_engine", lambda a: seen.update(vars(a)) or {})
    assert bench.main(["--device-sampler", "--temperature", "0.8", "--top-k", "50", "--top-p", "0.9", "--seeded"]) == 0
    assert (seen["device_sampler"], seen["temperature"], seen["top_k"], seen["top_p"], seen["seeded"]) == \
        (True, 0.8, 50, 0.9, True)
    seen.clear()
    assert bench.main([]) == 0
    assert (seen["device_sampler"], seen["temperature"], seen["top_k"], seen["top_p"], seen["seeded"]) == \
        (False, 0.0, 0, 1.0, False)
    ps = bench._sampling(argparse.Namespace(output_len=3, temperature=0.5, top_k=4, top_p=0.9, seeded=True), 3)
    assert [p.seed for p in ps] == [0, 1, 2] and ps[1].temperature == 0.5 and ps[1].top_k == 4 and ps[1].top_p == 0.9
    # a hand-built Namespace from before these flags still runs, greedy, and the record echoes the defaults
    a = argparse.Namespace(requests=3, input_len=12, output_len=3, max_batch=4, max_model_len=256,
                           max_prefill_tokens=4096, layers=2, no_graphs=True, fused_max_batch=0,
                           decode_weights="bf16", kv_cache_dtype="bf16", request_rate=500.0)
    r = bench.run_online(a, mc=_tiny(), device="cpu", backend="ref")
    assert (r["device_sampler"], r["temperature"], r["top_k"], r["top_p"], r["seeded"]) == (False, 0.0, 0, 1.0, False)
    a.temperature, a.top_p, a.device_sampler = 0.8, 0.9, True
    r = bench.run_online(a, mc=_tiny(), device="cpu", backend="ref")
    assert r["temperature"] == 0.8 and r["device_sampler"] is False and r["stats"]["decode_tokens"] > 0


def test_serve_parser_has_the_flag():
    import inspect

    from kgs.serve import api

    src = inspect.getsource(api.main)
    assert '"--device-sampler"' in src and "device_sampler=a.device_sampler" in src


def test_sample_rows_validation():
    from kgs.ops.transformer import sample_rows

    rows = 3
    good = dict(logits=torch.zeros(rows, 16, dtype=torch.bfloat16), temperature=torch.ones(rows),
                top_k=torch.zeros(rows, dtype=torch.int32), top_p=torch.ones(rows),
                seed=torch.zeros(rows, dtype=torch.int64), counter=torch.zeros(rows, dtype=torch.int64))

    def call(**kw):
        return sample_rows(**{**good, **kw})

    with pytest.raises(TypeError, match="logits"):
        call(logits=torch.zeros(rows, 16))
    for name, bad in (("temperature", torch.ones(rows, dtype=torch.float64)), ("top_k", torch.zeros(rows).long()),
                      ("top_p", torch.ones(rows).bfloat16()), ("seed", torch.zeros(rows, dtype=torch.int32)),
                      ("counter", torch.zeros(rows)), ("temperature", [1.0] * rows), ("out", torch.zeros(rows))):
        with pytest.raises(TypeError, match=name):
            call(**{name: bad})
    with pytest.raises(ValueError, match="logits"):
        call(logits=torch.zeros(16, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="logits"):
        call(logits=torch.zeros(16, rows, dtype=torch.bfloat16).t())
    for name in ("temperature", "top_k", "top_p", "seed", "counter"):
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:2]})
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name].repeat(2)[::2]})  # right length, not contiguous
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:, None].repeat(1, 2)})
    with pytest.raises(ValueError, match="out"):
        call(out=torch.zeros(rows + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="GPU"):  # everything well-formed, but on the host
        call()
