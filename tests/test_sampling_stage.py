"""kgs.serve.sampling on CPU: the packed staging buffers' layout and double
buffering, and the sampler's torch route on a bare Sampler (no model, no
scheduler: none of this needs the native scheduler module)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _sampler(params, max_batch=4, vocab=64, prompts=None, **cfg):
    """A Sampler over one request per SamplingParams (ids 0, 1, ...), all tracked."""
    from kgs.serve.engine import EngineConfig
    from kgs.serve.sampling import Request, Sampler

    requests = {}
    s = Sampler(EngineConfig(max_batch=max_batch, **cfg), "cpu", "ref", vocab, requests)
    for rid, p in enumerate(params):
        requests[rid] = Request(rid, list((prompts or {}).get(rid, [5, 6])), p)
        s.track(requests[rid])
    return s, requests


def test_sampling_penalties():
    from kgs.serve import SamplingParams

    s, reqs = _sampler([SamplingParams(max_tokens=1, presence_penalty=1.0, frequency_penalty=0.5,
                                       repetition_penalty=2.0)], vocab=16)
    reqs[0].output = [7, 7, 9]
    logits = torch.zeros(1, 16)
    logits[0, 5], logits[0, 7], logits[0, 9], logits[0, 3] = 4.0, 4.0, -2.0, 1.0
    rows, sub = s._penalized_rows([reqs[0]], logits)
    out = sub[0]
    # 7: (4 - 0.5*2 - 1) / 2 = 1; 9: (-2 - 0.5 - 1) * 2 = -7; 5 (prompt): 4 / 2 = 2; 3 untouched
    assert rows == [0]
    assert out[7].item() == 1.0 and out[9].item() == -7.0 and out[5].item() == 2.0 and out[3].item() == 1.0


def test_top_p_sampling_keeps_nucleus():
    from kgs.serve import SamplingParams

    s, _ = _sampler([SamplingParams(temperature=1.0, top_p=0.3),
                     SamplingParams(max_tokens=1, temperature=1.0, top_p=1.0)], prompts={0: [5, 6, 7]})
    # one dominant token (p ~ 0.9) -> top_p 0.3 always picks it; top_p 1.0 can pick others
    logits = torch.full((2, 64), -5.0)
    logits[:, 7] = 5.0
    picks = {int(s.sample([0, 1], logits).tokens[0]) for _ in range(50)}
    assert picks == {7}


def test_packed_staging_layouts_and_double_buffering():
    """rows = 3 (odd on purpose: a misplaced int64 field would sit at an odd
    multiple of 4). The offsets are the layouts the kernels' pointers rely on."""
    from kgs.ops.transformer import LOGPROB_KMAX
    from kgs.serve.sampling import LOGIT_OP_FIELDS, LOGPROB_FIELDS, PARAM_FIELDS, TOKEN_FIELDS, PackedStaging

    assert LOGPROB_KMAX == 32
    mb = 3
    p = PackedStaging(PARAM_FIELDS + LOGIT_OP_FIELDS, mb, "cpu")
    # seed i64 | counter i64 | temperature f32 | top_k i32 | top_p f32, then with the device logit ops
    # freq f32 | pres f32 | rep f32 | slot i32 | want i32
    assert p.offsets == {"seed": 0, "counter": 8 * mb, "temperature": 16 * mb, "top_k": 20 * mb, "top_p": 24 * mb,
                         "freq": 28 * mb, "pres": 32 * mb, "rep": 36 * mb, "slot": 40 * mb, "want": 44 * mb}
    assert list(p.offsets) == list(PackedStaging(PARAM_FIELDS, mb, "cpu").offsets) + [f[0] for f in LOGIT_OP_FIELDS]
    assert PackedStaging(PARAM_FIELDS, mb, "cpu").dev["top_p"].untyped_storage().nbytes() == 28 * mb
    lp = PackedStaging(LOGPROB_FIELDS, mb, "cpu")
    assert lp.offsets == {"lp": 0, "top_val": 4 * mb, "top_idx": 4 * mb * (1 + 32)}
    assert lp.dev["lp"].shape == (mb,) and lp.dev["top_val"].shape == (mb, 32) and lp.dev["top_idx"].shape == (mb, 32)
    assert lp.dev["top_idx"].untyped_storage().nbytes() == 4 * mb * (1 + 2 * 32)
    assert PackedStaging(TOKEN_FIELDS, mb, "cpu").offsets == {"tokens": 0}
    dt = {k: (v.dtype, p.host[k].dtype) for k, v in p.dev.items()}
    assert dt["seed"] == dt["counter"] == (torch.int64, np.int64)
    assert dt["top_k"] == dt["slot"] == dt["want"] == (torch.int32, np.int32)
    assert dt["temperature"] == dt["top_p"] == dt["freq"] == dt["pres"] == dt["rep"] == (torch.float32, np.float32)
    # every view sits at its offset of the one buffer
    base = p.dev["seed"].data_ptr()
    assert all(v.data_ptr() - base == p.offsets[k] for k, v in p.dev.items())

    # a write through the host view arrives in the device view after push()
    first = p.host
    first["seed"][:] = [-1, 2**62, 7]
    first["top_p"][:] = [0.25, 0.5, 1.0]
    first["want"][:] = [-1, 5, 32]
    p.push()
    assert p.dev["seed"].tolist() == [-1, 2**62, 7] and p.dev["top_p"].tolist() == [0.25, 0.5, 1.0]
    assert p.dev["want"].tolist() == [-1, 5, 32] and p.dev["counter"].tolist() == [0, 0, 0]
    # two successive push() calls use different host sides, the third the first again
    second = p.host
    assert second["seed"] is not first["seed"] and not np.shares_memory(second["seed"], first["seed"])
    assert second["seed"].tolist() == [0, 0, 0]
    second["seed"][:] = [1, 2, 3]
    p.push()
    assert p.dev["seed"].tolist() == [1, 2, 3] and p.host["seed"] is first["seed"]

    # pull(): the device buffer into one side, then the other
    lp.dev["top_idx"][2, 31] = 9
    a = lp.pull()
    lp.dev["top_idx"][2, 31] = 11
    b = lp.pull()
    assert a["top_idx"][2, 31] == 9 and b["top_idx"][2, 31] == 11 and not np.shares_memory(a["lp"], b["lp"])
    assert lp.pull()["top_idx"] is a["top_idx"]
    # ... or a field from a tensor of the caller's (the step's tokens), its leading rows
    t = PackedStaging(TOKEN_FIELDS, mb, "cpu")
    h = t.pull(tokens=torch.tensor([4, 5]))
    assert h["tokens"][:2].tolist() == [4, 5] and h["tokens"].dtype == np.int64

    # a misaligned field order raises
    with pytest.raises(AssertionError, match="misaligned"):
        PackedStaging((("temperature", np.float32), ("seed", np.int64)), mb, "cpu")


def test_device_flags_are_ignored_on_cpu_and_the_routes_agree():
    """A Sampler asked for the device sampler and the device logit ops on the
    ref backend reports both off and samples exactly as one that was not asked:
    a penalised, a seeded-temperature and a greedy-with-logprobs row, 4 steps."""
    from kgs.serve import SamplingParams
    from kgs.serve.engine import EngineConfig
    from kgs.serve.sampling import Sampler

    with pytest.raises(ValueError, match="device_logit_ops.*device_sampler"):
        Sampler(EngineConfig(device_logit_ops=True), "cpu", "ref", 64, {})
    ps = [SamplingParams(frequency_penalty=0.5, presence_penalty=0.3, repetition_penalty=1.3),
          SamplingParams(temperature=0.9, top_k=20, seed=11), SamplingParams(logprobs=3)]
    steps = [torch.randn(3, 64, generator=torch.Generator().manual_seed(i)) * 3 for i in range(4)]

    def run(flag):
        s, reqs = _sampler(ps, device_sampler=flag, device_logit_ops=flag, seed=5)
        assert s.device_sampler is False and s.device_logit_ops is False
        assert s.params is None and s.lp is None and all(r.draw is None for r in reqs.values())
        out = []
        for logits in steps:
            res = s.sample(np.arange(3), logits)
            toks, lps = res.result()
            assert res.event is None and toks.dtype == np.int32 and toks.tolist() == res.tokens.tolist()
            assert set(lps) == {2} and len(lps[2][1]) == 3 and lps[2][1][0][0] == toks[2]  # greedy: the top token
            for r, t in zip(reqs.values(), toks):
                r.output.append(int(t))
            out.append((toks.tolist(), lps))
        assert s.counts is None
        for rid in range(3):
            assert not s.can_overlap()
            s.forget(rid)
        assert s.can_overlap()
        for p in ps:  # each of the three alone keeps the batch on one step at a time
            one, _ = _sampler([p], device_sampler=flag, device_logit_ops=flag)
            assert not one.can_overlap()
            one.forget(0)
            assert one.can_overlap()
        return out

    on, off = run(True), run(False)
    assert on == off
    assert len({tuple(t) for t, _ in on}) > 1  # the steps did not all sample the same tokens
