"""The CPU side of EngineConfig.device_logit_ops: the numpy references that state
penalize_rows' and logprob_rows' semantics, the count-table slot bookkeeping on
CPU tensors, the ops' host-side validation, and the engine / bench / server
surface of the flag."""
import argparse

import numpy as np
import pytest

torch = pytest.importorskip("torch")

PROMPT = 1 << 30


def _pen(x, w, freq=0.0, pres=0.0, rep=1.0, slot=0):
    """penalize_rows_reference on one row: float values in, float values and bits out."""
    from kgs.ops.transformer import bf16_bits_to_float, penalize_rows_reference

    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    w = np.atleast_2d(np.asarray(w, dtype=np.int64)).astype(np.int32)
    bits = penalize_rows_reference(x, [freq], [pres], [rep], [slot], w)
    return bf16_bits_to_float(bits)[0], bits[0]


def test_penalize_reference_hand_checked_values():
    from kgs.ops.transformer import bf16_bits, penalize_rows_reference

    # 2.0 - (0.5 * 3 + 0.25) = 0.25, then / 2
    assert _pen([2.0], [3], freq=0.5, pres=0.25, rep=2.0)[0].tolist() == [0.125]
    # a prompt token that was never generated: only the repetition penalty, negative logits are multiplied
    assert _pen([-1.0], [PROMPT], freq=0.5, pres=0.25, rep=2.0)[0].tolist() == [-2.0]
    # prompt bit + a count: both; the count does not include the bit
    assert _pen([2.0], [PROMPT | 3], freq=0.5, pres=0.25, rep=2.0)[0].tolist() == [0.125]
    # counts above 2^16: 1.0 - 0.001 * 70000 (fp32: 0.001f * 70000f = 70.0 after one rounding) = -69 -> bf16
    v = np.float32(1.0) - (np.float32(0.001) * np.float32(70000) + np.float32(0))
    assert _pen([1.0], [70000], freq=0.001)[1].tolist() == bf16_bits(np.array([v])).tolist()
    assert abs(float(_pen([1.0], [70000], freq=0.001)[0][0]) + 69.0) <= 0.25
    # w == 0: the bits pass through, whatever they are (a NaN with a payload, -0, -inf)
    odd = np.array([[0x7fa5, 0x8000, 0xff80, 0xffff, 0x0001]], dtype=np.uint16)
    out = penalize_rows_reference(odd, [9.0], [9.0], [3.0], [0], np.zeros((1, 5), np.int32))
    assert out.tolist() == odd.tolist()
    # a row without a slot is copied, counts or not
    out = penalize_rows_reference(odd, [9.0], [9.0], [3.0], [-1], np.full((1, 5), 7, np.int32))
    assert out.tolist() == odd.tolist()
    # rep == 1 and no count: the value is kept even for a prompt token
    assert _pen([0.3359375], [PROMPT], freq=1.0, pres=1.0, rep=1.0)[0].tolist() == [0.3359375]
    # one rounding to bf16, nearest-even: 1 + 2^-8 is a tie between 1.0 and 1 + 2^-7 -> the even one, 1.0
    assert _pen([2.0], [1], pres=1.0 - 2.0 ** -8)[1].tolist() == [0x3f80]
    assert _pen([2.0], [1], pres=1.0 - 3 * 2.0 ** -8)[1].tolist() == [0x3f82]  # 1 + 3 * 2^-8: tie -> 1 + 2^-6


def test_logprob_reference_by_hand():
    from kgs.ops.transformer import LOGPROB_KMAX, logprob_rows_reference

    assert LOGPROB_KMAX == 32
    x = np.log(np.array([[0.1, 0.4, 0.2, 0.3]]))
    lp, tv, ti = logprob_rows_reference(x, [2], [3])
    assert np.isclose(lp[0], np.log(0.2))
    assert ti[0, :4].tolist() == [1, 3, 2, -1] and np.allclose(tv[0, :3], np.log([0.4, 0.3, 0.2]))
    assert np.isnan(tv[0, 3:]).all() and (ti[0, 3:] == -1).all()
    # ties: lowest index first, and -0 equals +0; exactly k entries
    lp, tv, ti = logprob_rows_reference([[0.0, 1.0, -0.0, 1.0, 0.0, -5.0, 1.0, -5.0]], [0], [4])
    assert ti[0, :5].tolist() == [1, 3, 6, 0, -1]
    lp, tv, ti = logprob_rows_reference([[0.0, 1.0, -0.0, 1.0, 0.0, -5.0, 1.0, -5.0]], [0], [6])
    assert ti[0, :6].tolist() == [1, 3, 6, 0, 2, 4]
    # k > cols clamps to cols, k > 32 clamps to 32
    lp, tv, ti = logprob_rows_reference(x, [0], [9])
    assert ti[0, :5].tolist() == [1, 3, 2, 0, -1]
    big = np.arange(40, dtype=np.float64)[None, ::-1]
    assert (logprob_rows_reference(big, [0], [40])[2][0] == np.arange(32)).all()
    # -inf: logprob -inf, ranked last; a sampled -inf token too
    lp, tv, ti = logprob_rows_reference([[0.0, -np.inf, 0.0, -np.inf]], [1], [3])
    assert lp[0] == -np.inf and ti[0, :3].tolist() == [0, 2, 1]
    assert np.allclose(tv[0, :2], np.log(0.5)) and tv[0, 2] == -np.inf
    # a NaN row, a row of -inf, a row with +inf: NaN everywhere, indices 0 .. k-1
    for row in ([0.0, np.nan, 1.0, 2.0], [-np.inf] * 4, [0.0, np.inf, 1.0, 2.0]):
        lp, tv, ti = logprob_rows_reference([row], [2], [2])
        assert np.isnan(lp[0]) and np.isnan(tv[0]).all() and ti[0, :3].tolist() == [0, 1, -1]
    # a token outside the row: NaN; a skipped row: nothing; k = 0: the logprob alone
    lp, tv, ti = logprob_rows_reference(np.concatenate([x, x, x]), [4, 1, 1], [1, -1, 0])
    assert np.isnan(lp[0]) and ti[0, 0] == 1
    assert np.isnan(lp[1]) and (ti[1] == -1).all()
    assert np.isclose(lp[2], np.log(0.4)) and (ti[2] == -1).all()


def _direct(prompt, output, vocab):
    row = np.zeros(vocab, np.int64)
    row[sorted(set(prompt))] = PROMPT
    np.add.at(row, output, 1)
    return row


def test_count_table_slots_on_cpu_tensors():
    from kgs.ops.transformer import COUNT_MASK, COUNT_PROMPT
    from kgs.serve.count_table import CountTable

    assert COUNT_PROMPT == PROMPT and COUNT_MASK == PROMPT - 1
    vocab = 64
    ct = CountTable(vocab, "cpu", slots=2)
    assert ct.slots == 2 and ct.used == 0 and ct.slot(7) == -1
    rng = np.random.default_rng(0)
    reqs = {rid: (rng.integers(0, vocab, 20).tolist(), rng.integers(0, vocab, 30).tolist()) for rid in range(5)}
    s0 = ct.acquire(0, *reqs[0])
    assert s0 == 0 and ct.acquire(0, [1], [2]) == 0  # a second acquire: the same slot, the row is not rebuilt
    assert ct.table[0].numpy().tolist() == _direct(*reqs[0], vocab).tolist()
    assert ct.acquire(1, *reqs[1]) == 1
    # the table grows by doubling and keeps its rows
    assert ct.acquire(2, *reqs[2]) == 2 and ct.slots == 4
    assert ct.acquire(3, *reqs[3]) == 3 and ct.acquire(4, *reqs[4]) == 4 and ct.slots == 8
    for rid in range(5):
        assert ct.table[ct.slot(rid)].numpy().tolist() == _direct(*reqs[rid], vocab).tolist()
    assert (ct.table[5:] == 0).all()
    # the row agrees with the reference's reading of it: a penalised copy from a direct count
    from kgs.ops.transformer import penalize_rows_reference

    x = rng.normal(size=(1, vocab)).astype(np.float32)
    a = penalize_rows_reference(x, [0.5], [0.25], [1.5], [ct.slot(3)], ct.table)
    b = penalize_rows_reference(x, [0.5], [0.25], [1.5], [0], _direct(*reqs[3], vocab)[None])
    assert a.tolist() == b.tolist() and a.tolist() != penalize_rows_reference(x, [0.], [0.], [1.], [-1],
                                                                              ct.table).tolist()
    # release (finish or abort): the slot is reused, its row rebuilt for the new owner
    ct.release(1)
    ct.release(1)  # releasing twice, or a request without a slot: nothing
    ct.release(99)
    assert ct.used == 4 and ct.slot(1) == -1
    assert ct.acquire(9, [3, 3, 5], []) == 1
    assert ct.table[1].numpy().tolist() == _direct([3, 5], [], vocab).tolist()
    # tokens outside the vocabulary are ignored rather than indexed
    ct.release(9)
    assert ct.acquire(10, [-1, vocab, 2], [vocab + 5, 2, 2]) == 1
    assert ct.table[1].numpy().tolist() == _direct([2], [2, 2], vocab).tolist()
    for rid in (0, 2, 3, 4, 10):
        ct.release(rid)
    assert ct.used == 0


def _tiny():
    from kgs.models.llama import LlamaConfig

    return LlamaConfig(hidden=256, intermediate=512, heads=2, kv_heads=1, layers=2, vocab=512)


def test_engine_flag_defaults_off_needs_the_device_sampler_and_is_ignored_by_the_ref_backend():
    pytest.importorskip("kgs._native._serve")
    from kgs.serve import EngineConfig, LLMEngine, SamplingParams

    assert EngineConfig().device_logit_ops is False
    base = dict(num_pages=64, max_batch=4, max_model_len=256, cuda_graphs=False)
    with pytest.raises(ValueError, match="device_logit_ops.*device_sampler"):
        LLMEngine(_tiny(), EngineConfig(device_logit_ops=True, **base), device="cpu", backend="ref")
    prompts = [[5, 6, 7], [9, 10], [11, 12, 13, 14]]
    ps = [SamplingParams(max_tokens=6, frequency_penalty=0.5, presence_penalty=0.3, ignore_eos=True),
          SamplingParams(max_tokens=6, logprobs=3, ignore_eos=True),
          SamplingParams(max_tokens=6, repetition_penalty=1.3, logprobs=2, ignore_eos=True)]

    def run(flag):
        eng = LLMEngine(_tiny(), EngineConfig(device_sampler=flag, device_logit_ops=flag, **base), device="cpu",
                        backend="ref")
        assert eng.device_logit_ops is False and eng.device_sampler is False
        for p in (ps[0], ps[1]):
            rid = eng.add_request(prompts[0], p)
            assert not eng._overlap_now()  # penalties / logprobs: still one step at a time
            eng.abort(rid)
        outs = eng.generate(prompts, ps)
        assert eng.sampler.counts is None  # no count table on this route
        return [(r.output, r.logprobs) for r in outs]

    on, off = run(True), run(False)
    assert on == off
    assert [len(lp) for _, lp in on] == [0, 6, 6] and len(on[1][1][0][1]) == 3


def test_bench_parser_and_online_run_without_the_new_arguments(monkeypatch):
    pytest.importorskip("kgs._native._serve")
    from kgs.serve import bench

    seen = {}
    monkeypatch.setattr(bench, "run_engine", lambda a: seen.update(vars(a)) or {})
    assert bench.main(["--device-sampler", "--device-logit-ops", "--logprobs", "5", "--presence-penalty", "0.2",
                       "--frequency-penalty", "0.5", "--repetition-penalty", "1.1"]) == 0
    keys = ("device_logit_ops", "logprobs", "presence_penalty", "frequency_penalty", "repetition_penalty")
    assert tuple(seen[k] for k in keys) == (True, 5, 0.2, 0.5, 1.1)
    seen.clear()
    assert bench.main([]) == 0
    assert tuple(seen[k] for k in keys) == (False, None, 0.0, 0.0, 1.0)
    ps = bench._sampling(argparse.Namespace(output_len=3, logprobs=2, frequency_penalty=0.5, repetition_penalty=1.2), 2)
    assert (ps[1].logprobs, ps[1].frequency_penalty, ps[1].presence_penalty, ps[1].repetition_penalty) == \
        (2, 0.5, 0.0, 1.2)
    # a hand-built Namespace from before these flags still runs, and the record echoes the defaults
    a = argparse.Namespace(requests=3, input_len=12, output_len=3, max_batch=4, max_model_len=256,
                           max_prefill_tokens=4096, layers=2, no_graphs=True, fused_max_batch=0,
                           decode_weights="bf16", kv_cache_dtype="bf16", request_rate=500.0)
    r = bench.run_online(a, mc=_tiny(), device="cpu", backend="ref")
    assert tuple(r[k] for k in keys) == (False, None, 0.0, 0.0, 1.0)
    a.device_sampler, a.device_logit_ops, a.logprobs, a.frequency_penalty = True, True, 2, 0.5
    r = bench.run_online(a, mc=_tiny(), device="cpu", backend="ref")
    assert tuple(r[k] for k in keys) == (False, 2, 0.0, 0.5, 1.0) and r["stats"]["decode_tokens"] > 0


def test_serve_parser_has_the_flag():
    import inspect

    from kgs.serve import api

    src = inspect.getsource(api.main)
    assert '"--device-logit-ops"' in src and "device_logit_ops=a.device_logit_ops" in src


def _raises_each(call, good, typed, vectors):
    for name, bad in typed:
        with pytest.raises(TypeError, match=name):
            call(**{name: bad})
    for name in vectors:
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:2]})
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name].repeat(2)[::2]})  # right length, not contiguous
        with pytest.raises(ValueError, match=name):
            call(**{name: good[name][:, None].repeat(1, 2)})
    with pytest.raises(ValueError, match="GPU"):  # everything well-formed, but on the host
        call()


def test_penalize_rows_validation():
    from kgs.ops.transformer import penalize_rows

    rows = 3
    good = dict(logits=torch.zeros(rows, 16, dtype=torch.bfloat16), freq=torch.zeros(rows), pres=torch.zeros(rows),
                rep=torch.ones(rows), slot=torch.zeros(rows, dtype=torch.int32),
                counts=torch.zeros(2, 16, dtype=torch.int32))
    call = lambda **kw: penalize_rows(**{**good, **kw})  # noqa: E731
    with pytest.raises(TypeError, match="logits"):
        call(logits=torch.zeros(rows, 16))
    _raises_each(call, good,
                 [("freq", torch.zeros(rows, dtype=torch.float64)), ("pres", torch.zeros(rows).bfloat16()),
                  ("rep", [1.0] * rows), ("slot", torch.zeros(rows, dtype=torch.int64)),
                  ("counts", torch.zeros(2, 16, dtype=torch.int64)), ("out", torch.zeros(rows, 16))],
                 ["freq", "pres", "rep", "slot"])
    with pytest.raises(ValueError, match="logits"):
        call(logits=torch.zeros(16, rows, dtype=torch.bfloat16).t())
    with pytest.raises(ValueError, match="counts"):
        call(counts=torch.zeros(2, 24, dtype=torch.int32))
    with pytest.raises(ValueError, match="counts"):
        call(counts=torch.zeros(2, 32, dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match="out"):
        call(out=torch.zeros(rows, 32, dtype=torch.bfloat16)[:, :16])  # the output is contiguous


def test_token_counts_add_validation():
    from kgs.ops.transformer import token_counts_add

    rows = 3
    good = dict(counts=torch.zeros(2, 16, dtype=torch.int32), tok=torch.zeros(rows, dtype=torch.int64),
                slot=torch.zeros(rows, dtype=torch.int32))
    call = lambda **kw: token_counts_add(**{**good, **kw})  # noqa: E731
    for name, bad in (("counts", torch.zeros(2, 16)), ("tok", torch.zeros(rows, dtype=torch.int32)),
                      ("slot", torch.zeros(rows, dtype=torch.int64))):
        with pytest.raises(TypeError, match=name):
            call(**{name: bad})
    with pytest.raises(ValueError, match="counts"):
        call(counts=torch.zeros(16, dtype=torch.int32))
    with pytest.raises(ValueError, match="slot"):
        call(slot=good["slot"][:2])
    with pytest.raises(ValueError, match="tok"):
        call(tok=good["tok"][:, None])
    with pytest.raises(ValueError, match="GPU"):
        call()


def test_logprob_rows_validation():
    from kgs.ops.transformer import logprob_rows

    rows = 3
    good = dict(logits=torch.zeros(rows, 16, dtype=torch.bfloat16), tok=torch.zeros(rows, dtype=torch.int64),
                want=torch.zeros(rows, dtype=torch.int32))
    call = lambda **kw: logprob_rows(**{**good, **kw})  # noqa: E731
    with pytest.raises(TypeError, match="logits"):
        call(logits=torch.zeros(rows, 16))
    _raises_each(call, good,
                 [("tok", torch.zeros(rows, dtype=torch.int32)), ("want", torch.zeros(rows, dtype=torch.int64)),
                  ("lp", torch.zeros(rows, dtype=torch.float64)), ("top_val", torch.zeros(rows, 32).bfloat16()),
                  ("top_idx", torch.zeros(rows, 32, dtype=torch.int64))],
                 ["tok", "want"])
    with pytest.raises(ValueError, match="lp"):
        call(lp=torch.zeros(rows + 1))
    with pytest.raises(ValueError, match="top_val"):
        call(top_val=torch.zeros(rows, 16))
    with pytest.raises(ValueError, match="top_idx"):
        call(top_idx=torch.zeros(rows, 64, dtype=torch.int32)[:, ::2])
