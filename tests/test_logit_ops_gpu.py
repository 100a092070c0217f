"""penalize_rows, token_counts_add and logprob_rows on the GPU
(native/kernels/logit_ops.hip) against their numpy references, and the engine
with EngineConfig.device_logit_ops.

penalize_rows is compared bit for bit (fp32 steps, each rounded once). The
logprob values carry a derived bound, not a measured one: the kernel sums
exp(x - m) in fp32, at most 2^10 sequential adds per thread (cols / 1024, 126
at the Llama-3 vocabulary) and a 10-level tree, each add within 2^-24 relative,
so the sum is within about 2^-14 = 6.1e-5 relative and its logarithm within
6.1e-5 absolute; expf, logf and the two subtractions at magnitude <= 64 add a
few ulps of 64 (2^-18 = 3.8e-6 each). Together below LP_TOL = 1e-4 wherever
|reference| <= 64. The torch fp32 log_softmax the kernel replaces is held to the
same bound on the same inputs."""
import dataclasses
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

VOCAB = 128256
COLS = (8, 520, 4104, VOCAB)
PROMPT = 1 << 30
LP_TOL = 1e-4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(x: torch.Tensor, pad: int = 8) -> torch.Tensor:
    """x as the first columns of a wider matrix whose other columns are NaN."""
    w = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    w[:, :x.shape[1]] = x.cuda()
    return w[:, :x.shape[1]]


# ---------------------------------------------------------------- penalize_rows
_FREQ = (0.5, -0.25, 0.0, 1.5)
_PRES = (0.25 + 2.0 ** -8, -1.0, 0.75, 0.0)
_REP = (2.0, 0.5, 1.0, 1.3)
_WORDS = np.array([0, 0, 0, 1, 2, 70000, PROMPT, PROMPT | 1, PROMPT | 5], np.int32)
# the first 8 columns of the first penalised row and of the unpenalised row after it:
# +inf, -inf, NaN, -0, a NaN with a payload, 2.0 (lands on a bf16 rounding tie), -0, 1.0
_SPECIAL_X = np.array([0x7f80, 0xff80, 0x7fc1, 0x8000, 0x7fa5, 0x4000, 0x8000, 0x3f80], np.uint16)
_SPECIAL_W = np.array([1, PROMPT, 1, PROMPT | 1, 0, 1, 0, 70000], np.int32)


@lru_cache(maxsize=None)
def _pen_case(cols: int, rows: int):
    from kgs.ops.transformer import bf16_bits, penalize_rows_reference

    rng = np.random.default_rng(cols + rows)
    x = bf16_bits(rng.normal(size=(rows, cols)).astype(np.float32) * 3)
    nslots = (rows + 1) // 2 + 1
    counts = _WORDS[rng.integers(0, len(_WORDS), size=(nslots, cols))]
    x[0, :8], counts[0, :8] = _SPECIAL_X, _SPECIAL_W
    if rows > 1:
        x[1, :8] = _SPECIAL_X
    j = np.arange(rows)
    slot = np.where(j % 2 == 0, j // 2, -1).astype(np.int32)  # penalised and unpenalised rows alternate
    if rows > 7:
        slot[7] = nslots + 3  # a slot past the table: copied too
    k = j // 2
    freq, pres, rep = (np.array(v, np.float32)[k % 4] for v in (_FREQ, _PRES, _REP))
    ref = penalize_rows_reference(x, freq, pres, rep, slot, counts)
    # the planted tie: 2.0 - (0.5 * 1 + 0.25 + 2^-8), then / 2, is halfway between two bf16 values
    v = (np.float32(2.0) - (np.float32(0.5) * np.float32(1) + pres[0])) / rep[0]
    assert int(np.float32(v).view(np.uint32)) & 0xffff == 0x8000 and ref[0, 5] == 0x3f20
    assert ref[0, 0] == 0x7f80 and ref[0, 1] == 0xff80 and ref[0, 2] == 0x7fc0 and ref[0, 4] == 0x7fa5
    assert ref[0, 6] == 0x8000 and (ref[1::2] == x[1::2]).all() and (ref[0] != x[0]).any()
    return x, (freq, pres, rep, slot), counts, ref


@pytest.mark.parametrize("rows", [1, 3, 9])
@pytest.mark.parametrize("cols", COLS)
def test_penalize_rows_is_bit_exact(cols, rows):
    from kgs.ops.transformer import bf16_bits, penalize_rows

    x, params, counts, ref = _pen_case(cols, rows)
    xd = _wide(_dev(x.view(np.int16)).view(torch.bfloat16))  # a row stride wider than cols, NaN beyond
    out = torch.empty((rows, cols), dtype=torch.bfloat16, device="cuda")
    got = penalize_rows(xd, *(_dev(p) for p in params), _dev(counts), out=out)
    assert got is out
    bad = np.argwhere(bf16_bits(got) != ref)
    assert len(bad) == 0, (bad[:8], bf16_bits(got)[tuple(bad[:8].T)], ref[tuple(bad[:8].T)])


def test_penalize_rows_zero_rows_and_kernel_errors():
    from kgs.ops import KernelError
    from kgs.ops.transformer import penalize_rows

    def args(rows, cols):
        return (torch.zeros(rows, cols, dtype=torch.bfloat16, device="cuda"), torch.zeros(rows, device="cuda"),
                torch.zeros(rows, device="cuda"), torch.ones(rows, device="cuda"),
                torch.zeros(rows, dtype=torch.int32, device="cuda"),
                torch.zeros(2, cols, dtype=torch.int32, device="cuda"))

    assert penalize_rows(*args(0, 16)).shape == (0, 16)
    with pytest.raises(KernelError):
        penalize_rows(*args(2, 12))  # cols % 8


def test_token_counts_add():
    from kgs.ops.transformer import token_counts_add

    slots, cols = 7, 520
    rng = np.random.default_rng(0)
    before = rng.integers(0, 5, size=(slots, cols)).astype(np.int32)
    before[2, 7] = PROMPT | 3  # the prompt bit rides along
    tok = np.array([7, 519, 0, 520, -1, 100, 7, 2**40 + 3], np.int64)
    slot = np.array([2, 0, -1, 1, 3, 5, 4, 6], np.int32)  # row 2: no slot; rows 3, 4, 7: tokens out of range
    slot2 = np.array([2, 0, -1, 1, 3, 9, 4, -5], np.int32)  # row 5: a slot past the table
    want = before.copy()
    for t, s in ((7, 2), (519, 0), (100, 5), (7, 4)):
        want[s, t] += 1
    table = _dev(before)
    assert token_counts_add(table, _dev(tok), _dev(slot)) is table
    assert np.array_equal(table.cpu().numpy(), want) and want[2, 7] == PROMPT | 4
    want[5, 100] -= 1
    table = _dev(before)
    token_counts_add(table, _dev(tok), _dev(slot2))
    assert np.array_equal(table.cpu().numpy(), want)
    token_counts_add(table, _dev(tok[:0]), _dev(slot[:0]))  # no rows: nothing


# ---------------------------------------------------------------- logprob_rows
KS = (0, 1, 5, 20, 32, 40)
SENTINEL = -7.0


@lru_cache(maxsize=None)
def _lp_case(cols: int, rows: int):
    """Rows by kind (j % 6): 0 random logits with a planted tie that straddles the
    5th place, 1 all equal, 2 three finite values in a row of -inf, 3 a NaN,
    4 skipped, 5 zeros of both signs on top. Reference for k = 32, once."""
    from kgs.ops.transformer import logprob_rows_reference

    g = torch.Generator().manual_seed(cols + rows)
    x = torch.randn(rows, cols, generator=g).mul(2).bfloat16()
    kinds = np.arange(rows) % 6
    for j, kind in enumerate(kinds):
        pos = torch.randperm(cols, generator=g)
        if kind == 0:  # three 16s above seven 15s (cols 8: five 15s), far above the noise
            x[j, pos[3:10]] = 15.0
            x[j, pos[:3]] = 16.0
        elif kind == 1:
            x[j] = 1.5
        elif kind == 2:
            x[j] = float("-inf")
            x[j, pos[:3]] = torch.tensor([0.5, -2.0, 0.5]).bfloat16()
        elif kind == 3:
            x[j, pos[0]] = float("nan")
        elif kind == 5:
            x[j] = -x[j].abs() - 0.5
            x[j, pos[:6]] = torch.tensor([0.0, -0.0, -0.0, 0.0, -0.0, 0.0]).bfloat16()
    tok = torch.randint(0, cols, (rows,), generator=g).numpy()
    if rows >= 3:
        tok[1], tok[2] = cols, -1  # outside the row: NaN
    skip = kinds == 4
    lp, tv, ti = logprob_rows_reference(x, tok, np.where(skip, -1, 32))
    return x, tok, skip, (lp, tv, ti)


def _run_lp(x, tok, want, wide=True):
    from kgs.ops.transformer import logprob_rows

    rows = x.shape[0]
    lp = torch.full((rows,), SENTINEL, device="cuda")
    tv = torch.full((rows, 32), SENTINEL, device="cuda")
    ti = torch.full((rows, 32), int(SENTINEL), dtype=torch.int32, device="cuda")
    xd = _wide(x) if wide else x.cuda()
    out = logprob_rows(xd, _dev(tok.astype(np.int64)), _dev(want.astype(np.int32)), lp, tv, ti)
    assert out[0] is lp and out[1] is tv and out[2] is ti
    return lp.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()


def _close(got, ref):
    """got within LP_TOL of ref wherever |ref| <= 64; -inf and NaN exactly where ref has them."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got == -np.inf, ref == -np.inf)
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all()
    chk = fin & (np.abs(ref) <= 64)
    err = np.abs(got[chk] - ref[chk])
    assert err.size == 0 or err.max() <= LP_TOL, err.max()


@pytest.mark.parametrize("rows", [1, 3, 33])
@pytest.mark.parametrize("cols", COLS)
def test_logprob_rows_matches_reference(cols, rows):
    x, tok, skip, (rlp, rtv, rti) = _lp_case(cols, rows)
    for k in KS:
        kk = min(k, cols, 32)
        lp, tv, ti = _run_lp(x, tok, np.where(skip, -1, k))
        assert (lp[skip] == SENTINEL).all() and (tv[skip] == SENTINEL).all() and (ti[skip] == SENTINEL).all()
        assert (tv[:, kk:] == SENTINEL).all() and (ti[:, kk:] == SENTINEL).all()  # entries past k: untouched
        assert np.array_equal(ti[~skip, :kk], rti[~skip, :kk]), (cols, rows, k)
        _close(lp[~skip], rlp[~skip])
        _close(tv[~skip, :kk], rtv[~skip, :kk])
    if rows == 33:  # the kinds are all there, and do what they are there for
        assert np.isnan(rlp[3]) and rti[3, :3].tolist() == [0, 1, 2]
        if cols >= 520:
            ties = np.flatnonzero(x[0].float().numpy() == 15.0)
            assert len(ties) == 7 and sorted(rti[0, 3:5].tolist()) == ties[:2].tolist()  # the lowest two of seven
            assert (rtv[2, 3:] == -np.inf).all() and np.isfinite(rtv[2, :3]).all()
            z = np.flatnonzero(x[5].float().numpy() == 0.0)
            assert rti[5, :6].tolist() == z.tolist()  # -0 and +0 tie: by index
        assert rti[1].tolist() == list(range(min(cols, 32))) + [-1] * (32 - min(cols, 32))


@pytest.mark.parametrize("cols", COLS)
def test_torch_log_softmax_meets_the_same_bound(cols):
    """The route logprob_rows replaces (fp32 log_softmax, gather, topk) on the same inputs and the same bound."""
    x, tok, skip, (rlp, rtv, rti) = _lp_case(cols, 33)
    lsm = torch.log_softmax(x.cuda().float(), dim=-1).cpu().numpy()
    rows = np.flatnonzero(~skip & ~np.isnan(x.float().numpy()).any(1))
    ok = rows[(tok[rows] >= 0) & (tok[rows] < cols)]
    _close(lsm[ok, tok[ok]], rlp[ok])
    kk = min(cols, 32)
    _close(np.take_along_axis(lsm[rows], rti[rows, :kk], axis=1), rtv[rows, :kk])


def test_logprob_rows_is_deterministic_and_row_independent():
    x, tok, skip, _ = _lp_case(4104, 33)
    want = np.where(skip, -1, 20)
    a = _run_lp(x, tok, want)
    b = _run_lp(x, tok, want, wide=False)  # another launch, another row stride
    perm = np.random.default_rng(0).permutation(33)
    c = _run_lp(x[torch.from_numpy(perm)], tok[perm], want[perm])
    for u, v, w in zip(a, b, c):
        assert np.array_equal(u, v, equal_nan=True) and np.array_equal(u[perm], w, equal_nan=True)
    for j in (0, 8, 32):  # alone
        for u, w in zip(a, _run_lp(x[j:j + 1], tok[j:j + 1], want[j:j + 1])):
            assert np.array_equal(u[j:j + 1], w, equal_nan=True)


def test_logprob_rows_zero_rows_and_kernel_errors():
    from kgs.ops import KernelError
    from kgs.ops.transformer import logprob_rows

    def args(rows, cols):
        return (torch.zeros(rows, cols, dtype=torch.bfloat16, device="cuda"),
                torch.zeros(rows, dtype=torch.int64, device="cuda"),
                torch.zeros(rows, dtype=torch.int32, device="cuda"))

    lp, tv, ti = logprob_rows(*args(0, 16))
    assert lp.shape == (0,) and tv.shape == (0, 32) and ti.shape == (0, 32)
    with pytest.raises(KernelError):
        logprob_rows(*args(2, 12))  # cols % 8
    lp, tv, ti = logprob_rows(*args(2, 16))  # buffers made by the wrapper: NaN / -1 past k
    assert np.allclose(lp.cpu().numpy(), -np.log(16)) and torch.isnan(tv).all() and (ti == -1).all()


# ------------------------------------------------------------------ engine
def _cfg():
    from kgs.models.llama import LlamaConfig

    return LlamaConfig(hidden=512, intermediate=1024, heads=4, kv_heads=1, layers=2, vocab=1024)


def _engine(**kw):
    from kgs.serve import EngineConfig, LLMEngine

    kw.setdefault("device_sampler", True)
    kw.setdefault("device_logit_ops", True)
    kw.setdefault("num_pages", 256)
    ec = EngineConfig(max_batch=8, max_model_len=1024, cuda_graphs=False, **kw)
    return LLMEngine(_cfg(), ec, device="cuda", backend="kgs")


def _prompts():
    rng = np.random.default_rng(7)
    return [rng.integers(3, 1024, size=n).tolist() for n in (30, 28, 31, 29)]  # each grows across a page boundary


def _params():
    from kgs.serve import SamplingParams

    return [SamplingParams(max_tokens=8, frequency_penalty=0.5, presence_penalty=0.3, ignore_eos=True),
            SamplingParams(max_tokens=8, temperature=0.8, top_k=40, top_p=0.9, seed=1234, repetition_penalty=1.3,
                           ignore_eos=True),
            SamplingParams(max_tokens=8, ignore_eos=True),
            SamplingParams(max_tokens=8, logprobs=3, ignore_eos=True)]


def _result(outs):
    return [(r.output, r.logprobs) for r in outs]


PEN, SEEDED, PLAIN, LP = range(4)  # the requests of _params()


@lru_cache(maxsize=None)
def _batched(overlap: bool, num_pages: int = 256, newest: int = LP):
    """The four requests in one batch, `newest` admitted last (the scheduler
    preempts the newest sequence); results in _params()' order."""
    eng = _engine(overlap=overlap, num_pages=num_pages)
    assert eng.device_logit_ops and eng.device_sampler
    order = [(newest + 1 + j) % 4 for j in range(4)]
    outs = eng.generate([_prompts()[j] for j in order], [_params()[j] for j in order])
    outs = [outs[order.index(j)] for j in range(4)]
    assert [len(r.output) for r in outs] == [8] * 4 and [len(r.logprobs) for r in outs] == [0, 0, 0, 8]
    assert eng.sampler.counts is not None and eng.sampler.counts.used == 0  # every slot is free again
    return _result(outs), dict(eng.stats)


def test_engine_mixed_batch_is_the_same_overlapped_sequential_alone_and_preempted():
    """Tokens and logprobs of the mixed batch: overlapped, sequential, each
    request alone, and under forced preemption, all identical.

    The preempted run admits the penalised request last, so that it is the one
    preempted: its count-table slot has to survive the recompute for its tokens
    to come out the same. A preempted request's later logits are not bit-stable
    in this engine, with or without device_logit_ops: the recompute runs the
    prompt pass over tokens the first run decoded one by one. Measured on an
    MI355X with the logprobs request preempted instead (after its 4th token):
    every token of every request still equal, but that request's logprobs of
    tokens 5 to 8 differ by 0.0148 to 0.0158 (one bf16 step of a logit near 2),
    the same figures with device_logit_ops off and with the torch sampler. So
    for that arrangement the test holds the tokens only."""
    on, _ = _batched(True)
    off, _ = _batched(False)
    assert on == off
    for j in range(4):
        eng = _engine(overlap=True)
        alone = _result(eng.generate(_prompts()[j:j + 1], _params()[j:j + 1]))
        assert alone[0] == on[j], j
        assert eng.sampler.counts is None or eng.sampler.counts.used == 0
    # 6 usable pages for 4 sequences that need 8: preemption + recompute
    pre, stats = _batched(True, num_pages=7, newest=PEN)
    assert stats["preemptions"] >= 1
    assert pre == on
    pre, stats = _batched(True, num_pages=7, newest=LP)
    assert stats["preemptions"] >= 1
    assert [t for t, _ in pre] == [t for t, _ in on] and [len(lp) for _, lp in pre] == [0, 0, 0, 8]
    # the logprobs request: 3 entries per token, sorted, the sampled (greedy) token first
    for tok, (lp, top) in zip(on[LP][0], on[LP][1]):
        assert len(top) == 3 and top[0][0] == tok and top[0][1] == lp and top[0][1] >= top[1][1] >= top[2][1]


def test_engine_penalised_and_logprob_requests_stay_overlapped():
    from kgs.serve import SamplingParams

    eng = _engine(overlap=True)
    rids = [eng.add_request(p, q) for p, q in zip(_prompts(), _params())]
    assert eng._overlap_now()
    seen = 0
    while eng.has_work():
        eng.step()
        if eng.has_work():
            assert eng._overlap_now() and eng._inflight is not None
            seen += 1
    assert seen >= 6 and eng.sampler.counts.used == 0
    assert [len(eng.requests[r].output) for r in rids] == [8] * 4
    # more than 32 logprobs: the blocking route, one step at a time, for as long as that request runs
    eng = _engine(overlap=True)
    big = SamplingParams(max_tokens=4, logprobs=40, ignore_eos=True)
    rid = eng.add_request(_prompts()[0], big)
    assert not eng._overlap_now()
    eng.abort(rid)
    assert eng._overlap_now()
    outs = eng.generate([_prompts()[0], _prompts()[LP]], [big, _params()[LP]])
    assert [len(r.logprobs) for r in outs] == [4, 8] and all(len(top) == 40 for _, top in outs[0].logprobs)
    assert _result(outs[1:]) == [_batched(True)[0][LP]]  # its batch mate's logprobs still come from the kernel
    for tok, (lp, top) in zip(outs[0].output, outs[0].logprobs):
        assert top[0][0] == tok and abs(top[0][1] - lp) <= LP_TOL


def test_engine_strong_presence_penalty_never_repeats_and_abort_frees_the_slot():
    from kgs.serve import SamplingParams

    eng = _engine(overlap=True)
    p = SamplingParams(max_tokens=24, presence_penalty=100.0, ignore_eos=True)
    out = eng.generate(_prompts()[:1], [p])[0].output
    assert len(out) == 24 and len(set(out)) == 24
    # an EOS the request samples as its third token: seen one step late, the extra step's token is dropped
    eng = _engine(overlap=True, eos_token_id=out[2])
    r = eng.generate(_prompts()[:1], [dataclasses.replace(p, ignore_eos=False)])[0]
    assert r.output == out[:3] and r.finish_reason == "stop" and eng.sampler.counts.used == 0
    eng = _engine(overlap=False)
    rid = eng.add_request(_prompts()[1], p)
    for _ in range(3):
        eng.step()
    assert eng.sampler.counts.used == 1 and eng.sampler.counts.slot(rid) >= 0
    eng.abort(rid)
    assert eng.sampler.counts.used == 0 and not eng.has_work()


def test_engine_unpenalised_greedy_tokens_equal_the_flag_off_engine_and_the_argmax():
    from kgs.serve import SamplingParams

    on, _ = _batched(True)
    off = _engine(device_logit_ops=False).generate(_prompts(), _params())
    assert on[PLAIN][0] == off[PLAIN].output
    # an unpenalised greedy request with logprobs: every recorded top-1 is the token the sampler's argmax picked
    p = SamplingParams(max_tokens=8, logprobs=1, ignore_eos=True)
    plain = _engine(device_logit_ops=False, device_sampler=False).generate(
        _prompts()[PLAIN:PLAIN + 1], [dataclasses.replace(p, logprobs=None)])[0].output
    r = _engine().generate(_prompts()[PLAIN:PLAIN + 1], [p])[0]
    assert r.output == plain == on[PLAIN][0] and [top[0][0] for _, top in r.logprobs] == plain
