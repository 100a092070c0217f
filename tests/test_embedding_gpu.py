"""GPU tests of the token embedding (native/kernels/embedding.hip): the gather
forward, the dense scatter-sum backward, the autograd op, graph capture, and
DecoderLM with the kgs embedding and tied weights.

The forward is exact: a bit copy at scale 1, one rounding of one product
otherwise. The backward is held to the criterion of
tests/embedding_refs.py against float64: ``|dw - ref64| <= 2^-7 |ref64| + n_v 2^-24
|scale| sum |dy_t|``, and zero bits in every row without a token.

Shapes: 8 columns is one 16-byte chunk, 520 is no multiple of a wave's 512-column
slice, 1536 and 4096 are several slices; 2053 rows make runs longer than any
unrolled batch; 3 and 1000 vocabulary rows are less and more than one wave's 32,
and 70001 rows (at 8 columns) are more than 65535."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from embedding_refs import check_embedding_backward, uniform_tokens, zipf_tokens
from forward_refs import POISON, poison_intact as _poison_intact, same_bits as _same_bits, wide as _wide

pytestmark = pytest.mark.gpu

DEV = "cuda"
COLS = (8, 520, 1536, 4096)
ROWS = (1, 5, 2053)
SHAPES = [(r, c, v) for c in COLS for r in ROWS for v in (3, 1000)] + [(r, 8, 70001) for r in ROWS]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g).bfloat16()


def _zero_bits(t):
    return int(t.contiguous().view(torch.int16).count_nonzero()) == 0


def _strays(vocab):
    return torch.tensor([-100, vocab, vocab + 7, 2 ** 32 + 3], device=DEV)


@functools.lru_cache(maxsize=None)
def _case(rows, cols, vocab, dist="uniform"):
    """Inputs and the kernels' outputs of one case, computed once and shared by the
    tests (nothing below modifies them)."""
    from kgs.ops.embedding import embedding_rows, embedding_rows_backward

    g = _gen(rows * 31 + cols + vocab)
    w, dy = _randn(g, vocab, cols), _randn(g, rows, cols)
    tok = {"uniform": uniform_tokens, "zipf": zipf_tokens}[dist](rows, vocab, g, DEV)
    out = embedding_rows(w, tok)
    dw = embedding_rows_backward(dy, tok, vocab)
    torch.cuda.synchronize()
    return {"w": w, "dy": dy, "tok": tok, "out": out, "dw": dw}


# ----------------------------------------------------------------------------
# forward

@pytest.mark.parametrize("rows,cols,vocab", SHAPES)
def test_forward_is_a_bit_copy_of_the_rows(rows, cols, vocab):
    from kgs.ops.embedding import embedding_rows

    c = _case(rows, cols, vocab)
    want = c["w"][c["tok"]]
    assert c["out"].shape == (rows, cols) and c["out"].dtype == torch.bfloat16
    assert torch.equal(c["out"], want) and _same_bits(c["out"], want)
    ww, _ = _wide(c["w"])  # a table whose row stride is wider than cols
    assert ww.stride(0) > cols
    assert _same_bits(embedding_rows(ww, c["tok"]), want)
    out, buf = _wide(torch.zeros_like(want), pad=72)
    got = embedding_rows(c["w"], c["tok"], out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _same_bits(out, want)
    assert _poison_intact(buf, rows, cols)


@pytest.mark.parametrize("scale", [0.5, 64.0])
@pytest.mark.parametrize("rows,cols,vocab", [(5, 8, 3), (2053, 520, 1000), (5, 4096, 1000), (2053, 8, 70001)])
def test_forward_scales_and_rounds_once(rows, cols, vocab, scale):
    from kgs.ops.embedding import embedding_rows

    c = _case(rows, cols, vocab)
    want = (c["w"][c["tok"]].float() * scale).bfloat16()
    assert torch.equal(embedding_rows(c["w"], c["tok"].reshape(rows, 1), scale), want)


@pytest.mark.parametrize("cols,vocab", [(8, 3), (520, 1000), (8, 70001)])
def test_out_of_range_tokens_are_zero_rows_and_contribute_nothing(cols, vocab):
    """-100, vocab, vocab + 7 and 2^32 + 3: the last is compared as 64 bits, so row 3
    (of 1000 or 70001) neither supplies its row nor gets a share of its gradient."""
    from kgs.ops.embedding import embedding_rows, embedding_rows_backward

    g = _gen(5)
    rows = 12
    w, dy = _randn(g, vocab, cols), _randn(g, rows, cols)
    tok = uniform_tokens(rows, vocab, g, DEV)
    tok[tok == 3] = 0
    tok[[1, 4, 7, 10]] = _strays(vocab)
    tok[2] = min(3, vocab - 1)
    ok = (tok >= 0) & (tok < vocab)
    assert int(ok.sum()) == rows - 4
    out = embedding_rows(w, tok)
    assert torch.equal(out[ok], w[tok[ok]]) and _zero_bits(out[~ok])
    dw = embedding_rows_backward(dy, tok, vocab)
    check_embedding_backward(dw, dy, tok, vocab)
    assert _same_bits(dw, embedding_rows_backward(dy[ok], tok[ok], vocab))
    if vocab > 3:
        assert int((tok == 3).sum()) == 1 and torch.equal(dw[3], dy[2])


def test_no_rows():
    from kgs.ops.embedding import embedding_rows, embedding_rows_backward

    w = _randn(_gen(6), 40, 520)
    tok = torch.zeros(0, dtype=torch.int64, device=DEV)
    out = embedding_rows(w, tok)
    assert out.shape == (0, 520) and out.dtype == torch.bfloat16
    dw, buf = _wide(torch.full((40, 520), 7.0, dtype=torch.bfloat16, device=DEV))
    got = embedding_rows_backward(torch.empty(0, 520, dtype=torch.bfloat16, device=DEV), tok, 40, out=dw)
    assert got.data_ptr() == dw.data_ptr() and _zero_bits(dw) and _poison_intact(buf, 40, 520)
    assert _zero_bits(embedding_rows_backward(torch.empty(0, 8, dtype=torch.bfloat16, device=DEV), tok, 70001))


# ----------------------------------------------------------------------------
# backward

@pytest.mark.parametrize("dist", ["uniform", "zipf"])
@pytest.mark.parametrize("rows,cols,vocab", SHAPES)
def test_backward_against_float64(rows, cols, vocab, dist):
    c = _case(rows, cols, vocab, dist)
    check_embedding_backward(c["dw"], c["dy"], c["tok"], vocab, what=f"dw[{rows}x{cols}->{vocab},{dist}]")
    used = torch.zeros(vocab, dtype=torch.bool, device=DEV)
    used[c["tok"]] = True
    assert _zero_bits(c["dw"][~used])


@pytest.mark.parametrize("scale", [0.5, 64.0])
def test_backward_scales_the_sum_before_its_one_rounding(scale):
    from kgs.ops.embedding import embedding_rows_backward

    c = _case(2053, 520, 1000, "zipf")
    dw = embedding_rows_backward(c["dy"], c["tok"], 1000, scale)
    check_embedding_backward(dw, c["dy"], c["tok"], 1000, scale)
    # a power of two commutes with the rounding
    assert torch.equal(dw, (c["dw"].float() * scale).bfloat16())


@pytest.mark.parametrize("cols", COLS)
def test_distinct_tokens_round_a_single_term_exactly(cols):
    from kgs.ops.embedding import embedding_rows_backward

    g = _gen(7)
    dy = _randn(g, 5, cols)
    tok = torch.tensor([999, 0, 31, 32, 517], device=DEV)
    dw = embedding_rows_backward(dy, tok, 1000)
    assert torch.equal(dw[tok], dy)
    check_embedding_backward(dw, dy, tok, 1000)


@pytest.mark.parametrize("cols,vocab,v", [(8, 3, 2), (520, 1000, 0), (4096, 1000, 999), (8, 70001, 65536)])
def test_one_token_2053_times(cols, vocab, v):
    """One run of 2053 rows: longer than any batch of loads a wave keeps in flight."""
    from kgs.ops.embedding import embedding_rows_backward

    dy = _randn(_gen(8), 2053, cols)
    tok = torch.full((2053,), v, device=DEV)
    dw = embedding_rows_backward(dy, tok, vocab)
    check_embedding_backward(dw, dy, tok, vocab)
    rest = torch.ones(vocab, dtype=torch.bool, device=DEV)
    rest[v] = False
    assert _zero_bits(dw[rest]) and not _zero_bits(dw[v])


def _raw_bwd(dy, tok, dw, vocab, cols, scale=1.0, pad=-1, rows=None, dy_off=0, lddw=None):
    from kgs.ops import _lib

    srt, order = torch.sort(tok, stable=True)
    rc = _lib.lib().kgs_embed_bwd_bf16(dy.data_ptr() + dy_off, srt.data_ptr(), order.data_ptr(), dw.data_ptr(),
                                       tok.numel() if rows is None else rows, vocab, cols, dy.stride(0),
                                       dw.stride(0) if lddw is None else lddw, scale, pad,
                                       _lib.stream_handle(dy.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("rows,cols,vocab", [(5, 8, 3), (2053, 520, 1000), (5, 1536, 1000), (2053, 8, 70001)])
def test_raw_entry_overwrites_a_poisoned_dw_and_nothing_else(rows, cols, vocab):
    """dw is a view with a wide row stride inside a poisoned buffer and is not zeroed:
    every element of [vocab, cols] is written, zero or the sum, nothing around it."""
    c = _case(rows, cols, vocab, "zipf")
    buf = torch.full((vocab + 2, cols + 72), POISON, dtype=torch.bfloat16, device=DEV)
    dw = buf[:vocab, 8:8 + cols]
    assert _raw_bwd(c["dy"], c["tok"], dw, vocab, cols) == 0
    assert _same_bits(dw, c["dw"])
    assert _poison_intact(buf, vocab, cols)
    dys, _ = _wide(c["dy"])  # a strided dy: the same bits
    buf2 = torch.full_like(buf, POISON)
    dw2 = buf2[:vocab, 8:8 + cols]
    assert dys.stride(0) > cols and _raw_bwd(dys, c["tok"], dw2, vocab, cols) == 0
    assert _same_bits(dw2, c["dw"]) and _poison_intact(buf2, vocab, cols)


def test_raw_entries_refuse_bad_arguments():
    from kgs.ops import _lib

    c = _case(5, 520, 1000)
    lib, st = _lib.lib(), _lib.stream_handle(torch.device(DEV))
    dw = torch.full((1000, 520), POISON, dtype=torch.bfloat16, device=DEV)
    out = torch.full((5, 520), POISON, dtype=torch.bfloat16, device=DEV)
    err = -3  # KGS_ERR_ARG
    assert _raw_bwd(c["dy"], c["tok"], dw, 1000, 516) == err            # cols % 8
    assert _raw_bwd(c["dy"], c["tok"], dw, 1000, 520, dy_off=2) == err  # misaligned pointer
    assert _raw_bwd(c["dy"], c["tok"], dw, 1000, 520, lddw=524) == err  # stride % 8
    assert _raw_bwd(c["dy"], c["tok"], dw, 1000, 520, rows=-1) == err
    assert _raw_bwd(c["dy"], c["tok"], dw, 0, 520) == err

    def fwd(rows=5, vocab=1000, cols=520, off=0, ldo=520):
        return lib.kgs_embed_fwd_bf16(c["w"].data_ptr() + off, c["tok"].data_ptr(), out.data_ptr(), rows, vocab, cols,
                                      520, ldo, 1.0, st)

    assert fwd(cols=516) == err and fwd(off=2) == err and fwd(ldo=524) == err
    assert fwd(rows=-1) == err and fwd(vocab=0) == err
    assert fwd(rows=0) == 0
    torch.cuda.synchronize()
    assert (dw == POISON).all() and (out == POISON).all()


@pytest.mark.parametrize("rows,cols,vocab", [(2053, 520, 1000), (5, 8, 3)])
def test_padding_idx_zeroes_its_row_and_only_that(rows, cols, vocab):
    from kgs.ops.embedding import embedding_rows_backward

    c = _case(rows, cols, vocab, "zipf")
    pad = int(c["tok"][0])
    assert not _zero_bits(c["dw"][pad])
    dw = embedding_rows_backward(c["dy"], c["tok"], vocab, padding_idx=pad)
    assert _zero_bits(dw[pad])
    keep = torch.ones(vocab, dtype=torch.bool, device=DEV)
    keep[pad] = False
    assert _same_bits(dw[keep], c["dw"][keep])
    check_embedding_backward(dw, c["dy"], c["tok"], vocab, padding_idx=pad)


def test_backward_is_bitwise_repeatable():
    from kgs.ops.embedding import embedding_rows_backward

    c = _case(2053, 4096, 1000, "zipf")
    again = embedding_rows_backward(c["dy"], c["tok"], 1000)
    assert _same_bits(again, c["dw"])
    junk = [torch.full((n,), 3.0, device=DEV) for n in (1 << 20, 12345, 1 << 22, 77)]  # move the allocator on
    del junk[1], junk[2]
    third = embedding_rows_backward(c["dy"].clone(), c["tok"].clone(), 1000)
    assert third.data_ptr() not in (again.data_ptr(), c["dw"].data_ptr())
    assert _same_bits(third, c["dw"])


# ----------------------------------------------------------------------------
# autograd, module, graph capture

@pytest.mark.parametrize("scale,padding_idx", [(1.0, None), (0.5, 1)])
def test_autograd_op_against_float64(scale, padding_idx):
    from kgs.ops.embedding import Embedding, embedding

    g = _gen(9)
    vocab, cols = 1000, 520
    w = _randn(g, vocab, cols)
    tok = zipf_tokens(6 * 40, vocab, g, DEV).reshape(6, 40)
    dy = _randn(g, 6, 40, cols)
    plain = embedding(w, tok, scale, padding_idx)
    assert plain.grad_fn is None and not plain.requires_grad  # nothing saved
    wg = w.clone().requires_grad_(True)
    out = embedding(wg, tok, scale, padding_idx)
    assert out.shape == (6, 40, cols) and torch.equal(out, plain)
    assert torch.equal(out, (w[tok].float() * scale).bfloat16())  # the padding row is returned as it is stored
    with torch.no_grad():
        assert embedding(wg, tok, scale, padding_idx).grad_fn is None
    out.backward(dy)
    first = wg.grad
    check_embedding_backward(first, dy.reshape(-1, cols), tok, vocab, scale, padding_idx)
    # an expanded gradient (sum()'s backward) is made contiguous first
    wg.grad = None
    embedding(wg, tok, scale, padding_idx).sum().backward()
    check_embedding_backward(wg.grad, torch.ones_like(dy), tok, vocab, scale, padding_idx)
    m = Embedding(vocab, cols, padding_idx=padding_idx, scale=scale, device=DEV)
    with torch.no_grad():
        m.weight.copy_(w)
    y = m(tok)
    assert torch.equal(y, plain)
    y.backward(dy)
    assert _same_bits(m.weight.grad, first)


_CAPTURE_CHILD = r"""
import json, torch
from kgs.ops.embedding import embedding
from kgs.utils.graph_audit import audit

dev, vocab, cols, rows = "cuda", 1000, 520, 2053
g = torch.Generator(device=dev).manual_seed(12)
w = torch.randn(vocab, cols, device=dev, generator=g).bfloat16().requires_grad_(True)
toks = [(torch.rand(rows, device=dev, generator=g) ** 3 * vocab).long().clamp_(0, vocab - 1) for _ in range(3)]
dys = [torch.randn(rows, cols, device=dev, generator=g).bfloat16() for _ in range(3)]

def step(tok, dy):
    out = embedding(w, tok)
    (dw,) = torch.autograd.grad(out, w, dy)
    return out, dw

# The eager results are kept detached: an output that keeps its autograd graph alive
# keeps w's AccumulateGrad node alive too, with the stream it was made on (this one),
# and the backward inside the capture would then synchronise the capture stream with it.
eager = [tuple(r.detach() for r in step(t, d)) for t, d in zip(toks, dys)]
tok, dy = toks[0].clone(), dys[0].clone()
torch.cuda.synchronize()
full = torch.cuda.CUDAGraph(keep_graph=True)
with torch.cuda.graph(full):
    out, dw = step(tok, dy)
sort_only = torch.cuda.CUDAGraph(keep_graph=True)
with torch.cuda.graph(sort_only):
    kept = torch.sort(tok, stable=True)
res = {"full": audit(full), "sort": audit(sort_only), "same": []}
for i in (1, 2):
    tok.copy_(toks[i]); dy.copy_(dys[i]); out.detach().zero_(); dw.fill_(5.0)
    full.replay()
    torch.cuda.synchronize()
    res["same"].append([bool(torch.equal(out.view(torch.int16), eager[i][0].view(torch.int16))),
                        bool(torch.equal(dw.view(torch.int16), eager[i][1].view(torch.int16)))])
print("RESULT " + json.dumps(res))
"""


def test_forward_and_backward_replay_from_one_graph():
    """Forward + backward captured once, replayed twice with new tokens and gradients
    copied into the static buffers: each replay equals the eager result bit for bit.
    The kgs entries put no memset node into the graph: the captured step holds as
    many as a graph of the device sort alone."""
    r = subprocess.run([sys.executable, "-c", _CAPTURE_CHILD], capture_output=True, text=True, timeout=120,
                       cwd=Path(__file__).resolve().parents[1])
    print(r.stdout[-4000:], r.stderr[-4000:], sep="\n")
    assert r.returncode == 0, r.returncode
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(res["full"], res["sort"])
    assert res["same"] == [[True, True], [True, True]]
    assert res["full"]["types"].get("kernel", 0) >= res["sort"]["types"].get("kernel", 0) + 2
    assert len(res["full"]["memsets"]) == len(res["sort"]["memsets"])


# ----------------------------------------------------------------------------
# the model

def _copy_rounded(dst, src):
    with torch.no_grad():
        for (n, p), (m, q) in zip(dst.named_parameters(), src.named_parameters()):
            assert n == m
            p.copy_(q.to(p.dtype))


def test_tied_decoder_lm_on_the_kgs_embedding_tracks_the_fp32_copy():
    """test_decoder_lm_sgd_steps_track_the_fp32_copy's procedure and criterion with
    embedding="kgs" and tied weights: eight SGD steps on one fixed seeded batch for kgs,
    a tied torch bf16 model and a tied fp32 copy of the same rounded initial weights.
    The kgs loss falls, and at every step |loss_kgs - loss_fp32| <= 2 |loss_torch -
    loss_fp32| + 1e-4. Then kgs.optim.AdamW drives the same tied model."""
    from kgs.models.decoder import DecoderLM
    from kgs.ops.embedding import Embedding
    from kgs.optim import AdamW

    vocab, dim, nl, nh, nkv, inter, b, s, lr = 1024, 512, 2, 4, 1, 1536, 2, 128, 0.1
    g = _gen(11)
    tokens = torch.randint(0, vocab, (b, s), device=DEV, generator=g)
    targets = tokens.roll(-1, 1).clone()
    targets[:, -1] = -100  # the last position has no next token
    args = (vocab, dim, nl, nh, nkv, inter)
    models = {"kgs": DecoderLM(*args, backend="kgs", embedding="kgs", tie_embeddings=True, device=DEV),
              "torch": DecoderLM(*args, backend="torch", tie_embeddings=True, device=DEV),
              "fp32": DecoderLM(*args, backend="torch", tie_embeddings=True, device=DEV, dtype=torch.float32)}
    kgs = models["kgs"]
    assert isinstance(kgs.embed, Embedding) and kgs.head.weight is kgs.embed.weight
    assert all(m.head.weight is m.embed.weight for m in models.values())
    assert all(torch.equal(p, q) for p, q in zip(kgs.parameters(), models["torch"].parameters()))
    _copy_rounded(models["fp32"], kgs)
    losses = {}
    for name, lm in models.items():
        losses[name] = []
        for _ in range(8):
            lm.zero_grad(set_to_none=True)
            loss = lm.loss(tokens, targets)
            loss.backward()
            with torch.no_grad():
                for p in lm.parameters():
                    p.add_(p.grad, alpha=-lr)
            losses[name].append(loss.item())
        print(name, [f"{v:.4f}" for v in losses[name]])
    assert all(torch.isfinite(torch.tensor(v)).all() for v in losses.values())
    assert losses["kgs"][7] < losses["kgs"][0]
    for i in range(8):
        e_kgs = abs(losses["kgs"][i] - losses["fp32"][i])
        e_base = abs(losses["torch"][i] - losses["fp32"][i])
        print(f"step {i}: kgs {e_kgs:.3e} torch {e_base:.3e}")
    for i in range(8):
        e_kgs = abs(losses["kgs"][i] - losses["fp32"][i])
        e_base = abs(losses["torch"][i] - losses["fp32"][i])
        assert e_kgs <= 2 * e_base + 1e-4, (i, e_kgs, e_base)

    lm = DecoderLM(*args, backend="kgs", embedding="kgs", tie_embeddings=True, device=DEV)
    opt = AdamW(lm.parameters(), lr=1e-3, backend="kgs")
    assert sum(p is lm.embed.weight for g_ in opt.param_groups for p in g_["params"]) == 1
    adam = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss = lm.loss(tokens, targets)
        loss.backward()
        opt.step()
        adam.append(loss.item())
    print("adamw", adam)
    assert all(torch.isfinite(torch.tensor(v)) for v in adam)
