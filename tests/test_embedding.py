"""CPU tests of the token embedding (the kernels themselves:
tests/test_embedding_gpu.py): the float64 references against torch, the backward's
criterion against the fp32 baseline and against wrong evaluations, the argument
checks, which raise before the native library is touched, tied weights in
DecoderLM's torch backend, and the kernels' compile-time resources."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from embedding_refs import check_embedding_backward, uniform_tokens, zipf_tokens
from kgs.ops.embedding import (Embedding, embedding, embedding_rows, embedding_rows_backward, ref_embedding_rows,
                               ref_embedding_rows_backward)

F64 = torch.float64
TOL = 1e-12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------
# the references against torch

def _with_strays(tok, vocab):
    """``tok`` with out-of-range values in four places, and the mask of the places kept."""
    tok = tok.clone()
    tok[1], tok[4], tok[7], tok[10] = -100, vocab, vocab + 7, 2 ** 32 + 3
    return tok, (tok >= 0) & (tok < vocab)


@pytest.mark.parametrize("scale", [1.0, 0.5, 8.0])
def test_ref_embedding_rows_is_torchs_embedding(scale):
    g = _gen(1)
    vocab, cols = 11, 16
    w = torch.randn(vocab, cols, generator=g, dtype=F64)
    tok, ok = _with_strays(uniform_tokens(23, vocab, g), vocab)
    want = torch.zeros(23, cols, dtype=F64)
    want[ok] = torch.nn.functional.embedding(tok[ok], w) * scale
    got = ref_embedding_rows(w, tok, scale)
    assert got.dtype == F64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= TOL
    assert (got[~ok] == 0).all()
    # any token shape is flattened; float32 is the baseline's dtype
    assert torch.equal(ref_embedding_rows(w, tok[:20].reshape(4, 5), scale), got[:20])
    assert ref_embedding_rows(w.bfloat16(), tok, scale, dtype=torch.float32).dtype == torch.float32


@pytest.mark.parametrize("padding_idx", [None, 3])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_ref_embedding_rows_backward_is_autograds_gradient(scale, padding_idx):
    g = _gen(2)
    vocab, cols, rows = 11, 16, 40
    w = torch.randn(vocab, cols, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(rows, cols, generator=g, dtype=F64)
    tok, ok = _with_strays(zipf_tokens(rows, vocab, g), vocab)
    tok[12] = 3  # the padding row is used
    out = torch.nn.functional.embedding(tok[ok], w, padding_idx=padding_idx) * scale
    (want,) = torch.autograd.grad(out, w, dy[ok])
    got = ref_embedding_rows_backward(dy, tok, vocab, scale, padding_idx)
    assert got.dtype == F64 and got.shape == (vocab, cols)
    assert (got - want).abs().max().item() <= TOL
    if padding_idx is not None:
        assert (got[padding_idx] == 0).all()
    assert (got[3] != 0).any() == (padding_idx is None)


# ----------------------------------------------------------------------------
# the criterion: accepts the fp32 baseline, rejects wrong evaluations

def _sequential(dy, tok, vocab, scale=1.0, descending=False, drop_last=False, round_each=False):
    """dw by one pass over the positions, as a kernel would: an fp32 accumulator per
    row, rounded once at the end (or after every addition: ``round_each``)."""
    acc = torch.zeros(vocab, dy.shape[1], dtype=torch.float32)
    last = {int(v): t for t, v in enumerate(tok.tolist())}
    count = torch.bincount(tok[(tok >= 0) & (tok < vocab)], minlength=vocab)
    pos = range(tok.numel() - 1, -1, -1) if descending else range(tok.numel())
    for t in pos:
        v = int(tok[t])
        if not 0 <= v < vocab or (drop_last and count[v] > 1 and last[v] == t):
            continue
        acc[v] += dy[t].float()
        if round_each:
            acc[v] = acc[v].bfloat16().float()
    return (acc * scale).bfloat16()


@pytest.mark.parametrize("tokens", [uniform_tokens, zipf_tokens])
def test_backward_criterion_accepts_the_fp32_sum_in_either_order(tokens):
    g = _gen(3)
    vocab, cols, rows = 1000, 16, 2053
    dy = torch.randn(rows, cols, generator=g).bfloat16()
    tok, _ = _with_strays(tokens(rows, vocab, g), vocab)
    for scale in (1.0, 0.5):
        for descending in (False, True):
            check_embedding_backward(_sequential(dy, tok, vocab, scale, descending), dy, tok, vocab, scale)
    # the float32 reference rounded once is the same baseline
    check_embedding_backward(ref_embedding_rows_backward(dy, tok, vocab, dtype=torch.float32).bfloat16(), dy, tok,
                             vocab)


def test_backward_criterion_rejects_a_dropped_occurrence():
    g = _gen(4)
    vocab, cols, rows = 1000, 16, 2053
    dy = torch.randn(rows, cols, generator=g).bfloat16()
    tok = zipf_tokens(rows, vocab, g)
    with pytest.raises(AssertionError):
        check_embedding_backward(_sequential(dy, tok, vocab, drop_last=True), dy, tok, vocab)


def test_backward_criterion_rejects_a_rounding_after_every_addition():
    """2053 occurrences of one token, dy of one sign: a bf16 accumulator stops growing
    once an addend is under half its spacing, long before the true sum is reached."""
    g = _gen(5)
    vocab, cols, rows = 3, 16, 2053
    dy = (0.5 + torch.rand(rows, cols, generator=g)).bfloat16()
    tok = torch.full((rows,), 1, dtype=torch.int64)
    check_embedding_backward(_sequential(dy, tok, vocab), dy, tok, vocab)
    with pytest.raises(AssertionError):
        check_embedding_backward(_sequential(dy, tok, vocab, round_each=True), dy, tok, vocab)


def test_backward_criterion_rejects_an_unused_row_left_non_zero():
    g = _gen(6)
    vocab, cols, rows = 1000, 16, 5
    dy = torch.randn(rows, cols, generator=g).bfloat16()
    tok = torch.tensor([3, 17, 3, 999, 500])
    dw = _sequential(dy, tok, vocab)
    check_embedding_backward(dw, dy, tok, vocab)
    dw[4, 9] = 2.0 ** -30  # what an uninitialised buffer may hold
    with pytest.raises(AssertionError):
        check_embedding_backward(dw, dy, tok, vocab)
    dw[4, 9] = -0.0  # zero, but not zero bits: the kernel writes the row itself
    with pytest.raises(AssertionError, match="zero bits"):
        check_embedding_backward(dw, dy, tok, vocab)


# ----------------------------------------------------------------------------
# argument checks: raised before the native library is loaded (there is no GPU here)

def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


@pytest.fixture
def no_native(monkeypatch):
    from kgs.ops import _lib

    def boom():
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(_lib, "lib", boom)


def test_embedding_rows_checks_its_arguments(no_native):
    w, tok = _bf(10, 16), torch.zeros(4, dtype=torch.int64)
    for fn in (embedding_rows, embedding, lambda a, b, *r: embedding(a.requires_grad_(True), b, *r)):
        with pytest.raises(TypeError):
            fn(w.float(), tok)
        with pytest.raises(TypeError):
            fn(w, tok.int())
        with pytest.raises(TypeError):
            fn(w, tok, torch.ones(1))
        with pytest.raises(ValueError, match="multiple of 8"):
            fn(_bf(10, 12), tok)
        with pytest.raises(ValueError, match="row-major"):
            fn(_bf(16, 10).t(), tok)
        with pytest.raises(ValueError, match="row-major"):
            fn(_bf(10, 16, 2), tok)
        with pytest.raises(ValueError, match="row stride"):
            fn(_bf(10, 20)[:, :16], tok)
        with pytest.raises(ValueError, match="GPU"):
            fn(w, tok)
        with pytest.raises(ValueError, match="GPU"):
            fn(w, tok.reshape(2, 2))
    with pytest.raises(TypeError):
        embedding_rows(w, tok, out=_bf(4, 16).float())
    with pytest.raises(ValueError):
        embedding_rows(w, tok, out=_bf(5, 16))
    with pytest.raises(ValueError):
        embedding_rows(w, tok, out=_bf(4, 24))
    with pytest.raises(ValueError, match="padding_idx"):
        embedding(w, tok, padding_idx=10)
    with pytest.raises(ValueError, match="padding_idx"):
        embedding(w, tok, padding_idx=-1)
    with pytest.raises(TypeError):
        embedding(w, tok, padding_idx=1.0)


def test_embedding_rows_backward_checks_its_arguments(no_native):
    dy, tok = _bf(4, 16), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError):
        embedding_rows_backward(dy.float(), tok, 10)
    with pytest.raises(TypeError):
        embedding_rows_backward(dy, tok.int(), 10)
    with pytest.raises(TypeError):
        embedding_rows_backward(dy, tok, 10.0)
    with pytest.raises(TypeError):
        embedding_rows_backward(dy, tok, 10, scale="1")
    with pytest.raises(TypeError):
        embedding_rows_backward(dy, tok, 10, out=_bf(10, 16).float())
    with pytest.raises(ValueError, match="multiple of 8"):
        embedding_rows_backward(_bf(4, 12), tok, 10)
    with pytest.raises(ValueError, match="row-major"):
        embedding_rows_backward(_bf(16, 4).t(), tok, 10)
    with pytest.raises(ValueError, match="row stride"):
        embedding_rows_backward(_bf(4, 20)[:, :16], tok, 10)
    with pytest.raises(ValueError, match="rows"):
        embedding_rows_backward(dy, tok[:3], 10)
    with pytest.raises(ValueError, match="vocab"):
        embedding_rows_backward(dy, tok, 0)
    with pytest.raises(ValueError, match="vocab"):
        embedding_rows_backward(dy, tok, 2 ** 31)
    with pytest.raises(ValueError, match="padding_idx"):
        embedding_rows_backward(dy, tok, 10, padding_idx=10)
    with pytest.raises(ValueError):
        embedding_rows_backward(dy, tok, 10, out=_bf(9, 16))
    with pytest.raises(ValueError):
        embedding_rows_backward(dy, tok, 10, out=_bf(10, 24))
    with pytest.raises(ValueError, match="GPU"):
        embedding_rows_backward(dy, tok, 10, padding_idx=9)
    with pytest.raises(ValueError, match="GPU"):
        embedding_rows_backward(dy, tok.reshape(2, 2), 10, scale=0.5, out=_bf(10, 16))


def test_embedding_module_on_the_cpu(no_native):
    with pytest.raises(ValueError, match="multiple of 8"):
        Embedding(10, 12)
    with pytest.raises(ValueError, match="padding_idx"):
        Embedding(10, 16, padding_idx=10)
    m = Embedding(10, 16, padding_idx=2, scale=4.0)
    assert isinstance(m.weight, torch.nn.Parameter) and m.weight.dtype == torch.bfloat16
    assert m.weight.shape == (10, 16) and (m.weight[2] == 0).all() and (m.weight[3] != 0).any()
    assert [n for n, _ in m.named_parameters()] == ["weight"]
    with pytest.raises(ValueError, match="GPU"):
        m(torch.zeros(2, 3, dtype=torch.int64))


def test_ops_are_exported_from_kgs_ops():
    import kgs.ops
    import kgs.ops.embedding as module

    for name in ("embedding", "Embedding", "embedding_rows", "embedding_rows_backward", "ref_embedding_rows",
                 "ref_embedding_rows_backward"):
        assert callable(getattr(kgs.ops, name)), name
    assert kgs.ops.Embedding is Embedding and kgs.ops.embedding_rows is embedding_rows
    # the op shares its name with its module: kgs.ops.embedding(...) is the op either way
    assert module.embedding is embedding
    w, tok = _bf(10, 16), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        kgs.ops.embedding(w, tok)
    with pytest.raises(TypeError):
        kgs.ops.embedding(w.float(), tok)


# ----------------------------------------------------------------------------
# DecoderLM: tied weights, on the torch backend

def test_decoder_lm_ties_the_head_to_the_embedding():
    from kgs.models.decoder import DecoderLM

    args = (64, 32, 2, 2, 1, 48)
    kw = dict(backend="torch", device="cpu", dtype=torch.float32)
    tied, twin = DecoderLM(*args, tie_embeddings=True, **kw), DecoderLM(*args, **kw)
    assert tied.head.weight is tied.embed.weight and twin.head.weight is not twin.embed.weight
    names = [n for n, _ in tied.named_parameters()]
    assert names == [n for n, _ in twin.named_parameters() if n != "head.weight"]
    assert len(list(tied.parameters())) == len(list(twin.parameters())) - 1
    assert "embed.weight" in names and "head.weight" not in names
    # the shared weight takes the head's init; everything else is the untied model's
    assert torch.equal(tied.embed.weight, twin.head.weight)
    assert tied.embed.weight.std().item() < 2 * 32 ** -0.5
    with torch.no_grad():
        twin.embed.weight.copy_(tied.embed.weight)
    g = _gen(7)
    tokens = torch.randint(0, 64, (2, 8), generator=g)
    targets = tokens.roll(-1, 1).clone()
    targets[:, -1] = -100
    lt, lu = tied.loss(tokens, targets), twin.loss(tokens, targets)
    assert torch.equal(lt, lu)
    lt.backward()
    lu.backward()
    both = twin.embed.weight.grad + twin.head.weight.grad
    assert twin.embed.weight.grad.abs().max() > 0 and twin.head.weight.grad.abs().max() > 0
    assert (tied.embed.weight.grad - both).abs().max().item() <= 1e-6 * both.abs().max().item()
    for (n, p), (m, q) in zip(tied.named_parameters(), ((m, q) for m, q in twin.named_parameters()
                                                         if m != "head.weight")):
        if n != "embed.weight":
            assert n == m and torch.equal(p.grad, q.grad), n
    # the defaults are today's model
    assert twin.embedding == "torch" and not twin.tie_embeddings and isinstance(twin.embed, torch.nn.Embedding)


def test_decoder_lm_checks_the_embedding_argument():
    from kgs.models.decoder import DecoderLM

    with pytest.raises(ValueError, match="kgs backend"):
        DecoderLM(64, 32, 1, 2, 1, 48, backend="torch", device="cpu", embedding="kgs")
    with pytest.raises(ValueError, match="embedding"):
        DecoderLM(64, 32, 1, 2, 1, 48, backend="torch", device="cpu", embedding="hip")


# ----------------------------------------------------------------------------
# compile-time resources (hipcc cross-compiles gfx950 without a GPU)

@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_embedding_kernels_use_no_scratch(tmp_path):
    """Both kernels: no spilled VGPR, no scratch. The backward keeps eight 16-B loads
    in flight next to its accumulators; a regression here slows every training step."""
    root = Path(__file__).resolve().parents[1]
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", str(root / "native/kernels"),
                          str(root / "native/kernels/embedding.hip"), "-o", str(tmp_path / "embedding.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600,
                         cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    assert len(res) == 2 and any("embed_fwd" in n for n in res) and any("embed_bwd" in n for n in res), sorted(res)
    assert all("ScratchSize" in r and "VGPRs Spill" in r and "VGPRs" in r for r in res.values()), res
    bad = {n: r for n, r in res.items() if r["ScratchSize"] or r["VGPRs Spill"]}
    assert not bad, bad
    assert all(r["VGPRs"] <= 128 for r in res.values()), res  # four waves per SIMD at the least
