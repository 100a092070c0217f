"""Shared by tests/test_embedding.py (CPU) and tests/test_embedding_gpu.py: the
criterion of the embedding's scatter-sum backward and the token distributions.
As in tests/forward_refs.py, the GPU tests apply the criterion to the kernel's
output and the CPU test applies the same function to the fp32 baseline (must be
accepted) and to deliberately wrong evaluations (must be rejected). Nothing in
here is measured against a kernel.
"""
import torch

from forward_refs import within
from kgs.ops.embedding import ref_embedding_rows_backward


def check_embedding_backward(dw, dy, tok, vocab, scale=1.0, padding_idx=None, what="embedding_rows_backward"):
    """``|dw - ref64| <= 2^-7 |ref64| + n_v 2^-24 |scale| sum_t |dy_t|`` per element, with
    ``n_v`` the number of tokens summed into row ``v`` and the sum over those tokens:
    one bf16 rounding plus the textbook bound of an fp32 sum of ``n_v`` terms in any
    order. A row without a token has ref64 = 0 and n_v = 0: it must be exactly zero."""
    assert dw.dtype == torch.bfloat16 and tuple(dw.shape) == (vocab, dy.shape[-1])
    ref = ref_embedding_rows_backward(dy, tok, vocab, scale, padding_idx)
    mass = ref_embedding_rows_backward(dy.abs(), tok, vocab, abs(scale), padding_idx)
    n_v = ref_embedding_rows_backward(torch.ones_like(dy[..., :1]), tok, vocab, 1.0, padding_idx)
    within(dw, ref, n_v * 2.0 ** -24 * mass, what)
    unused = n_v[:, 0] == 0
    assert int(dw[unused].view(torch.int16).count_nonzero()) == 0, f"{what}: a row with no token is not zero bits"
    return ref


def uniform_tokens(rows, vocab, gen, device="cpu"):
    return torch.randint(0, vocab, (rows,), generator=gen, device=device)


def zipf_tokens(rows, vocab, gen, device="cpu"):
    """Log-uniform over [0, vocab): P(token = k) ~ 1 / (k + 1), Zipf with exponent 1.
    Small ids come in long runs, most large ids not at all."""
    u = torch.rand(rows, generator=gen, device=device, dtype=torch.float64)
    return (torch.exp(u * torch.log(torch.tensor(vocab + 1.0, dtype=torch.float64))) - 1).long().clamp_(0, vocab - 1)
