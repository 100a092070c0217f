"""CPU tests of the fused LM head + loss (kgs/ops/linear_xent.py): the float64 reference and the
argument checks; the kernels are tested in test_linear_xent_gpu.py."""
import pytest
import torch

from kgs.models.decoder import DecoderLM
from kgs.ops import linear_xent as lx


def _case(t=128, v=256, k=64):
    g = torch.Generator().manual_seed(t + v + k)
    h, w = torch.randn(t, k, generator=g).bfloat16(), torch.randn(v, k, generator=g).bfloat16()
    tg = torch.randint(0, v, (t,), generator=g)
    tg[:4] = torch.tensor([0, v - 1, -100, v])
    return h, w, tg


def test_ref_is_torchs_cross_entropy_on_the_float64_logits():
    h, w, tg = _case()
    z = h.double() @ w.double().T
    loss, lse = lx.ref_linear_cross_entropy(h, w, tg)
    want = torch.nn.functional.cross_entropy(z, torch.where((tg >= 0) & (tg < 256), tg, -100), reduction="none")
    assert loss.dtype == torch.float64 and torch.allclose(loss, want, rtol=0, atol=1e-12)
    assert loss[2] == 0 and loss[3] == 0 and torch.allclose(lse, torch.logsumexp(z, 1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("fn", [lx.linear_cross_entropy, lx.linear_cross_entropy_rows,
                                lambda h, w, tg: lx.linear_cross_entropy_dlogits(h, w, tg, tg.float(), tg.float())])
def test_argument_checks(fn):
    h, w, tg = _case()
    with pytest.raises(ValueError, match="multiples of 128"):
        fn(h, w[:200], tg)
    with pytest.raises(ValueError, match="row stride"):
        fn(torch.zeros(128, 68, dtype=torch.bfloat16)[:, :64], w, tg)
    with pytest.raises(TypeError, match="h must be a bf16"):
        fn(h.float(), w, tg)
    with pytest.raises(TypeError, match="target must be a int64"):
        fn(h, w, tg.int())
    with pytest.raises(ValueError, match="on a GPU"):  # every check before the device's passed
        fn(h, w, tg)


def test_decoder_option():
    kw = dict(vocab=256, dim=128, layers=1, heads=1, kv_heads=1, inter=64, backend="torch")
    assert DecoderLM(**kw).fused_loss is False
    with pytest.raises(ValueError, match="fused_loss takes backend='kgs'"):
        DecoderLM(**kw, fused_loss=True)
    with pytest.raises(ValueError, match="multiple of 128"):
        DecoderLM(vocab=200, dim=512, layers=0, heads=4, kv_heads=4, inter=64, backend="kgs", fused_loss=True)
