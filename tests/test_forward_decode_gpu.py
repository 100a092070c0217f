"""GPU tests of the paged decode attention (native/kernels/decode.hip: paged_decode,
paged_reduce) in which every key is accounted for, through both entries
(paged_decode_attention, rope_paged_decode_attention), bf16 and e4m3 caches, scattered
pages and a block table wider than any context needs.

* A needle inside the context -- one key c q / |q| whose float64 softmax weight is at least
  1 - 2^-12 -- must bring back its own V row within a bf16 rounding, wherever it sits: key 0,
  key ctx - 1, the first and last slot of the first and last page of every split, the last
  valid table entry.
* The same needle past the context (key ctx, ctx + 1, the rest of the last page, every table
  entry beyond) must leave the output bit-identical.
* Random inputs per element against float64, within twice the error of the fp32 torch
  evaluation rounded to bf16.

The criteria are tests/forward_refs.py's; tests/test_forward_criteria.py shows on the CPU
that they reject a skipped page, keys read past ctx and a swapped page.

Grids: (32 heads, 8 KV heads) x 6 sequences is the pipelined kernel with the paged_reduce
merge, (16, 1) x 6 the pipelined kernel with the in-launch merge (``pipe=False``: the
one-page-at-a-time kernel with the serial in-launch merge), 80 sequences x 8 KV heads x 4
splits the large-grid kernel. The fused RoPE entry takes at most 6 q heads per KV head, so
it runs (32, 8) only."""
import functools

import pytest
import torch

import forward_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL = (1, 32, 33, 64, 97, 300)  # one key; ending at slot 31 (32, 64) and slot 0 (33, 97) of a page; ten pages
LARGE = (300,) + (1, 5, 32, 33, 40) * 16  # 81 sequences: 648 (sequence, KV head) groups x 4 splits > 1024 waves
EACH = (1, 33, 300, 1056)
GRIDS = [(32, 8, "plain"), (32, 8, "rope"), (16, 1, "plain")]


@functools.lru_cache(maxsize=None)
def _tables():
    from kgs.ops.transformer import rope_tables

    return rope_tables(2048, R.HD, 5e5, DEV)


@functools.lru_cache(maxsize=None)
def _base(heads, hkv, kv_dtype, ctxs, group_q, kv_scale=1.0):
    return R.decode_case(heads, hkv, kv_dtype, ctxs, DEV, len(ctxs) + heads, *_tables(), group_q=group_q,
                         kv_scale=kv_scale)


def _run(entry, c, q, cache, pps, pipe=None):
    """The kernel's output for the state (q, cache). The fused RoPE entry gets the
    pre-rotation rows as two exact half partials and a cache whose new-token slots are
    cleared: it rotates q itself and stores the new K / V before it attends."""
    from kgs.ops.decode import paged_decode_attention, rope_paged_decode_attention

    if entry == "plain":
        out = paged_decode_attention(q, cache, c.bt, c.ctx_t, c.heads, c.hkv, pages_per_split=pps, pipe=pipe)
    else:
        mine = cache.clone()
        zeros = torch.zeros(c.b, c.hkv, R.HD, device=DEV)
        R.write_tokens(mine, c.slots.long() // R.PAGE, c.slots.long() % R.PAGE, zeros, zeros)
        half = 0.5 * c.qkv_pre.float()
        out = rope_paged_decode_attention(torch.stack((half, half)).contiguous(), c.cos, c.sin, c.pos, c.slots, mine,
                                          c.bt, c.ctx_t, c.heads, c.hkv, pages_per_split=pps, pipe=pipe)
    torch.cuda.synchronize()
    return out


def _needles_inside(heads, hkv, entry, kv_dtype, ctxs, pps, pipe=None):
    base = _base(heads, hkv, kv_dtype, ctxs, True)
    assert (base.width + pps - 1) // pps == {13: 1, 7: 2, 4: 4, 3: 5}[pps]
    places = [R.needle_positions(ctx, pps) for ctx in ctxs]
    for turn in range(max(len(p) for p in places)):
        needles = [p[turn % len(p)] for p in places]
        c, q, cache = R.decode_turn(base, needles)
        out = _run(entry, c, q, cache, pps, pipe)
        R.check_needles(out, q, cache, c, needles, f"{entry} {heads}/{hkv} {kv_dtype} pps {pps} turn {turn}")


@pytest.mark.parametrize("pps", [13, 7, 3])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("heads,hkv,entry", GRIDS)
def test_a_needle_inside_the_context_brings_back_its_value(heads, hkv, entry, kv_dtype, pps):
    """One, two and five splits of a 13-entry table (the ten-page context fills four of the five)."""
    _needles_inside(heads, hkv, entry, kv_dtype, SMALL, pps)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_a_needle_inside_the_context_without_the_page_pipeline(kv_dtype):
    _needles_inside(16, 1, "plain", kv_dtype, SMALL, 3, pipe=False)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("entry", ["plain", "rope"])
def test_a_needle_inside_the_context_on_the_large_grid(entry, kv_dtype):
    assert len(LARGE) * 8 * 4 > 1024
    _needles_inside(32, 8, entry, kv_dtype, LARGE, 4)


def _needles_outside(heads, hkv, entry, kv_dtype, ctxs, pps, pipe=None):
    base = _base(heads, hkv, kv_dtype, ctxs, True)
    c, q, cache = R.decode_turn(base)
    clean = _run(entry, c, q, cache, pps, pipe)
    c2, q2, planted = R.decode_turn(base, outside=True)
    assert R.same_bits(q, q2) and not R.same_bits(planted, cache)
    assert int(c2.bt.min()) >= 0 and int(c2.bt.max()) < planted.shape[0]  # every table entry a valid page
    assert R.same_bits(_run(entry, c2, q2, planted, pps, pipe), clean)
    # and the clean output is right: per element against float64, twice the fp32 baseline's error
    ref = R.ref_paged_decode(q, cache, c.bt, c.ctx_t, heads, hkv)
    basel = R.baseline(R.ref_paged_decode, q, cache, c.bt, c.ctx_t, heads, hkv)
    R.check_decode_against_baseline(clean, basel, ref, heads, f"{entry} {heads}/{hkv} {kv_dtype} pps {pps}")


@pytest.mark.parametrize("pps", [13, 3])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("heads,hkv,entry", GRIDS)
def test_a_needle_outside_the_context_changes_no_bit(heads, hkv, entry, kv_dtype, pps):
    _needles_outside(heads, hkv, entry, kv_dtype, SMALL, pps)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("entry", ["plain", "rope"])
def test_a_needle_outside_the_context_on_the_large_grid(entry, kv_dtype):
    _needles_outside(32, 8, entry, kv_dtype, LARGE, 4)


def test_a_needle_outside_the_context_without_the_page_pipeline():
    _needles_outside(16, 1, "plain", "bf16", SMALL, 3, pipe=False)


@functools.lru_cache(maxsize=None)
def _each_case(heads, hkv, kv_dtype):
    """ctx 1, 33, 300 and 1056 with the value scales of test_paged_decode_small_and_large_grids
    (q ~ N(0, 1), K and V ~ 0.7 N(0, 1)), the float64 reference and the fp32 baseline."""
    c, q, cache = R.decode_turn(_base(heads, hkv, kv_dtype, EACH, False, 0.7))
    ref = R.ref_paged_decode(q, cache, c.bt, c.ctx_t, heads, hkv)
    return c, q, cache, ref, R.baseline(R.ref_paged_decode, q, cache, c.bt, c.ctx_t, heads, hkv)


@pytest.mark.parametrize("pps", [36, 12, 4])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("heads,hkv,entry", GRIDS)
def test_every_element_against_float64_within_twice_the_fp32_baselines_error(heads, hkv, entry, kv_dtype, pps):
    """One, three and nine splits of a 36-entry table."""
    c, q, cache, ref, basel = _each_case(heads, hkv, kv_dtype)
    assert c.width == 36
    out = _run(entry, c, q, cache, pps)
    R.check_decode_against_baseline(out, basel, ref, heads, f"{entry} {heads}/{hkv} {kv_dtype} pps {pps}")


def test_fused_rope_entry_refuses_wide_head_groups():
    c, q, cache = R.decode_turn(_base(16, 1, "bf16", SMALL, True))
    with pytest.raises(ValueError):
        _run("rope", c, q, cache, 13)
