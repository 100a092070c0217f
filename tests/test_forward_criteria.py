"""CPU proof that the criteria of tests/test_forward_block_gpu.py and
tests/test_forward_decode_gpu.py discriminate. Each ``check_*`` of tests/forward_refs.py
is applied here, with no GPU, to two stand-ins for a kernel's output: the same formula
evaluated by plain torch in fp32 and rounded once to bf16 (must be accepted), and that
evaluation with one fault planted (must be rejected). The wrappers' argument checks that
keep the RoPE kernel inside its tables are tested here too: they raise before a device is
looked at."""
import pytest
import torch

import forward_refs as R

CPU = "cpu"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).bfloat16()


def _weight(g, cols):
    return (1 + 0.1 * torch.randn(cols, generator=g)).bfloat16()


def _rejects(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def _tables(rows, hd, theta):
    from kgs.ops.transformer import rope_tables

    return rope_tables(rows, hd, theta, CPU)


# ----------------------------------------------------------------------------
# add_rmsnorm

def _small_rows(g, rows=5, cols=1536):
    scale = torch.tensor([1.0, 1e-3, 0.0, 1e-3, 10.0])[:, None]
    return (torch.randn(rows, cols, generator=g) * scale).bfloat16()


def test_dropped_eps_is_rejected_on_small_rows_and_invisible_on_unit_rows():
    g = _gen(0)
    x, d, w = _small_rows(g), _small_rows(g), _weight(g, 1536)
    for eps in (1e-5, 1e-6, 1e-2):
        res, y = R.baseline(R.ref_add_rmsnorm, x, d, w, eps)
        R.check_add_rmsnorm(res, y, x, d, w, eps)
        _rejects(R.check_add_rmsnorm, *R.baseline(R.ref_add_rmsnorm, x, d, w, 0.0), x, d, w, eps)
        _rejects(R.check_add_rmsnorm, *R.baseline(R.ref_add_rmsnorm, x, d, w, 1e-4), x, d, w, eps)
    # why the small rows are needed: at unit scale the same fault passes
    xu, du = _randn(g, 5, 1536), _randn(g, 5, 1536)
    R.check_add_rmsnorm(*R.baseline(R.ref_add_rmsnorm, xu, du, w, 0.0), xu, du, w, 1e-5)


def test_swapped_weight_chunks_and_a_wrong_residual_are_rejected():
    g = _gen(1)
    rows, cols = 5, 8192
    x = torch.randn(rows, cols, generator=g)
    x[2] *= (2.0 ** torch.arange(16)).repeat_interleave(512)
    x = x.bfloat16()
    d = _randn(g, rows, cols)
    w = ((1 + torch.arange(16) / 16.0).repeat_interleave(512) * (1 + 0.01 * torch.randn(cols, generator=g))).bfloat16()
    res, y = R.baseline(R.ref_add_rmsnorm, x, d, w, 1e-5)
    R.check_add_rmsnorm(res, y, x, d, w, 1e-5)
    ws = w.clone()
    ws[512:1024], ws[1024:1536] = w[1024:1536], w[512:1024]
    _rejects(R.check_add_rmsnorm, *R.baseline(R.ref_add_rmsnorm, x, d, ws, 1e-5), x, d, w, 1e-5)
    # a residual summed in bf16 steps (x + d rounded twice) is not the bits of bf16(x + d)
    bad = res.clone()
    bad[0, 0] = (bad[0, 0].float() * (1 + 2.0 ** -7)).bfloat16()
    _rejects(R.check_add_rmsnorm, bad, y, x, d, w, 1e-5)


# ----------------------------------------------------------------------------
# e4m3 rows

def _fp8_kernel(y32, cols_for_amax=None):
    """What an fp32 kernel emits for rows y32: (codes, scales); the planted fault takes the
    row maximum over the first ``cols_for_amax`` columns only."""
    ys = R.ref_row_scale(y32[:, :cols_for_amax] if cols_for_amax else y32).float()
    return R.ref_quantize_rows(y32, ys), ys


def test_fp8_norm_criteria_accept_fp32_and_reject_a_partial_amax():
    g = _gen(2)
    shares = []
    for cols in (512, 4096, 8192):
        x, d, w = _randn(g, 130, cols), _randn(g, 130, cols), _weight(g, cols)
        x[1], d[1] = 0, 0
        _, y64 = R.ref_add_rmsnorm(x, d, w, 1e-5)
        _, y32 = R.ref_add_rmsnorm(x, d, w, 1e-5, dtype=torch.float32)
        y8, ys = _fp8_kernel(y32)
        shares.append(R.check_codes_near(y8, ys, y64, f"fp32 norm -> e4m3 [{cols}]"))
        err = ((ys.double() - R.ref_row_scale(y64)).abs() / R.fp32_ulp(R.ref_row_scale(y64))).max().item()
        print(f"fp32 torch scale error at {cols}: {err:.3f} ulp")
        # the one-ulp bound on the scale is beyond the row maximum of an fp32 y, and within reach of
        # what the kernel does: the exact fp32 maximum of |x w| times a root taken in double (its
        # eps the fp32 one), divided by 448 and rounded once; the codes with it meet their criterion
        res, _ = R.ref_add_rmsnorm(x, d, w)
        root = torch.rsqrt(res.double().pow(2).mean(-1) + float(torch.tensor(1e-5, dtype=torch.float32)))
        exact = (((res.float() * w.float()).abs().amax(dim=1).double() * root).clamp_min(1e-12) / R.E4M3_MAX).float()
        R.check_row_scale(exact, y64, f"exact maximum, double root [{cols}]")
        R.check_codes_near(R.ref_quantize_rows(y32, exact), exact, y64, f"fp32 codes on that scale [{cols}]")
        if cols > 512:
            b8, bs = _fp8_kernel(y32, 512)
            _rejects(R.check_row_scale, bs, y64, "partial amax")
    # the share the GPU test demands is one the fp32 evaluation reaches
    assert min(shares) >= R.FP8_EQUAL_SHARE, shares


def test_quantize_rows_criteria_accept_the_quantiser_and_reject_faults():
    g = _gen(3)
    x = _randn(g, 130, 2048, scale=3.0)
    x[1] = 0
    x[3] = 0
    x[3, 2045] = 2.5
    y8, ys = _fp8_kernel(x.float())
    R.check_row_scale(ys, x, "quantiser")
    R.check_codes_bitwise(y8, ys, x, "quantiser")
    assert int(y8[1].count_nonzero()) == 0 and int(y8[3].count_nonzero()) == 1
    b8, bs = _fp8_kernel(x.float(), 512)
    _rejects(R.check_row_scale, bs, x, "partial amax")
    trunc = (x.float() / ys[:, None]).clamp(-448, 448)
    trunc = (trunc.abs().floor() * trunc.sign()).to(R.FP8).view(torch.uint8)  # round toward zero
    _rejects(R.check_codes_bitwise, trunc, ys, x, "truncating quantiser")


# ----------------------------------------------------------------------------
# SwiGLU

def _gate_up(g, rows, inter):
    gate = torch.where(torch.rand(rows, inter, generator=g) < 0.5, 2 * torch.randn(rows, inter, generator=g),
                       200 * torch.rand(rows, inter, generator=g) - 100)
    gate[:, :5] = torch.tensor([0.0, 88.0, -88.0, 100.0, -100.0])
    return torch.cat((gate, torch.randn(rows, inter, generator=g)), dim=1).bfloat16()


def test_silu_criterion_accepts_fp32_and_rejects_a_zero_tail_chunk():
    g = _gen(4)
    for inter in (8, 2056):
        gu = _gate_up(g, 5, inter)
        out = R.baseline(R.ref_silu_mul, gu)
        R.check_silu_mul(out, gu)
        ys = R.ref_row_scale(out.float()).float()
        R.check_codes_bitwise(R.ref_quantize_rows(out, ys), ys, out, "silu e4m3")
        bad = out.clone()
        bad[:, -8:] = 0  # chunk 256 of 257: the one the c < nch guard owns
        _rejects(R.check_silu_mul, bad, gu)
        _rejects(R.check_codes_bitwise, R.ref_quantize_rows(bad, ys), ys, out, "silu e4m3 zero tail")
    # a kernel that lets exp overflow to NaN (inf / inf) instead of 0 is rejected: outputs must be finite
    nan = out.clone()
    nan[0, 4] = float("nan")
    _rejects(R.check_silu_mul, nan, gu)


# ----------------------------------------------------------------------------
# RoPE

@pytest.mark.parametrize("hd,theta", [(128, 1e4), (64, 5e5)])
def test_rope_criterion_accepts_fp32_and_rejects_ignored_positions(hd, theta):
    g = _gen(5)
    tokens, heads = 37, 5
    cos, sin = _tables(8192, hd, theta)
    pos = torch.randint(0, 8192, (tokens,), generator=g).int()
    pos[:4] = torch.tensor([0, 1, 8191, 8191]).int()
    qkv = _randn(g, tokens, (heads + 2) * hd)

    def kernel(p):
        got = qkv.clone()
        got[:, :heads * hd] = R.baseline(lambda *a, **k: R.ref_rope(*a, **k)[0], qkv, cos, sin, heads, hd, p)
        return got

    R.check_rope(kernel(pos), qkv, cos, sin, heads, hd, pos)
    _rejects(R.check_rope, kernel(R.default_positions(tokens, tokens, CPU)), qkv, cos, sin, heads, hd, pos)
    spilled = kernel(pos)
    spilled[3, heads * hd] = 0  # a write past the rotated heads
    _rejects(R.check_rope, spilled, qkv, cos, sin, heads, hd, pos)


def test_rope_wrapper_refuses_what_would_read_past_its_tables():
    """Nothing is launched: every call raises on its arguments alone."""
    from kgs.ops.transformer import rope_qkv_

    qkv = torch.zeros(6, 4 * 64, dtype=torch.bfloat16)
    cos, sin = _tables(4, 64, 1e4)
    with pytest.raises(ValueError, match="at least seq rows"):
        rope_qkv_(qkv, cos, sin, 2, 64, 6)
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros(7, dtype=torch.int32),
                torch.zeros(6, 1, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="one entry per row"):
            rope_qkv_(qkv, cos, sin, 2, 64, 6, positions=bad)
    with pytest.raises(ValueError, match="qkv's device"):
        rope_qkv_(qkv, cos, sin, 2, 64, 6, positions=torch.zeros(6, dtype=torch.int32, device="meta"))


# ----------------------------------------------------------------------------
# split-K reduce + add + rmsnorm

def test_splitk_criterion_accepts_slice_order_and_rejects_the_reverse():
    g = _gen(6)
    rows, cols, nslice = 5, 4096, 14
    p = R.cancelling_partials(nslice, rows, cols, g, CPU)
    x, w = _randn(g, rows, cols), _weight(g, cols)
    res, y = R.baseline(R.ref_splitk_add_rmsnorm, p, x, w, 1e-5)
    R.check_splitk_add_rmsnorm(res, y, p, x, w, 1e-5)
    _rejects(R.check_splitk_add_rmsnorm, *R.baseline(R.ref_splitk_add_rmsnorm, p.flip(0), x, w, 1e-5), p, x, w, 1e-5)
    # plain randn partials, as most of the GPU cases use: the reverse order still shows in some element
    q = torch.randn(nslice, 130, 2048, generator=g)
    x2, w2 = _randn(g, 130, 2048), _weight(g, 2048)
    _rejects(R.check_splitk_add_rmsnorm, *R.baseline(R.ref_splitk_add_rmsnorm, q.flip(0), x2, w2, 1e-5), q, x2, w2,
             1e-5)
    small = p * 1e-3
    _rejects(R.check_splitk_add_rmsnorm, *R.baseline(R.ref_splitk_add_rmsnorm, small, x * 1e-3, w, 0.0), small,
             x * 1e-3, w, 1e-2)


def test_argmax_reference_is_torch_argmax_on_the_edges():
    x = torch.full((4, 16), -1.0).bfloat16()
    x[0] = float("-inf")
    x[1] = float("nan")
    x[2, 5], x[2, 9] = -0.0, 0.0
    x[3, 5], x[3, 9] = 0.0, -0.0
    assert R.ref_argmax(x).tolist() == [0, 0, 5, 5]


# ----------------------------------------------------------------------------
# paged decode attention

HEADS, HKV = 8, 2


def _decode_tables():
    return _tables(2048, 128, 5e5)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_decode_criterion_rejects_a_skipped_page_and_keys_past_the_context(kv_dtype):
    """The value scales of test_paged_decode_small_and_large_grids at ctx 1056, where either
    fault moves the output by about 2e-2 absolute (printed), the bound of that test."""
    cos, sin = _decode_tables()
    c, q, cache = R.decode_turn(R.decode_case(HEADS, HKV, kv_dtype, [1056, 33], CPU, 0, cos, sin, kv_scale=0.7))
    ref = R.ref_paged_decode(q, cache, c.bt, c.ctx_t, HEADS, HKV)
    base = R.baseline(R.ref_paged_decode, q, cache, c.bt, c.ctx_t, HEADS, HKV)
    R.check_decode_against_baseline(base, base, ref, HEADS, "fp32 decode")
    skipped = c.bt.clone()
    skipped[0, 17:-1] = c.bt[0, 18:]  # page 17 never read
    bad = R.baseline(R.ref_paged_decode, q, cache, skipped, c.ctx_t - torch.tensor([32, 0], dtype=torch.int32), HEADS,
                     HKV)
    print("skipped page moves the output by", (bad.double() - ref).abs().max().item())
    _rejects(R.check_decode_against_baseline, bad, base, ref, HEADS, "skipped page")
    over = R.baseline(R.ref_paged_decode, q, cache, c.bt, c.ctx_t + 8, HEADS, HKV)
    print("8 keys past ctx move the output by", (over.double() - ref).abs().max().item())
    _rejects(R.check_decode_against_baseline, over, base, ref, HEADS, "8 keys past ctx")


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_needle_criterion_accepts_fp32_everywhere_and_rejects_a_swapped_page(kv_dtype):
    cos, sin = _decode_tables()
    ctxs, pps = [1, 32, 33, 300], 3
    places = [R.needle_positions(ctx, pps) for ctx in ctxs]
    assert places[0] == [0] and places[2] == [0, 31, 32]
    assert places[3] == [0, 31, 64, 95, 96, 127, 160, 191, 192, 223, 256, 287, 288, 299]
    base_case = R.decode_case(HEADS, HKV, kv_dtype, ctxs, CPU, 1, cos, sin, group_q=True)
    for turn in range(max(len(p) for p in places)):
        needles = [p[turn % len(p)] for p in places]
        c, q, cache = R.decode_turn(base_case, needles)
        base = R.baseline(R.ref_paged_decode, q, cache, c.bt, c.ctx_t, HEADS, HKV)
        R.check_needles(base, q, cache, c, needles, f"fp32 decode, turn {turn}")
    # the needle in the last valid table entry; a kernel that reads its neighbour instead loses it
    swapped = c.bt.clone()
    last = (ctxs[3] - 1) // R.PAGE
    assert needles[3] // R.PAGE == last
    swapped[3, last], swapped[3, last + 1] = c.bt[3, last + 1], c.bt[3, last]
    bad = R.baseline(R.ref_paged_decode, q, cache, swapped, c.ctx_t, HEADS, HKV)
    _rejects(R.check_needles, bad, q, cache, c, needles, "swapped page")


def test_a_needle_outside_the_context_changes_the_reference_only_if_it_is_read():
    """The bitwise test of the GPU file in miniature: planted past ctx the needles leave the
    fp32 evaluation bit-identical; read (ctx + 8 keys) they take the output over."""
    cos, sin = _decode_tables()
    ctxs = [1, 32, 33, 300]
    base_case = R.decode_case(HEADS, HKV, "bf16", ctxs, CPU, 2, cos, sin, group_q=True)
    for ctx in ctxs:
        keys = R.outside_positions(ctx, base_case.width)
        assert keys[0] == ctx and keys[1] == ctx + 1 and keys[-1] == base_case.width * R.PAGE - 1
    c, q, cache = R.decode_turn(base_case)
    clean = R.baseline(R.ref_paged_decode, q, cache, c.bt, c.ctx_t, HEADS, HKV)
    c, q2, planted = R.decode_turn(base_case, outside=True)
    assert R.same_bits(q, q2) and not R.same_bits(planted, cache)
    assert R.same_bits(R.baseline(R.ref_paged_decode, q, planted, c.bt, c.ctx_t, HEADS, HKV), clean)
    assert not R.same_bits(R.baseline(R.ref_paged_decode, q, planted, c.bt, c.ctx_t + 8, HEADS, HKV), clean)
