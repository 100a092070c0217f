"""GPU tests of the forward decoder-block glue (native/kernels/transformer.hip) at the
standard of the training kernels' tests: every element against a float64 reference
on the same bf16 inputs (tests/forward_refs.py: ``|out - ref64| <= 2^-7 |ref64| +
atol``, the atol derived at each ``check_*``), every template instantiation launched,
rows 1 (one wave), 5 (a partly filled last 4-wave block) and 130 (more than one
block, more than 128), and every strided operand a view into a poisoned buffer.
tests/test_forward_criteria.py shows on the CPU that these criteria reject the
mistakes they are here for."""
import functools

import pytest
import torch

import forward_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 5, 130)
FP8_COLS = tuple(512 * n for n in (1, 2, 4, 6, 8, 10, 12, 16))


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, device=DEV, generator=g)).bfloat16()


def _weight(g, cols):
    return (1 + 0.1 * torch.randn(cols, device=DEV, generator=g)).bfloat16()


def _lib():
    from kgs.ops import _lib

    return _lib


def _stream():
    return _lib().stream_handle(torch.device(DEV))


def _padded_vector(n, dtype=torch.float32):
    """[n] inside a poisoned vector: (view, buffer)."""
    buf = torch.full((n + 8,), R.POISON, dtype=dtype, device=DEV)
    return buf[4:4 + n], buf


def _vector_intact(buf, n):
    return bool((buf[:4] == R.POISON).all() and (buf[4 + n:] == R.POISON).all())


# ----------------------------------------------------------------------------
# add_rmsnorm<NC>

def _run_add_rmsnorm(x, d, w, eps):
    """x and d as equal-stride views into poisoned buffers, out strided: checks everything."""
    from kgs.ops.transformer import add_rmsnorm

    rows, cols = x.shape
    xv, xbuf = R.wide(x, pad=64)
    dv, dbuf = R.wide(d, pad=64) if d is not None else (None, None)
    ov, obuf = R.wide(torch.zeros_like(x), pad=72)
    got = add_rmsnorm(xv, dv, w, eps, out=ov)
    torch.cuda.synchronize()
    assert got.data_ptr() == ov.data_ptr()
    R.check_add_rmsnorm(xv, ov, x, d, w, eps, f"add_rmsnorm[{rows}x{cols}]")
    assert R.poison_intact(xbuf, rows, cols) and R.poison_intact(obuf, rows, cols)
    if d is not None:
        assert R.same_bits(dv, d) and R.poison_intact(dbuf, rows, cols)


@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("cols", [512 * n for n in range(1, 17)])
def test_add_rmsnorm_every_width_against_float64(cols, with_d):
    g = _gen(cols + with_d)
    w = _weight(g, cols)
    for rows in ROWS:
        _run_add_rmsnorm(_randn(g, rows, cols), _randn(g, rows, cols) if with_d else None, w, 1e-5)


@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("eps", [1e-5, 1e-6, 1e-2])
def test_add_rmsnorm_eps_decides_small_rows(eps, with_d):
    """Rows at 1e-3 (mean(x^2) = 1e-6 < eps: eps carries the result), an all-zero row
    (y = 0 exactly, never NaN), unit rows beside them."""
    g = _gen(7)
    rows, cols = 5, 1536
    scale = torch.tensor([1.0, 1e-3, 0.0, 1e-3, 10.0], device=DEV)[:, None]
    x = (torch.randn(rows, cols, device=DEV, generator=g) * scale).bfloat16()
    d = (torch.randn(rows, cols, device=DEV, generator=g) * scale).bfloat16() if with_d else None
    s = x.float() if d is None else x.float() + d.float()
    assert s[1].pow(2).mean().item() < 1e-5 and s[2].abs().max().item() == 0
    _run_add_rmsnorm(x, d, _weight(g, cols), eps)


def test_add_rmsnorm_chunk_to_weight_pairing():
    """Row 2's 512-column chunks are scaled 1, 2, 4, ... and the weight's chunks 1, 17/16,
    18/16, ...: pairing a chunk with another chunk's weight moves y by at least 1/32."""
    g = _gen(11)
    rows, cols = 5, 8192
    x = torch.randn(rows, cols, device=DEV, generator=g)
    x[2] *= (2.0 ** torch.arange(16, device=DEV)).repeat_interleave(512)
    w = ((1 + torch.arange(16, device=DEV) / 16.0).repeat_interleave(512) *
         (1 + 0.01 * torch.randn(cols, device=DEV, generator=g))).bfloat16()
    _run_add_rmsnorm(x.bfloat16(), _randn(g, rows, cols), w, 1e-5)


def test_add_rmsnorm_separate_residual_output_leaves_x_alone():
    from kgs.ops.transformer import _add_rmsnorm_out_of_place

    g = _gen(13)
    rows, cols = 130, 2560
    x, d, w = _randn(g, rows, cols), _randn(g, rows, cols), _weight(g, cols)
    x0, d0 = x.clone(), d.clone()
    res, y = _add_rmsnorm_out_of_place(x, d, w, 1e-5)
    torch.cuda.synchronize()
    assert R.same_bits(x, x0) and R.same_bits(d, d0) and res.data_ptr() != x.data_ptr()
    R.check_add_rmsnorm(res, y, x0, d0, w, 1e-5, "add_rmsnorm xo != x")


# ----------------------------------------------------------------------------
# add_rmsnorm<NC, true> and quant_rows<NC>

def _special_rows(x):
    """From 5 rows up: row 1 all zero, row 3 a single non-zero element."""
    if x.shape[0] >= 5:
        x[1] = 0
        keep = x[3, 7].clone()
        x[3] = 0
        x[3, x.shape[1] - 3] = keep if float(keep) != 0 else 1.0
    return x


@functools.lru_cache(maxsize=None)
def _norm_fp8_case(rows, cols, with_d):
    """One fused-norm launch through the raw entry (y8 strided in a poisoned buffer, ys in a
    padded vector) and its float64 reference; shared by the tests, never modified."""
    g = _gen(3 * cols + rows + with_d)
    x = _special_rows(_randn(g, rows, cols))
    d = None
    if with_d:
        d = _randn(g, rows, cols)
        if rows >= 5:
            d[1] = 0
            d[3] = 0
    w = _weight(g, cols)
    xv, xbuf = R.wide(x, pad=64)
    dv = R.wide(d, pad=64)[0] if with_d else None
    y8, ybuf = R.wide_bytes(rows, cols, DEV)
    ys, sbuf = _padded_vector(rows)
    rc = _lib().lib().kgs_add_rmsnorm_fp8(xv.data_ptr(), 0 if d is None else dv.data_ptr(),
                                         0 if d is None else xv.data_ptr(), w.data_ptr(), y8.data_ptr(), ys.data_ptr(),
                                         rows, cols, xv.stride(0), y8.stride(0), 1e-5, _stream())
    torch.cuda.synchronize()
    res, y64 = R.ref_add_rmsnorm(x, d, w, 1e-5)
    return {"rc": rc, "x": x, "xv": xv, "xbuf": xbuf, "y8": y8, "ybuf": ybuf, "ys": ys, "sbuf": sbuf, "res": res,
            "y64": y64}


@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("cols", FP8_COLS)
def test_add_rmsnorm_fp8_codes_against_float64(cols, with_d):
    """Residual: bitwise. Codes: within one e4m3 code of the float64 y quantised with the
    kernel's scale, at least 99 % equal (fp32 torch reaches 99.99 %, see
    test_forward_criteria.py). Pad bytes beside y8 and ys untouched."""
    for rows in ROWS:
        c = _norm_fp8_case(rows, cols, with_d)
        assert c["rc"] == 0
        assert R.same_bits(c["xv"], c["res"]) and R.poison_intact(c["xbuf"], rows, cols)
        R.check_codes_near(c["y8"], c["ys"], c["y64"], f"add_rmsnorm_fp8[{rows}x{cols}]")
        assert R.poison_intact(c["ybuf"], rows, cols, off=16, fill=R.POISON_BYTE)
        assert _vector_intact(c["sbuf"], rows)
        if rows >= 5:  # the all-zero row: scale 1e-12 / 448, codes 0
            assert int(c["y8"][1].count_nonzero()) == 0
            assert int(c["y8"][3].count_nonzero()) == 1


@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("cols", FP8_COLS)
def test_add_rmsnorm_fp8_scales_within_one_ulp_of_float64(cols, with_d):
    """ys within one fp32 ulp of max(amax, 1e-12) / 448 of the float64 y. An fp32 evaluation
    of y (sum of squares, rsqrt, two products) is up to 2.3 ulp off before the division --
    fp32 torch as much as the kernel's own y -- so the kernel takes the scale from the exact
    fp32 maximum of |x w| and a root of the sum of squares in double."""
    for rows in ROWS:
        c = _norm_fp8_case(rows, cols, with_d)
        R.check_row_scale(c["ys"], c["y64"], f"add_rmsnorm_fp8[{rows}x{cols}] ys")


@pytest.mark.parametrize("cols", FP8_COLS)
def test_quantize_rows_fp8_is_the_reference_quantiser(cols):
    """Scales within one fp32 ulp of max(amax, 1e-12) / 448; codes bitwise the reference
    quantiser's with the kernel's own scales; strided x and y8, pads untouched."""
    g = _gen(cols)
    for rows in ROWS:
        x = _special_rows(_randn(g, rows, cols, scale=3.0))
        xv, xbuf = R.wide(x, pad=64)
        y8, ybuf = R.wide_bytes(rows, cols, DEV)
        ys, sbuf = _padded_vector(rows)
        rc = _lib().lib().kgs_quant_rows_fp8(xv.data_ptr(), y8.data_ptr(), ys.data_ptr(), rows, cols, xv.stride(0),
                                            y8.stride(0), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        R.check_row_scale(ys, x, f"quantize_rows_fp8[{rows}x{cols}] ys")
        R.check_codes_bitwise(y8, ys, x, f"quantize_rows_fp8[{rows}x{cols}]")
        assert R.same_bits(xv, x) and R.poison_intact(xbuf, rows, cols)
        assert R.poison_intact(ybuf, rows, cols, off=16, fill=R.POISON_BYTE) and _vector_intact(sbuf, rows)
        if rows >= 5:
            assert int(y8[1].count_nonzero()) == 0 and int(y8[3].count_nonzero()) == 1


def test_quantize_rows_fp8_wrapper_matches_the_raw_entry():
    from kgs.ops.transformer import quantize_rows_fp8

    x = _randn(_gen(5), 5, 1024, scale=3.0)
    y8, ys = quantize_rows_fp8(x)
    torch.cuda.synchronize()
    R.check_row_scale(ys, x, "quantize_rows_fp8 wrapper ys")
    R.check_codes_bitwise(y8, ys, x, "quantize_rows_fp8 wrapper")


def test_fp8_rows_refuse_a_width_without_an_instantiation():
    from kgs.ops import KernelError
    from kgs.ops.transformer import add_rmsnorm_fp8, quantize_rows_fp8

    g = _gen(1)
    x, w = _randn(g, 5, 1536), _weight(g, 1536)
    with pytest.raises(KernelError):
        add_rmsnorm_fp8(x, None, w)
    with pytest.raises(KernelError):
        quantize_rows_fp8(x)


# ----------------------------------------------------------------------------
# silu_mul and silu_mul_q8<CPT>

SILU_INTER = (8, 2040, 2048, 2056, 14336, 32768)
GATES = (0.0, 88.0, -88.0, 100.0, -100.0)


def _gate_up(g, rows, inter):
    """Gates half unit-scale (x2), half uniform in [-100, 100], with 0, +-88, +-100 planted
    at the head of every row and (from 16 columns up) at its tail; up at unit scale."""
    wide_g = 200 * torch.rand(rows, inter, device=DEV, generator=g) - 100
    unit = 2 * torch.randn(rows, inter, device=DEV, generator=g)
    gate = torch.where(torch.rand(rows, inter, device=DEV, generator=g) < 0.5, unit, wide_g).clamp(-100, 100)
    special = torch.tensor(GATES, device=DEV)
    gate[:, :5] = special
    if inter >= 16:
        gate[:, -5:] = special
    up = torch.randn(rows, inter, device=DEV, generator=g)
    return torch.cat((gate, up), dim=1).bfloat16()


def _raw_silu_fp8(guv, rows, inter):
    y8, ybuf = R.wide_bytes(rows, inter, DEV)
    ys, sbuf = _padded_vector(rows)
    rc = _lib().lib().kgs_silu_mul_fp8(guv.data_ptr(), y8.data_ptr(), ys.data_ptr(), rows, inter, guv.stride(0),
                                      y8.stride(0), _stream())
    torch.cuda.synchronize()
    return rc, y8, ybuf, ys, sbuf


@pytest.mark.parametrize("inter", SILU_INTER)
def test_silu_mul_and_its_fp8_form(inter):
    """bf16: per element against float64, strided in and out, poison intact. fp8: the
    scale is max(amax, 1e-12) / 448 of the bf16 result within an ulp and the codes are
    bitwise the reference quantiser's on it (the kernel rounds through bf16 first);
    where quant_rows has the width, bitwise quantize_rows_fp8(silu_mul(gu)) as well."""
    from kgs.ops.transformer import quantize_rows_fp8, silu_mul

    g = _gen(inter)
    for rows in ROWS:
        gu = _gate_up(g, rows, inter)
        guv, gbuf = R.wide(gu, pad=64)
        ov, obuf = R.wide(torch.zeros(rows, inter, dtype=torch.bfloat16, device=DEV), pad=72)
        silu_mul(guv, out=ov)
        rc, y8, ybuf, ys, sbuf = _raw_silu_fp8(guv, rows, inter)
        assert rc == 0
        R.check_silu_mul(ov, gu, f"silu_mul[{rows}x{inter}]")
        assert R.same_bits(guv, gu) and R.poison_intact(gbuf, rows, 2 * inter)
        assert R.poison_intact(obuf, rows, inter)
        out = ov.contiguous()
        R.check_row_scale(ys, out, f"silu_mul_fp8[{rows}x{inter}] ys")
        R.check_codes_bitwise(y8, ys, out, f"silu_mul_fp8[{rows}x{inter}]")
        assert R.poison_intact(ybuf, rows, inter, off=16, fill=R.POISON_BYTE) and _vector_intact(sbuf, rows)
        if inter % 512 == 0 and inter <= 8192:
            q8, qs = quantize_rows_fp8(out)
            assert torch.equal(qs, ys) and R.same_bits(q8, y8)


@pytest.mark.parametrize("cpt", range(1, 17))
def test_silu_mul_fp8_every_chunks_per_thread_count(cpt):
    """inter = 2048 cpt - 8: cpt chunks per thread with the last one ragged (the c < nch guards
    decide). Through the raw entry: the e4m3 row stride must be a multiple of 16, which the
    wrapper's own buffer is not at these widths."""
    from kgs.ops.transformer import silu_mul

    inter = 2048 * cpt - 8
    gu = _gate_up(_gen(cpt), 1, inter)
    out = silu_mul(gu)
    rc, y8, ybuf, ys, sbuf = _raw_silu_fp8(gu, 1, inter)
    assert rc == 0
    R.check_silu_mul(out, gu, f"silu_mul[1x{inter}]")
    R.check_row_scale(ys, out, f"silu_mul_fp8[1x{inter}] ys")
    R.check_codes_bitwise(y8, ys, out, f"silu_mul_fp8[1x{inter}]")
    assert R.poison_intact(ybuf, 1, inter, off=16, fill=R.POISON_BYTE) and _vector_intact(sbuf, 1)


def test_silu_mul_fp8_refuses_rows_wider_than_its_registers():
    from kgs.ops import KernelError
    from kgs.ops.transformer import silu_mul_fp8

    with pytest.raises(KernelError):
        silu_mul_fp8(torch.zeros(1, 2 * 32776, dtype=torch.bfloat16, device=DEV))


# ----------------------------------------------------------------------------
# rope_qkv

TABLE_ROWS = 8192


@functools.lru_cache(maxsize=None)
def _tables(hd, theta):
    from kgs.ops.transformer import rope_tables

    return rope_tables(TABLE_ROWS, hd, theta, DEV)


@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("hd", [128, 64])
def test_rope_scattered_positions_against_float64(hd, theta):
    """37 tokens x 5 rotated heads (37 * 5 * hd / 16 threads: no multiple of 256), a padded
    row stride, positions scattered over the 8192-row table with 0, 1, the last row and
    repeats. The default token % seq result is far away, so ignored positions fail."""
    from kgs.ops.transformer import rope_qkv_

    tokens, heads = 37, 5
    assert (tokens * heads * hd // 16) % 256
    g = _gen(hd)
    cos, sin = _tables(hd, theta)
    pos = torch.randint(0, TABLE_ROWS, (tokens,), device=DEV, generator=g).int()
    pos[:6] = torch.tensor([0, 1, TABLE_ROWS - 1, TABLE_ROWS - 1, 4097, 4097], device=DEV).int()
    qkv = _randn(g, tokens, (heads + 2) * hd)
    qv, qbuf = R.wide(qkv, pad=64)
    rope_qkv_(qv, cos, sin, heads, hd, tokens, positions=pos)
    torch.cuda.synchronize()
    R.check_rope(qv, qkv, cos, sin, heads, hd, pos, f"rope hd {hd} theta {theta:g}")
    assert R.poison_intact(qbuf, tokens, qkv.shape[1])
    other = R.ref_rope(qkv, cos, sin, heads, hd, R.default_positions(tokens, tokens, DEV))[0]
    assert (other - R.ref_rope(qkv, cos, sin, heads, hd, pos)[0]).abs().max().item() > 1.0


@pytest.mark.parametrize("hd", [128, 64])
def test_rope_default_positions_batch_3_seq_40(hd):
    """token % 40 over 120 tokens from a table of exactly 40 rows."""
    from kgs.ops.transformer import rope_qkv_

    batch, seq, heads = 3, 40, 5
    g = _gen(hd + 1)
    cos, sin = (t[:seq].clone() for t in _tables(hd, 5e5))
    qkv = _randn(g, batch * seq, (heads + 2) * hd)
    qv, qbuf = R.wide(qkv, pad=64)
    rope_qkv_(qv, cos, sin, heads, hd, seq)
    torch.cuda.synchronize()
    R.check_rope(qv, qkv, cos, sin, heads, hd, R.default_positions(batch * seq, seq, DEV), f"rope default hd {hd}")
    assert R.poison_intact(qbuf, batch * seq, qkv.shape[1])


# ----------------------------------------------------------------------------
# splitk_add_rmsnorm<NJ, NSL>

def _run_splitk(partials, x, w, eps):
    from kgs.ops.transformer import splitk_add_rmsnorm

    rows, cols = x.shape
    xv, xbuf = R.wide(x, pad=64)
    ov, obuf = R.wide(torch.zeros_like(x), pad=72)
    p0 = partials.clone()
    splitk_add_rmsnorm(partials, xv, w, eps, out=ov)
    torch.cuda.synchronize()
    R.check_splitk_add_rmsnorm(xv, ov, p0, x, w, eps, f"splitk_add_rmsnorm[{partials.shape[0]}x{rows}x{cols}]")
    assert torch.equal(partials, p0)
    assert R.poison_intact(xbuf, rows, cols) and R.poison_intact(obuf, rows, cols)


@pytest.mark.parametrize("nslice", [1, 2, 3, 4, 8, 14])
@pytest.mark.parametrize("cols", [2048, 4096, 6144, 8192])
def test_splitk_add_rmsnorm_every_instantiation_against_float64(cols, nslice):
    g = _gen(cols + nslice)
    w = _weight(g, cols)
    for rows in ROWS:
        _run_splitk(torch.randn(nslice, rows, cols, device=DEV, generator=g), _randn(g, rows, cols), w, 1e-5)


@pytest.mark.parametrize("nslice", [3, 4, 8, 14])
def test_splitk_add_rmsnorm_sums_in_slice_order(nslice):
    """Partials that cancel late (forward_refs.cancelling_partials): hundreds of the bf16
    deltas depend on the order of the fp32 sum, so the reverse order fails the bitwise residual."""
    g = _gen(nslice)
    rows, cols = 5, 4096
    p = R.cancelling_partials(nslice, rows, cols, g, DEV)
    x, w = _randn(g, rows, cols), _weight(g, cols)
    a, b = R.ref_splitk_delta(p), R.ref_splitk_delta(p.flip(0))
    assert int((a.view(torch.int16) != b.view(torch.int16)).sum()) > 100
    _run_splitk(p, x, w, 1e-5)


@pytest.mark.parametrize("eps", [1e-6, 1e-2])
@pytest.mark.parametrize("cols,nslice", [(2048, 3), (6144, 4)])
def test_splitk_add_rmsnorm_eps_decides_small_rows(cols, nslice, eps):
    g = _gen(cols)
    rows = 5
    scale = torch.tensor([1.0, 1e-3, 0.0, 1e-3, 10.0], device=DEV)[:, None]
    p = torch.randn(nslice, rows, cols, device=DEV, generator=g) * scale
    x = (torch.randn(rows, cols, device=DEV, generator=g) * scale).bfloat16()
    _run_splitk(p.contiguous(), x, _weight(g, cols), eps)


@pytest.mark.parametrize("cols", [1024, 10240])
def test_splitk_add_rmsnorm_refuses_other_widths(cols):
    from kgs.ops import KernelError
    from kgs.ops.transformer import splitk_add_rmsnorm

    g = _gen(2)
    with pytest.raises(KernelError):
        splitk_add_rmsnorm(torch.zeros(2, 1, cols, device=DEV), _randn(g, 1, cols), _weight(g, cols))


# ----------------------------------------------------------------------------
# argmax_rows

def test_argmax_rows_edges():
    """cols 65544 = 8 * 8193 chunks: thread 0 alone enters a second round of the clamped
    loads. The maximum at the last element and at 65536 (both in that round), an all -inf
    and an all-NaN row, a -0.0 / +0.0 tie (equal: the first index), in a strided view whose
    padding holds a larger value than any column."""
    from kgs.ops.transformer import argmax_rows

    cols = 65544
    x = _randn(_gen(3), 7, cols)
    x[0, cols - 1] = 50.0
    x[1, 65536] = 50.0
    x[2] = float("-inf")
    x[3] = float("nan")
    x[4] = -1.0
    x[4, 300] = -0.0
    x[4, 70] = 0.0
    x[4, 65540] = 0.0
    x[5] = -1.0
    x[5, 70] = -0.0
    x[5, 300] = 0.0
    xv, xbuf = R.wide(x, pad=64)
    assert float(xbuf[0, 0]) > 50.0
    got = argmax_rows(xv)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64
    assert torch.equal(got, R.ref_argmax(x))
    assert got.tolist()[:6] == [cols - 1, 65536, 0, 0, 70, 70]
    assert R.same_bits(xv, x) and R.poison_intact(xbuf, 7, cols)

