"""Shared helpers of the forward-kernel tests (tests/test_forward_*.py) and of the
training-kernel tests: float64 references of the decoder-block glue
(native/kernels/transformer.hip) and of the paged decode attention
(native/kernels/decode.hip), the per-element criterion, poisoned wide buffers, and
the checks themselves.

Every reference takes the bf16 (or e4m3 / fp32) tensors the kernel takes, on the
CPU or on a GPU, and evaluates the formula in ``dtype`` (float64 by default).
``dtype=torch.float32`` rounded once to bf16 is the *baseline*: what a correct
kernel computes up to the order of its sums. The ``check_*`` functions are the
criteria: the GPU tests apply them to the kernels' outputs,
tests/test_forward_criteria.py applies the same functions on the CPU to the
baseline (must be accepted) and to deliberately wrong evaluations (must be
rejected). Nothing in here is measured against a kernel.
"""
import math

import torch

REL = 2.0 ** -7
POISON = 1234.0
POISON_BYTE = 0xA5
E4M3_MAX = 448.0
FP8 = torch.float8_e4m3fn
PAGE = 32
HD = 128


# ----------------------------------------------------------------------------
# criterion and buffers

def within(out, ref, atol, what):
    """|out - ref| <= REL |ref| + atol elementwise (atol a number or a tensor); prints the margin."""
    err = (out.double() - ref).abs()
    slack = REL * ref.abs() + atol - err
    print(f"{what}: max err {err.max().item():.3e}, least margin {slack.min().item():.3e}")
    assert torch.isfinite(out.float()).all(), what
    assert slack.min().item() >= 0, (what, err.max().item(), slack.min().item())


def wide(t, pad=64, off=8, extra_rows=2, fill=POISON):
    """A copy of ``t`` as a view into a wider, taller poisoned buffer: (view, buffer)."""
    buf = torch.full((t.shape[0] + extra_rows, t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    view = buf[:t.shape[0], off:off + t.shape[1]]
    view.copy_(t)
    return view, buf


def poison_intact(buf, rows, cols, off=8, fill=POISON):
    return bool((buf[:, :off] == fill).all() and (buf[:, off + cols:] == fill).all() and
                (buf[rows:] == fill).all())


def wide_bytes(rows, cols, device, pad=48, off=16, extra_rows=2):
    """Room for an e4m3 [rows, cols] output inside a poisoned byte buffer whose row stride
    is a multiple of 16: (uint8 view, buffer)."""
    buf = torch.full((rows + extra_rows, (cols + pad + 15) // 16 * 16), POISON_BYTE, dtype=torch.uint8, device=device)
    return buf[:rows, off:off + cols], buf


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.uint8)


def same_bits(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def fp32_ulp(x):
    """The spacing of fp32 numbers at ``|x|`` (x a float64 tensor of normal magnitudes)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


# ----------------------------------------------------------------------------
# references

def ref_add_rmsnorm(x, d, w, eps=1e-5, dtype=torch.float64):
    """(residual bf16 -- the exact sum rounded once --, rmsnorm(residual) * w in ``dtype``)."""
    res = x if d is None else (x.float() + d.float()).to(torch.bfloat16)  # an fp32 sum of two bf16 is exact
    r = res.to(dtype)
    y = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w.to(dtype)
    return res, y


def ref_row_scale(y):
    """Per-row e4m3 scale max(amax, 1e-12) / 448 of ``y`` [rows, cols], in y's dtype."""
    return y.abs().amax(dim=1).clamp_min(1e-12) / E4M3_MAX


def ref_quantize_rows(y, sc):
    """The reference quantiser: ``clamp(y * (1 / sc), +-448)`` in fp32, converted to e4m3
    round-to-nearest-even, with the scales ``sc`` [rows] fp32 it is given. Returns bytes."""
    inv = (1.0 / sc.double()).float()  # the correctly rounded fp32 reciprocal, on any device
    q = (y.float() * inv[:, None]).clamp(-E4M3_MAX, E4M3_MAX)
    return q.to(FP8).view(torch.uint8)


def e4m3_order(codes):
    """e4m3 bytes -> integers ordered like the values they encode (+0 and -0 both 0)."""
    c = codes.view(torch.uint8).to(torch.int32)
    mag = c & 0x7f
    return torch.where(c >= 0x80, -mag, mag)


def ref_silu_mul(gu, dtype=torch.float64):
    i = gu.shape[1] // 2
    g, u = gu[:, :i].to(dtype), gu[:, i:].to(dtype)
    return g * torch.sigmoid(g) * u


def default_positions(tokens, seq, device):
    return (torch.arange(tokens, device=device) % seq).int()


def ref_rope(qkv, cos, sin, heads, hd, positions, dtype=torch.float64):
    """Rotate-half RoPE of the first ``heads`` heads of every row at ``positions`` (int
    tensor [tokens]) from the fp32 tables: ``(rotated [tokens, heads * hd], atol)`` in
    ``dtype``, atol the size of the two products of each element times 2^-23 (an fp32
    difference of products loses that much when the products cancel)."""
    t = qkv.shape[0]
    x = qkv[:, :heads * hd].to(dtype).reshape(t, heads, hd)
    p = positions.long()
    c, s = cos[p].to(dtype)[:, None, :], sin[p].to(dtype)[:, None, :]
    x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
    rot = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).reshape(t, heads * hd)
    mag = torch.cat(((x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()), dim=-1)
    return rot, 2.0 ** -23 * mag.reshape(t, heads * hd).double()


def ref_splitk_delta(partials):
    """bf16(((P0 + P1) + P2) + ...) summed in fp32 in slice order."""
    acc = partials[0].clone()
    for s in range(1, partials.shape[0]):
        acc = acc + partials[s]
    return acc.to(torch.bfloat16)


def cancelling_partials(nslice, rows, cols, gen, device):
    """fp32 partials whose sum cancels late: unit noise plus big, big, ..., -(nslice - 1) big
    with big ~ 1000 N(0, 1). The running sum stays large until the last slice, so its low
    bits -- and about one bf16 delta in thirty -- depend on the order of the slices."""
    p = torch.randn(nslice, rows, cols, generator=gen, device=device)
    coef = torch.ones(nslice, device=device)
    coef[-1] = -(nslice - 1)
    return (p + coef[:, None, None] * (1000 * torch.randn(rows, cols, generator=gen, device=device))).contiguous()


def ref_splitk_add_rmsnorm(partials, x, w, eps=1e-5, dtype=torch.float64):
    return ref_add_rmsnorm(x, ref_splitk_delta(partials), w, eps, dtype)


def ref_argmax(x):
    """torch.argmax's answer on the bf16 rows: the first index of the maximum, NaN the largest."""
    return x.float().argmax(dim=-1)


def kv_index_tables(device):
    """Where token tau, dim d of a page lives inside its K / V region (kgs.ops.decode.kv_index_tables)."""
    tau = torch.arange(PAGE, device=device)[:, None]
    d = torch.arange(HD, device=device)[None, :]
    k_idx = (((tau >> 4) * 4 + (d >> 5)) * 64 + ((d >> 3) & 3) * 16 + (tau & 15)) * 8 + (d & 7)
    v_idx = ((d >> 4) * 64 + ((tau >> 2) & 3) * 16 + (d & 15)) * 8 + (tau & 3) + 4 * (tau >> 4)
    return k_idx, v_idx


def gather_kv(cache_layer, pages, ntok, dtype=torch.float64):
    """The first ``ntok`` tokens a block-table row names: (k, v), each [ntok, HKV, 128] in
    ``dtype`` (an e4m3 cache is dequantised, scale 1)."""
    k_idx, v_idx = kv_index_tables(cache_layer.device)
    npg = (ntok + PAGE - 1) // PAGE
    sel = cache_layer[pages[:npg].long()]  # [npg, hkv, 2, 4096]
    hkv = cache_layer.shape[1]
    out = []
    for region, idx in ((0, k_idx), (1, v_idx)):
        t = sel[:, :, region].to(dtype)[..., idx]  # [npg, hkv, 32, 128]
        out.append(t.permute(0, 2, 1, 3).reshape(npg * PAGE, hkv, HD)[:ntok])
    return out[0], out[1]


def ref_paged_decode(q, cache_layer, block_tables, ctx_lens, heads, kv_heads, scale=None, dtype=torch.float64,
                     weights=False):
    """softmax(q K^T scale) V over the first ctx tokens of each sequence's pages:
    [B, heads * 128] in ``dtype``; with ``weights`` also the list of softmax weights [heads, ctx]."""
    scale = 1.0 / math.sqrt(HD) if scale is None else scale
    rep = heads // kv_heads
    outs, ws = [], []
    for i in range(q.shape[0]):
        ctx = int(ctx_lens[i])
        k, v = gather_kv(cache_layer, block_tables[i], ctx, dtype)
        qi = q[i, :heads * HD].to(dtype).reshape(kv_heads, rep, HD)
        s = torch.einsum("grd,tgd->grt", qi, k) * scale
        p = torch.softmax(s, dim=-1)
        outs.append(torch.einsum("grt,tgd->grd", p, v).reshape(-1))
        ws.append(p.reshape(heads, ctx))
    out = torch.stack(outs)
    return (out, ws) if weights else out


def baseline(ref, *args, **kw):
    """The same formula in fp32 torch, rounded once to bf16."""
    out = ref(*args, dtype=torch.float32, **kw)
    if isinstance(out, tuple):
        return tuple(o.to(torch.bfloat16) if o.dtype == torch.float32 else o for o in out)
    return out.to(torch.bfloat16)


# ----------------------------------------------------------------------------
# criteria

def check_add_rmsnorm(res, y, x, d, w, eps, what="add_rmsnorm"):
    """Residual: the bits of bf16(x + d). y: every element within REL of float64, atol 0 --
    the kernel rounds an fp32 value once to bf16 (2^-9) and its fp32 steps (a sum of
    squares, rsqrt, two products) add a few 2^-24, all relative; bf16 shares fp32's
    exponent range, so nothing underflows into an absolute term. Returns the reference."""
    rres, ry = ref_add_rmsnorm(x, d, w, eps)
    assert same_bits(res, rres), what + ": residual"
    within(y, ry, 0.0, what + " y")
    return ry


def check_splitk_add_rmsnorm(res, y, partials, x, w, eps, what="splitk_add_rmsnorm"):
    """As check_add_rmsnorm, the delta being the fp32 slice-order sum rounded to bf16."""
    rres, ry = ref_splitk_add_rmsnorm(partials, x, w, eps)
    assert same_bits(res, rres), what + ": residual"
    within(y, ry, 0.0, what + " y")


def check_row_scale(ys, y64, what):
    """ys within one fp32 ulp of max(amax, 1e-12) / 448 of the float64 rows."""
    want = ref_row_scale(y64.double())
    err = (ys.double() - want).abs() / fp32_ulp(want)
    print(f"{what}: scale error {err.max().item():.3f} ulp")
    assert ys.dtype == torch.float32 and torch.isfinite(ys).all(), what
    assert err.max().item() <= 1.0, (what, err.max().item())


def check_codes_bitwise(y8, ys, ybf, what):
    """Codes are the reference quantiser's on the bf16 rows ``ybf`` with the scales given."""
    want = ref_quantize_rows(ybf, ys)
    bad = int((y8.view(torch.uint8) != want).sum())
    assert bad == 0, (what, bad)


FP8_EQUAL_SHARE = 0.99


def check_codes_near(y8, ys, y64, what):
    """Codes within one e4m3 code of the float64 rows quantised with the scales given, and
    equal for at least FP8_EQUAL_SHARE of the elements."""
    want = e4m3_order(ref_quantize_rows(y64, ys))
    dist = (e4m3_order(y8) - want).abs()
    share = (dist == 0).double().mean().item()
    print(f"{what}: code distance max {int(dist.max())}, equal share {share:.6f}")
    assert int(dist.max()) <= 1, (what, int(dist.max()))
    assert share >= FP8_EQUAL_SHARE, (what, share)
    return share


SILU_ATOL = 1e-35


def check_silu_mul(out, gu, what="silu_mul"):
    """Per element against float64. atol 1e-35: for a gate below -88.7 fp32's exp(-g)
    overflows and the quotient is 0 where the exact |silu(g)| is below 88.8 * 2^-128 =
    2.6e-37, times |u| < 32; above that every step is a relative fp32 error (the exp's
    argument reduction costs |g| 2^-24 ln 2 < 6e-6 at |g| = 100) and one bf16 rounding."""
    ref = ref_silu_mul(gu)
    within(out, ref, SILU_ATOL, what)
    return ref


def check_rope(got, orig, cos, sin, heads, hd, positions, what="rope"):
    """Rotated heads per element against float64 (atol: ref_rope's cancellation term);
    every other column bitwise untouched."""
    ref, atol = ref_rope(orig, cos, sin, heads, hd, positions)
    within(got[:, :heads * hd], ref, atol, what)
    assert same_bits(got[:, heads * hd:], orig[:, heads * hd:]), what + ": columns past the rotated heads"


def decode_row_errors(out, ref64, heads):
    """max |out - ref64| of every (sequence, head) row over max |ref64| of that row: [B, heads]."""
    b = ref64.shape[0]
    o = out.double().reshape(b, heads, HD)
    r = ref64.reshape(b, heads, HD)
    return (o - r).abs().amax(-1) / r.abs().amax(-1)


def check_decode_against_baseline(out, base, ref64, heads, what):
    """Per sequence (one context length each): the largest |out - ref64| over the rows of the
    sequence, each row relative to its max |ref64|, is at most twice the same figure of the
    baseline, and the baseline's is under 2e-2. Two numbers per sequence, as in
    test_gradients_are_within_twice_the_bf16_baselines_error -- a row-by-row comparison
    would hold the kernel to the luck of the baseline's 128 roundings in that row. A
    one-key context has a baseline error of 0 and so demands the exact V row."""
    e_out = decode_row_errors(out, ref64, heads).amax(dim=1)
    e_base = decode_row_errors(base, ref64, heads).amax(dim=1)
    print(f"{what}: err {[f'{e:.3e}' for e in e_out.tolist()[:8]]}, baseline "
          f"{[f'{e:.3e}' for e in e_base.tolist()[:8]]}, least margin {(2 * e_base - e_out).min().item():.3e}")
    assert torch.isfinite(out.float()).all(), what
    assert e_base.max().item() < 2e-2, (what, e_base.max().item())  # no hiding behind a bad baseline
    assert bool((e_out <= 2 * e_base).all()), (what, e_out.tolist()[:8], e_base.tolist()[:8])


NEEDLE_WEIGHT = 1 - 2.0 ** -12
SCORE_BOUND = 6.0  # |q.k| / sqrt(128) of unit-scale keys against a unit-scale q: N(0, 1), six sigma


def needle_gain(ctx):
    """c of the needle key c q / |q|: its score is c |q| / sqrt(128), about c for a
    unit-scale q; the other ctx - 1 keys score below SCORE_BOUND, so their weight is at
    most ctx exp(SCORE_BOUND - c). c = ln ctx + SCORE_BOUND + 17 ln 2 makes that 2^-17 --
    2^-12 with a factor 32 in hand for |q| != sqrt(128) and e4m3's rounding of the key."""
    return math.log(ctx) + SCORE_BOUND + 17 * math.log(2.0)




# ----------------------------------------------------------------------------
# paged decode scenarios (CPU or GPU)

class DecodeCase:
    """A batch for the paged decode attention, described by what the fused RoPE entry
    takes -- pre-rotation rows ``qkv_pre`` [B, (H + 2 HKV) * 128] of the new token of every
    sequence, at position ctx - 1 -- from which follow the rotated query the plain entry
    takes (float64 RoPE rounded to bf16) and the new token's K / V in the cache."""

    def copy(self):
        c = DecodeCase()
        c.__dict__.update(self.__dict__)
        c.qkv_pre = self.qkv_pre.clone()
        return c


def decode_case(heads, hkv, kv_dtype, ctxs, device, seed, cos, sin, extra_pages=3, group_q=False, kv_scale=1.0):
    """Scattered pages, a block table ``extra_pages`` wider than the longest context needs with
    every entry a valid page of its own, K / V at ``kv_scale``, q at unit scale (``group_q``:
    one row shared by the heads of a KV group). ``cache`` holds random tokens everywhere;
    :func:`decode_turn` stores the new token and the needles into a copy."""
    g = torch.Generator(device=device).manual_seed(seed)
    b = len(ctxs)
    width = max((c + PAGE - 1) // PAGE for c in ctxs) + extra_pages
    npages = b * width + 4
    c = DecodeCase()
    c.heads, c.hkv, c.ctxs, c.b, c.width, c.device = heads, hkv, list(ctxs), b, width, device
    c.cos, c.sin = cos, sin
    c.bt = torch.randperm(npages, generator=g, device=device)[:b * width].view(b, width).int().contiguous()
    c.ctx_t = torch.tensor(c.ctxs, dtype=torch.int32, device=device)
    c.pos = (c.ctx_t - 1).contiguous()
    last = c.pos.long()
    c.slots = (c.bt.gather(1, (last // PAGE).view(-1, 1)).view(-1).long() * PAGE + last % PAGE).int().contiguous()
    dt = FP8 if kv_dtype == "fp8" else torch.bfloat16
    c.cache = (kv_scale * torch.randn(npages, hkv, 2, PAGE * HD, generator=g, device=device)).to(dt)
    qpre = torch.randn(b, hkv if group_q else heads, HD, generator=g, device=device)
    if group_q:
        qpre = qpre.repeat_interleave(heads // hkv, dim=1)
    kv = kv_scale * torch.randn(b, 2 * hkv, HD, generator=g, device=device)
    c.qkv_pre = torch.cat((qpre, kv), dim=1).reshape(b, (heads + 2 * hkv) * HD).bfloat16()
    return c


def rotate_rows(rows, cos, sin, nheads, pos, inverse=False):
    """float64 RoPE (head_dim 128) of the first ``nheads`` heads of each row, rounded to bf16."""
    return ref_rope(rows, cos, -sin if inverse else sin, nheads, HD, pos)[0].to(torch.bfloat16)


def write_tokens(cache_layer, pages, taus, k=None, v=None):
    """Store K and / or V rows [n, HKV, 128] of n tokens at (pages[n], taus[n]) (saturating for e4m3)."""
    k_idx, v_idx = kv_index_tables(cache_layer.device)
    hk = torch.arange(cache_layer.shape[1], device=cache_layer.device)[None, :, None]
    pg = pages.long()[:, None, None]

    def cvt(t):
        if cache_layer.dtype == FP8:
            return t.float().clamp(-E4M3_MAX, E4M3_MAX).to(FP8)
        return t.to(cache_layer.dtype)

    if k is not None:
        cache_layer[pg, hk, 0, k_idx[taus.long()][:, None, :]] = cvt(k)
    if v is not None:
        cache_layer[pg, hk, 1, v_idx[taus.long()][:, None, :]] = cvt(v)


def needle_keys(q, ctxs, heads, hkv):
    """The needle of every (sequence, KV group): needle_gain(ctx) q / |q| of the group's first head, [B, HKV, 128]."""
    qg = q[:, :heads * HD].reshape(q.shape[0], hkv, heads // hkv, HD)[:, :, 0].double()
    gain = torch.tensor([needle_gain(c) for c in ctxs], dtype=torch.float64, device=q.device)[:, None, None]
    return (gain * qg / qg.norm(dim=-1, keepdim=True)).to(torch.bfloat16)


def needle_positions(ctx, pps):
    """Key indices at which the needle is placed in turn: key 0, key ctx - 1, and the first
    and the last valid slot of the first and of the last page of every split (the last
    split's last page is the last valid table entry)."""
    npg = (ctx + PAGE - 1) // PAGE
    keys = {0, ctx - 1}
    for p0 in range(0, npg, pps):
        for p in (p0, min(npg, p0 + pps) - 1):
            keys.add(p * PAGE)
            keys.add(min(ctx - 1, p * PAGE + PAGE - 1))
    return sorted(keys)


def outside_positions(ctx, width):
    """Key indices past the context where a needle must change nothing: ctx, ctx + 1, the
    last slot of the last partial page, and the first and last slot of every table entry
    beyond the context."""
    npg = (ctx + PAGE - 1) // PAGE
    keys = {ctx, ctx + 1, npg * PAGE - 1}
    for p in range(npg, width):
        keys.add(p * PAGE)
        keys.add(p * PAGE + PAGE - 1)
    return sorted(k for k in keys if ctx <= k < width * PAGE)


def decode_turn(base, needles=None, outside=False):
    """One launch's inputs from ``base``: ``(case, q, cache)``. ``needles[i]`` is the key index
    of sequence i that becomes its needle (key ctx - 1 is the new token: its pre-rotation K
    in ``case.qkv_pre`` is the needle rotated back). ``outside``: needles with V rows of 100
    at every :func:`outside_positions` key of every sequence, all past its context."""
    c = base.copy()
    heads, hkv, b, dev = c.heads, c.hkv, c.b, c.device
    seqs = torch.arange(b, device=dev)
    if needles is not None:
        keys = torch.tensor(needles, device=dev)
        new = keys == c.pos.long()
        q0 = rotate_rows(c.qkv_pre, c.cos, c.sin, heads, c.pos)
        back = rotate_rows(needle_keys(q0, c.ctxs, heads, hkv).reshape(b, hkv * HD), c.cos, c.sin, hkv, c.pos,
                           inverse=True)
        c.qkv_pre[new, heads * HD:(heads + hkv) * HD] = back[new]
    rot = rotate_rows(c.qkv_pre, c.cos, c.sin, heads + hkv, c.pos)
    q = rot[:, :heads * HD].contiguous()
    cache = c.cache.clone()
    write_tokens(cache, c.slots.long() // PAGE, c.slots.long() % PAGE,
                 rot.reshape(b, -1, HD)[:, heads:heads + hkv], c.qkv_pre.reshape(b, -1, HD)[:, heads + hkv:])
    nk = needle_keys(q, c.ctxs, heads, hkv)
    if needles is not None and bool((~new).any()):
        old = seqs[~new]
        write_tokens(cache, c.bt[old, keys[old] // PAGE], keys[old] % PAGE, k=nk[old])
    if outside:
        pairs = [(i, k) for i, ctx in enumerate(c.ctxs) for k in outside_positions(ctx, c.width)]
        si = torch.tensor([p[0] for p in pairs], device=dev)
        ki = torch.tensor([p[1] for p in pairs], device=dev)
        write_tokens(cache, c.bt[si, ki // PAGE], ki % PAGE, k=nk[si],
                     v=torch.full((len(pairs), hkv, HD), 100.0, device=dev))
    return c, q, cache


def check_needles(out, q, cache, c, needles, what):
    """Every (sequence, head) row of ``out`` against the V row of that sequence's needle: one
    bf16 rounding (2^-8 |v|) plus what the other keys can add, (1 - w)(|v| + vmax), with w the
    needle's float64 softmax weight (asserted >= NEEDLE_WEIGHT) and vmax the largest |V| of
    the context."""
    heads, hkv = c.heads, c.hkv
    rep = heads // hkv
    slacks, weights = [], []
    for i, (ctx, key) in enumerate(zip(c.ctxs, needles)):
        k, v = gather_kv(cache, c.bt[i], ctx)
        qi = q[i, :heads * HD].double().reshape(hkv, rep, HD)
        p = torch.softmax(torch.einsum("grd,tgd->grt", qi, k) / math.sqrt(HD), dim=-1)
        w = p[:, :, key].amin(-1)[:, None, None]
        vn = v[key][:, None, :].abs()
        vmax = v.abs().amax(dim=(0, 2))[:, None, None]
        err = (out[i, :heads * HD].double().reshape(hkv, rep, HD) - v[key][:, None, :]).abs()
        slacks.append((2.0 ** -8 * vn + (1 - w) * (vn + vmax) - err).min())
        weights.append(w.min())
    slack, weight = torch.stack(slacks).min().item(), torch.stack(weights).min().item()
    print(f"{what}: needles {needles[:8]}: least weight 1 - {1 - weight:.2e}, least margin {slack:.3e}")
    assert torch.isfinite(out.float()).all(), what
    assert weight >= NEEDLE_WEIGHT, (what, weight)
    assert slack >= 0, (what, slack)
