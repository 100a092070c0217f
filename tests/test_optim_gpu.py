"""GPU tests of the fused AdamW (native/kernels/optimizer.hip) under
``kgs.optim.AdamW(backend="kgs")``.

Every check of the kernels compares one step against the float64 reference
(``ref_adamw_step``) fed the kernel's own inputs: the fp32 state read back before
the step, that step's bf16 gradients, the clip factor the device computed, and lr,
weight decay, betas and eps as the fp32 values the kernel is handed. The bounds
are therefore one-step bounds and do not accumulate:

* m, v:    ``|out - ref| <= 2^-22 |ref| + 2^-125``
* master:  ``|out - ref| <= 2^-23 |ref| + lr 2^-20 |u_ref| + 2^-125`` with ``u_ref =
  m_hat / (sqrt(v_hat) + eps)``: the first term is the rounding of ``1 - lr wd`` and
  of the stored result, the second allows about 16 fp32 roundings on the way to
  ``lr u`` (m and v carry two each, two divisions, the square root, the sum with
  eps, the rounded bias corrections, the product with lr)
* bf16 weight: bitwise the stored master ``.bfloat16()``
* grad_norm^2: within ``n 2^-24 sum g^2`` of the float64 sum, the textbook bound of
  an fp32 sum of n terms in any order

Each test prints its least margin."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
BF = torch.bfloat16
POISON = 1536.0  # exact in bf16
BETAS, EPS = (0.9, 0.95), 1e-8
KEYS = ("master", "exp_avg", "exp_avg_sq")


def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _chunk():
    from kgs.ops.optim import adamw_chunk

    return adamw_chunk()


def _grad(g, n, special=True, scale=1.0):
    """bf16 gradients: gaussian, with zeros, +-1e-30 and +-1e4 sprinkled in; no NaN."""
    x = scale * torch.randn(n, device=DEV, generator=g)
    if special:
        i = torch.arange(n, device=DEV)
        for mod, rem, val in ((7, 0, 0.0), (7, 1, 1e-30), (7, 2, -1e-30), (11, 3, 1e4), (11, 4, -1e4)):
            x[i % mod == rem] = val
    return x.to(BF)


def _wide(t, off=8, pad=24):
    """A copy of 1-D ``t`` as a view at an 8-element offset inside a poisoned buffer: (view, buffer)."""
    buf = torch.full((t.numel() + off + pad,), POISON, dtype=t.dtype, device=t.device)
    view = buf[off:off + t.numel()]
    view.copy_(t)
    return view, buf


def _poison_intact(buf, n, off=8):
    return bool((buf[:off] == POISON).all() and (buf[off + n:] == POISON).all())


class Case:
    """Parameters (views into poisoned buffers), an optimizer on them, gradients."""

    def __init__(self, numels, seed=0, none=(), groups=None, zero_state=lambda i: i % 2 == 1, step0=0, **kw):
        from kgs.optim import AdamW

        g = _gen(seed)
        self.gen = g
        made, bufs = [], {}
        for n in numels:
            view, buf = _wide(torch.randn(n, device=DEV, generator=g).to(BF))
            made.append(view.requires_grad_(True))
            bufs[id(made[-1])] = buf
        if groups is None:
            groups = [{"params": made}]
        else:  # [(indices, lr, wd)]
            groups = [{"params": [made[i] for i in idx], "lr": lr, "weight_decay": wd} for idx, lr, wd in groups]
        self.opt = AdamW(groups, betas=BETAS, eps=EPS, backend="kgs", **kw)
        self.params = self.opt._params  # in group order, as everything below
        self.wbufs = [bufs[id(p)] for p in self.params]
        self.numels = [p.numel() for p in self.params]
        self.none = {i for i, p in enumerate(self.params) if any(p is made[j] for j in none)}
        # poison the padding of the flat state buffers, fill the state
        self.pad = torch.ones(self.opt._flat["master"].numel(), dtype=torch.bool, device=DEV)
        for off, n in zip(self.opt._offsets, self.numels):
            self.pad[off:off + n] = False
        for k in KEYS:
            self.opt._flat[k][self.pad] = POISON
        for i, p in enumerate(self.params):
            st = self.opt.state[p]
            if not zero_state(i):
                st["exp_avg"].copy_(0.1 * torch.randn(p.numel(), device=DEV, generator=g))
                st["exp_avg_sq"].copy_(0.01 * torch.rand(p.numel(), device=DEV, generator=g))
        if step0:
            from kgs.ops.optim import STATE_STEP

            self.opt._state[STATE_STEP] = step0
        self.gbufs = [None] * len(self.params)

    def set_grads(self, special=True, scale=1.0, fresh=True):
        for i, p in enumerate(self.params):
            if i in self.none:
                p.grad = None
                continue
            new = _grad(self.gen, p.numel(), special, scale)
            if fresh or p.grad is None:
                p.grad, self.gbufs[i] = _wide(new)
            else:
                p.grad.copy_(new)

    def snapshot(self):
        return {"w": [b.clone() for b in self.wbufs], "g": [None if b is None else b.clone() for b in self.gbufs],
                **{k: self.opt._flat[k].clone() for k in KEYS}, "state": self.opt._state.clone()}

    def borders_intact(self):
        ok = all(_poison_intact(b, n) for b, n in zip(self.wbufs, self.numels))
        ok = ok and all(b is None or _poison_intact(b, n) for b, n in zip(self.gbufs, self.numels))
        return ok and all(bool((self.opt._flat[k][self.pad] == POISON).all()) for k in KEYS)


def _same(a, b, skip=("state", "g")):
    for k in a:
        if k in skip:
            continue
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            if not torch.equal(x.view(torch.int16) if x.dtype == BF else x.view(torch.int32),
                               y.view(torch.int16) if y.dtype == BF else y.view(torch.int32)):
                return False
    return True


def _check_step(case, before, step, clip=1.0, what=""):
    """One step of ``case.opt`` against the float64 reference on the state ``before``
    it (a snapshot); returns the least margins. Tensors without a gradient must be
    bitwise unchanged."""
    from kgs.ops.optim import ref_adamw_step

    opt = case.opt
    betas, eps = tuple(_f32(b) for b in BETAS), _f32(EPS)
    group_of = opt._group_of
    least = {"m": float("inf"), "v": float("inf"), "p": float("inf")}
    for i, (p, off, n) in enumerate(zip(case.params, opt._offsets, case.numels)):
        st = opt.state[p]
        seg = {k: before[k][off:off + n] for k in KEYS}
        if p.grad is None:
            for k in KEYS:
                assert torch.equal(st[k].reshape(-1), seg[k]), (what, i, k)
            assert torch.equal(p.detach().reshape(-1), before["w"][i][8:8 + n]), (what, i)
            continue
        grp = opt.param_groups[group_of[i]]
        lr, wd = _f32(grp["lr"]), _f32(grp["weight_decay"])
        rp, rm, rv = ref_adamw_step(seg["master"], seg["exp_avg"], seg["exp_avg_sq"], p.grad.reshape(-1), step, lr,
                                    betas, eps, wd, clip=clip)
        u = (rm / (1 - betas[0] ** step)) / ((rv / (1 - betas[1] ** step)).sqrt() + eps)
        tiny = 2.0 ** -125
        for key, out, ref, tol in (("m", st["exp_avg"], rm, 2.0 ** -22 * rm.abs() + tiny),
                                   ("v", st["exp_avg_sq"], rv, 2.0 ** -22 * rv.abs() + tiny),
                                   ("p", st["master"], rp, 2.0 ** -23 * rp.abs() + lr * 2.0 ** -20 * u.abs() + tiny)):
            assert torch.isfinite(out).all(), (what, i, key)
            if n == 0:
                continue
            # margin relative to the bound: 1 = exact, 0 = at the bound
            margin = (1 - (out.reshape(-1).double() - ref).abs() / tol).min().item()
            least[key] = min(least[key], margin)
            assert margin >= 0, (what, i, n, key, margin)
        assert torch.equal(p.detach().reshape(-1).view(torch.int16),
                           st["master"].reshape(-1).to(BF).view(torch.int16)), (what, i)
    print(f"{what}: least margin (share of the bound left) m {least['m']:.3f} v {least['v']:.3f} p {least['p']:.3f}")
    return least


def _sizes():
    c = _chunk()
    return [0, 1, 7, 8, 9, 511, 512, 4097, c - 1, c, c + 1, 3 * c + 5, 100]


# ----------------------------------------------------------------------------
# shapes, borders

@pytest.mark.parametrize("step", [1, 1000])
def test_every_tail_length_two_groups_and_a_skipped_tensor(step):
    sizes = _sizes()
    n = len(sizes)
    case = Case(sizes, seed=step, none={n - 1},
                groups=[(list(range(0, n, 2)), 1e-3, 0.1), (list(range(1, n, 2)), 3e-2, 0.0)], step0=step - 1)
    case.set_grads()
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    _check_step(case, before, step, what=f"shapes step {step}")
    assert case.borders_intact()
    assert all(torch.equal(a, b) for a, b in zip(before["g"], case.snapshot()["g"]) if a is not None)
    assert case.opt.step_count == step and case.opt.skipped_steps == 0
    assert case.opt.table_refreshes == 1 and case.opt._nchunks == sum(-(-s // _chunk()) for s in sizes)


@pytest.mark.parametrize("count", [1, 2, 3, 64, 65, 200])
def test_tensor_counts_across_the_table_searchs_boundaries(count):
    sizes = [(5 * i) % 23 for i in range(count)]  # tiny, some empty (every 23rd)
    sizes[-1] = 9
    if count >= 64:
        sizes[31] = _chunk() + 3  # one tensor of two chunks in the middle
    case = Case(sizes, seed=count, max_grad_norm=1e9)
    case.set_grads(special=False)
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    assert case.opt.clip == 1.0
    _check_step(case, before, 1, what=f"{count} tensors")
    assert case.borders_intact()


def test_borders_and_skipped_tensors_survive_three_steps():
    c = _chunk()
    case = Case([1, 7, 9, 511, c + 1, 0, 15], seed=5, none={2, 4}, max_grad_norm=10.0, weight_decay=0.1)
    for step in (1, 2, 3):
        case.set_grads(special=False)
        before = case.snapshot()
        case.opt.step()
        torch.cuda.synchronize()
        _check_step(case, before, step, clip=case.opt.clip, what=f"borders step {step}")
        assert case.borders_intact()


# ----------------------------------------------------------------------------
# repeatability

def test_three_steps_are_bitwise_repeatable():
    runs = []
    for _ in range(2):
        case = Case(_sizes(), seed=7, max_grad_norm=1.0, weight_decay=0.1, lr=1e-2)
        for _ in range(3):
            case.set_grads(special=False)
            case.opt.step()
        torch.cuda.synchronize()
        runs.append(case.snapshot())
    assert _same(runs[0], runs[1], skip=()) and torch.equal(runs[0]["state"], runs[1]["state"])
    assert runs[0]["state"][0].item() == 3


def test_every_streaming_variant_is_bitwise_the_default():
    """The variants differ in cache policy and in groups per trip, never in arithmetic
    or in summation order."""
    from kgs.ops import optim as ops

    def run(variant):
        case = Case(_sizes(), seed=8, none={3}, max_grad_norm=1.0, weight_decay=0.1, lr=1e-2)
        for _ in range(2):
            case.set_grads(special=False)
            opt = case.opt
            if variant is None:
                opt.step()
                continue
            opt._update_table()
            opt.update_groups()
            ops.grad_norm(opt._table, opt._nchunks, opt._state, opt.betas, partials=opt._partials,
                          max_norm=opt.max_grad_norm, variant=variant & 1)
            ops.adamw_step_(opt._table, opt._nchunks, opt._groups, opt._state, opt.betas, opt.eps, variant=variant)
        torch.cuda.synchronize()
        assert case.borders_intact()
        return case.snapshot()

    want = run(None)
    for variant in range(6):
        got = run(variant)
        assert _same(want, got, skip=("g",)) and torch.equal(want["state"], got["state"]), variant


# ----------------------------------------------------------------------------
# clipping, skipping

def _norm_check(case, what):
    from kgs.ops.optim import ref_grad_norm

    grads = [p.grad for p in case.params if p.grad is not None]
    n = sum(g.numel() for g in grads)
    ss = ref_grad_norm(grads).item() ** 2
    got = case.opt.grad_norm
    bound = n * 2.0 ** -24 * ss
    print(f"{what}: grad_norm {got:.6e}, |norm^2 - ref| {abs(got * got - ss):.3e}, bound {bound:.3e}")
    assert abs(got * got - ss) <= bound
    return got


def test_clipping_below_the_norm_is_the_reference_step_on_the_scaled_gradient():
    case = Case(_sizes(), seed=9, max_grad_norm=0.5, weight_decay=0.1)
    case.set_grads(special=False)
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    norm, clip = _norm_check(case, "clip"), case.opt.clip
    assert norm > 0.5 and clip < 1.0
    # two fp32 roundings (the sum with 1e-6, the division) from the fp32 norm to clip
    assert abs(clip - 0.5 / (norm + 1e-6)) <= 2.0 ** -22 * clip
    _check_step(case, before, 1, clip=clip, what="clipped step")
    # the special values too: the norm is then ~1e4 sqrt(n / 11)
    case.set_grads()
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    _norm_check(case, "clip, special values")
    _check_step(case, before, 2, clip=case.opt.clip, what="clipped step, special values")


def test_clipping_above_the_norm_is_bitwise_the_unclipped_step():
    out = {}
    for name, kw in (("off", {}), ("on", {"max_grad_norm": 1e6})):
        case = Case(_sizes(), seed=10, **kw)
        for _ in range(2):
            case.set_grads(special=False)
            case.opt.step()
        torch.cuda.synchronize()
        out[name] = case.snapshot()
        if kw:
            assert case.opt.clip == 1.0
            _norm_check(case, "no clip")
    assert _same(out["off"], out["on"], skip=("state",))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_gradient_that_is_not_finite_skips_the_step(bad):
    case = Case(_sizes()[:-1] + [13], seed=11, max_grad_norm=1.0, weight_decay=0.1)
    case.set_grads(special=False)
    case.opt.step()
    case.set_grads(special=False)
    case.params[-1].grad[-1] = bad
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    after = case.snapshot()
    assert _same(before, after, skip=("state",))
    assert case.opt.step_count == 1 and case.opt.skipped_steps == 1 and case.borders_intact()
    case.set_grads(special=False)
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    assert case.opt.step_count == 2 and case.opt.skipped_steps == 1
    _check_step(case, before, 2, clip=case.opt.clip, what="the step after a skipped one")


# ----------------------------------------------------------------------------
# graph capture, table refresh

def test_a_captured_step_replays_eager_steps_bitwise_and_follows_lr():
    sizes = _sizes()
    eager, graph = (Case(sizes, seed=12, max_grad_norm=1.0, weight_decay=0.1, lr=1e-2) for _ in range(2))
    grads = [[_grad(_gen(100 + k), n, special=False) for n in eager.numels] for k in range(4)]

    def load(case, k):
        for p, g in zip(case.params, grads[k]):
            if p.grad is None:
                p.grad = torch.empty_like(g)
            p.grad.copy_(g)

    for case in (eager, graph):  # step 1, eager on both: builds the table, warms up
        load(case, 0)
        case.opt.step()
        case.opt.zero_grad(set_to_none=False)
    torch.cuda.synchronize()
    refreshes = (graph.opt.table_refreshes, graph.opt.group_refreshes)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph.opt.step()
    assert (graph.opt.table_refreshes, graph.opt.group_refreshes) == refreshes == (1, 1)
    for k in (1, 2, 3):
        if k == 3:  # a new lr, no re-capture
            for case in (eager, graph):
                case.opt.param_groups[0]["lr"] = 5e-3
            assert graph.opt.update_groups()
        load(eager, k)
        eager.opt.step()
        eager.opt.zero_grad(set_to_none=False)
        load(graph, k)
        g.replay()
        graph.opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        a, b = eager.snapshot(), graph.snapshot()
        assert _same(a, b, skip=("g",)) and torch.equal(a["state"], b["state"]), k
    assert graph.opt.step_count == 4 and graph.opt.table_refreshes == 1
    # the lr did take effect: a third run that keeps 1e-2 ends elsewhere
    third = Case(sizes, seed=12, max_grad_norm=1.0, weight_decay=0.1, lr=1e-2)
    for k in range(4):
        load(third, k)
        third.opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(third.snapshot()["master"], graph.snapshot()["master"])


def test_reallocated_gradients_are_followed():
    case = Case([9, 512, _chunk() + 1, 100], seed=13, none={3}, max_grad_norm=1.0)
    keep = []
    for step in (1, 2, 3):
        case.opt.zero_grad(set_to_none=True)
        if step == 3:
            case.none = set()  # the tensor that had no gradient gets one
        case.set_grads(special=False, fresh=True)
        keep.append(list(case.gbufs))  # the old ones stay allocated: new addresses
        before = case.snapshot()
        case.opt.step()
        torch.cuda.synchronize()
        assert case.opt.table_refreshes == step
        _check_step(case, before, step, clip=case.opt.clip, what=f"refresh step {step}")
    case.opt.step()  # nothing moved: no refresh
    assert case.opt.table_refreshes == 3


# ----------------------------------------------------------------------------
# raw entries

def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    from kgs.ops import _lib
    from kgs.ops.optim import adamw_table

    lib = _lib.lib()
    w = torch.full((32,), POISON, dtype=BF, device=DEV)
    f = [torch.full((32,), POISON, device=DEV) for _ in range(3)]
    g = torch.ones(32, dtype=BF, device=DEV)
    host, nchunks = adamw_table([w], [f[0]], [f[1]], [f[2]], [g], [0], 1, pin=False)
    assert nchunks == 1 and lib.kgs_adamw_row_bytes() == 64 and lib.kgs_adamw_state_bytes() == 32
    bad = host.clone()
    bad[0, 4] += 2
    assert lib.kgs_adamw_table_check(bad.data_ptr(), 1, 1) == -2  # KGS_ERR_ALIGN: misaligned gradient
    bad = host.clone()
    bad[0, 1] = 0
    assert lib.kgs_adamw_table_check(bad.data_ptr(), 1, 1) == -2  # null master
    bad = host.clone()
    bad[0, 7] = 1
    assert lib.kgs_adamw_table_check(bad.data_ptr(), 1, 1) == -1  # KGS_ERR_SHAPE: chunk0 is not the prefix
    bad = host.clone()
    bad[0, 5] = -1
    assert lib.kgs_adamw_table_check(bad.data_ptr(), 1, 1) == -1
    assert lib.kgs_adamw_table_check(host.data_ptr(), 1, 0) == -3  # KGS_ERR_ARG: group out of range
    with pytest.raises(ValueError, match="aligned"):
        adamw_table([w[1:9]], [f[0][:8]], [f[1][:8]], [f[2][:8]], [g[:8]], [0], 1)
    table = host.to(DEV)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    groups = torch.tensor([[1e-3, 0.0]], device=DEV)
    parts = torch.full((4,), POISON, device=DEV)
    st = _lib.stream_handle(w.device)
    T, S, G, P = table.data_ptr(), state.data_ptr(), groups.data_ptr(), parts.data_ptr()
    assert lib.kgs_adamw_grad_sumsq_v(T, 1, 1, P, 6, st) == -3 and lib.kgs_adamw_grad_sumsq(T + 8, 1, 1, P, st) == -2
    assert lib.kgs_adamw_grad_sumsq(T, 1, -1, P, st) == -1 and lib.kgs_adamw_grad_sumsq(T, 0, 1, P, st) == -1
    assert lib.kgs_adamw_grad_sumsq(T, 1, 1, 0, st) == -2
    assert lib.kgs_adamw_finalize(P, 1, 1.0, 0.9, 0.95, S + 4, st) == -2
    assert lib.kgs_adamw_finalize(P, 1, 0.0, 0.9, 0.95, S, st) == -3
    assert lib.kgs_adamw_finalize(P, 1, 1.0, 1.0, 0.95, S, st) == -3
    assert lib.kgs_adamw_finalize(0, 1, 1.0, 0.9, 0.95, S, st) == -2
    assert lib.kgs_adamw_step_v(T, 1, 1, G, S, 0.9, 0.95, 1e-8, 7, st) == -3
    assert lib.kgs_adamw_step(T, 1, 1, G + 4, S, 0.9, 0.95, 1e-8, st) == -2
    assert lib.kgs_adamw_step(T, 1, 1, G, S, 0.9, 0.95, -1.0, st) == -3
    assert lib.kgs_adamw_step(T, 1, 0, G, S, 0.9, 0.95, 1e-8, st) == 0  # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert (w == POISON).all() and all((t == POISON).all() for t in f) and (parts == POISON).all()
    assert int(state.count_nonzero()) == 0


# ----------------------------------------------------------------------------
# DecoderLM, end to end

def test_decoder_lm_trains_with_masters_and_every_step_is_the_reference_step():
    """Eight AdamW steps (clipped at 1.0, matrices decayed) of the small DecoderLM of
    test_decoder_lm_sgd_steps_track_the_fp32_copy on one fixed batch: every step
    within the one-step bounds of the float64 reference fed that step's real
    gradients, the weights always the rounded masters, the norm weights' masters off
    1.0 (a bf16 norm weight alone would not move at this lr), and the loss at least
    halved: a sanity cap, the torch backend of this configuration memorises the
    batch (7.45 to below 0.01) with or without masters."""
    from kgs.models.decoder import DecoderLM
    from kgs.optim import AdamW, decay_groups

    vocab, dim, nl, nh, nkv, inter, b, s = 1024, 512, 2, 4, 1, 1536, 2, 128
    g = _gen(11)
    tokens = torch.randint(0, vocab, (b, s), device=DEV, generator=g)
    targets = tokens.roll(-1, 1).clone()
    targets[:, -1] = -100
    lm = DecoderLM(vocab, dim, nl, nh, nkv, inter, backend="kgs", device=DEV)
    opt = AdamW(decay_groups(lm, 0.1), lr=1e-3, betas=BETAS, eps=EPS, max_grad_norm=1.0, backend="kgs")

    class Shim:  # what _check_step reads of a Case
        pass

    shim = Shim()
    shim.opt, shim.params, shim.numels = opt, opt._params, [p.numel() for p in opt._params]
    losses = []
    for step in range(1, 9):
        opt.zero_grad(set_to_none=True)
        loss = lm.loss(tokens, targets)
        loss.backward()
        before = {k: opt._flat[k].clone() for k in KEYS}
        opt.step()
        losses.append(loss.item())
        clip = opt.clip
        # the weights of a tensor without a gradient are not looked at: every parameter has one here
        assert all(p.grad is not None for p in opt._params)
        _check_step(shim, before, step, clip=clip, what=f"lm step {step} (clip {clip:.4f})")
        assert opt.step_count == step and opt.skipped_steps == 0
    print("loss", [f"{v:.4f}" for v in losses])
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[7] < 0.5 * losses[0]
    names = {id(p): n for n, p in lm.named_parameters()}
    norms = [p for p in opt._params if names[id(p)].endswith(("attn_norm", "mlp_norm"))]
    assert len(norms) == 2 * nl
    for p in opt._params:
        assert torch.equal(p.detach(), opt.state[p]["master"].to(BF))
    for p in norms:
        assert (opt.state[p]["master"] != 1.0).all()
