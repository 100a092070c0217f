"""GPU tests of gradient accumulation into fp32 main gradients
(native/kernels/grad_accum.hip) under ``kgs.optim.AdamW(main_grads=True,
backend="kgs")``.

The accumulate kernel is held to bitwise equality with the sequential fp32 sum
computed by torch: one IEEE add per micro-batch has one correct answer. The step
is held to the one-step bounds of tests/test_optim_gpu.py against the float64
reference (``ref_adamw_step``) fed the kernel's own inputs: the fp32 state and the
fp32 main gradients read back before the step, the clip factor the device
computed, and ``s`` (``1 / n`` or 1) as a float64 scale:

* m, v:    ``|out - ref| <= 2^-22 |ref| + 2^-125``
* master:  ``|out - ref| <= 2^-23 |ref| + lr 2^-20 |u_ref| + 2^-125``
* bf16 weight: bitwise the stored master ``.bfloat16()``
* grad_norm^2: within ``(n + 1) 2^-24 sum (s a)^2`` of the float64 sum: the bound of
  an fp32 sum of n terms in any order, plus one rounding of each square (an fp32
  main gradient has 24 significant bits, its square does not fit)

A cycle of one micro-batch must be bit for bit the bf16-gradient step. Each test
prints its least margin."""
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
ALWAYS = "always"


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


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


class Case:
    """Parameters (views into poisoned buffers), an optimizer on them, gradients that
    stay at their addresses (views into poisoned buffers too). ``none_at``: index of a
    tensor (as given) -> the micro-batch numbers in which it has no gradient, or ALWAYS."""

    def __init__(self, numels, seed=0, none_at=None, groups=None, zero_state=lambda i: i % 2 == 1, step0=0, **kw):
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
        self.none_at = {i: (none_at or {}).get(j, ()) for i, p in enumerate(self.params)
                        for j, q in enumerate(made) if p is q}
        self.keys = KEYS + (("main_grad",) if self.opt.main_grads else ())
        # poison the padding of the flat buffers, fill the state
        self.pad = torch.ones(self.opt._flat["master"].numel(), dtype=torch.bool, device=DEV)
        for off, n in zip(self.opt._offsets, self.numels):
            self.pad[off:off + n] = False
        for k in self.keys:
            self.opt._flat[k][self.pad] = POISON
        for i, p in enumerate(self.params):
            st = self.opt.state[p]
            if not zero_state(i):
                st["exp_avg"].copy_(0.1 * torch.randn(p.numel(), device=DEV, generator=g))
                st["exp_avg_sq"].copy_(0.01 * torch.rand(p.numel(), device=DEV, generator=g))
        if step0:
            from kgs.ops.optim import STATE_STEP

            self.opt._state[STATE_STEP] = step0
        self.gviews = [None] * len(self.params)
        self.gbufs = [None] * len(self.params)

    def micro(self, j, special=True, scale=1.0, poke=None):
        """Micro-batch ``j``'s gradients into ``.grad`` (what backward() leaves: the
        buffers keep their addresses); returns clones of them, ``None`` where there is none."""
        out = []
        for i, p in enumerate(self.params):
            if self.none_at[i] == ALWAYS or j in self.none_at[i]:
                p.grad = None
                out.append(None)
                continue
            new = _grad(self.gen, p.numel(), special, scale)
            if poke is not None and i == poke[0]:
                new[poke[1]] = poke[2]
            if self.gviews[i] is None:
                self.gviews[i], self.gbufs[i] = _wide(new)
            else:
                self.gviews[i].copy_(new)
            p.grad = self.gviews[i]
            out.append(new)
        return out

    def cycle(self, k, special=False, scale=1.0, first=0):
        for j in range(first, first + k):
            self.micro(j, special, scale)
            self.opt.accumulate()

    def snapshot(self):
        return {"w": [b.clone() for b in self.wbufs], "g": [None if b is None else b.clone() for b in self.gbufs],
                **{k: self.opt._flat[k].clone() for k in self.keys}, "state": self.opt._state.clone()}

    def borders_intact(self):
        ok = all(_poison_intact(b, n) for b, n in zip(self.wbufs, self.numels))
        ok = ok and all(b is None or _poison_intact(b, n) for b, n in zip(self.gbufs, self.numels))
        return ok and all(bool((self.opt._flat[k][self.pad] == POISON).all()) for k in self.keys)


def _same(a, b, skip=("state", "g")):
    for k in a:
        if k in skip or k not in b:
            continue
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            if (x is None) != (y is None) or (x is not None and not torch.equal(_bits(x), _bits(y))):
                return False
    return True


def _check_step(case, before, step, clip, scale, live, what=""):
    """One main-gradient step of ``case.opt`` against the float64 reference on the
    state and the main gradients ``before`` it (a snapshot); returns the least margins.
    Tensors outside ``live`` (no gradient in the cycle) must be bitwise unchanged."""
    from kgs.ops.optim import ref_adamw_step

    opt = case.opt
    betas, eps = tuple(_f32(b) for b in BETAS), _f32(EPS)
    least = {"m": float("inf"), "v": float("inf"), "p": float("inf")}
    for i, (p, off, n) in enumerate(zip(case.params, opt._offsets, case.numels)):
        st = opt.state[p]
        seg = {k: before[k][off:off + n] for k in KEYS + ("main_grad",)}
        if i not in live:
            for k in KEYS:
                assert torch.equal(st[k].reshape(-1), seg[k]), (what, i, k)
            assert torch.equal(p.detach().reshape(-1), before["w"][i][8:8 + n]), (what, i)
            continue
        grp = opt.param_groups[opt._group_of[i]]
        lr, wd = _f32(grp["lr"]), _f32(grp["weight_decay"])
        rp, rm, rv = ref_adamw_step(seg["master"], seg["exp_avg"], seg["exp_avg_sq"], seg["main_grad"], step, lr,
                                    betas, eps, wd, clip=clip, scale=scale)
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
        assert torch.equal(_bits(p.detach().reshape(-1)), _bits(st["master"].reshape(-1).to(BF))), (what, i)
    print(f"{what}: least margin (share of the bound left) m {least['m']:.3f} v {least['v']:.3f} p {least['p']:.3f}")
    return least


def _norm_check(case, before, scale, live, what):
    """grad_norm^2 against the float64 sum of (scale * main)^2 over the live tensors."""
    from kgs.ops.optim import ref_grad_norm

    mains = [before["main_grad"][off:off + n] for i, (off, n) in enumerate(zip(case.opt._offsets, case.numels))
             if i in live]
    n = sum(a.numel() for a in mains)
    ss = ref_grad_norm(mains, scale=scale).item() ** 2
    got = case.opt.grad_norm
    bound = (n + 1) * 2.0 ** -24 * ss
    print(f"{what}: grad_norm {got:.6e}, |norm^2 - ref| {abs(got * got - ss):.3e}, bound {bound:.3e}")
    assert abs(got * got - ss) <= bound
    return got


def _sizes():
    c = _chunk()
    return [0, 1, 7, 8, 9, 511, 512, 4097, c - 1, c, c + 1, 3 * c + 5, 100]


def _two_groups(n):
    return [(list(range(0, n, 2)), 1e-3, 0.1), (list(range(1, n, 2)), 3e-2, 0.0)]


# ----------------------------------------------------------------------------
# accumulate

def test_accumulate_is_the_sequential_fp32_sum_and_leaves_zeroed_gradients_in_place():
    """Three micro-batches with the special values, two groups, a tensor without a
    gradient throughout (100 elements), one without in the first micro-batch only
    (c + 1) and one without in the second only (511). The main gradients start from
    stale values, which the first micro-batch must overwrite, with zeros where there
    is no gradient."""
    sizes = _sizes()
    n = len(sizes)
    case = Case(sizes, seed=1, none_at={n - 1: ALWAYS, 10: (0,), 5: (1,)}, groups=_two_groups(n), main_grads=True)
    opt = case.opt
    opt._flat["main_grad"][~case.pad] = 7.0
    want = [None] * n
    for j in range(3):
        grads = case.micro(j)
        addr = [None if p.grad is None else p.grad.data_ptr() for p in case.params]
        opt.accumulate()
        torch.cuda.synchronize()
        for i, (p, g) in enumerate(zip(case.params, grads)):
            if j == 0:
                want[i] = torch.zeros(p.numel(), device=DEV) if g is None else g.float()
            elif g is not None:
                want[i] = want[i] + g.float()  # one fp32 add
            assert torch.equal(_bits(opt.main_grad(p).reshape(-1)), _bits(want[i])), (j, i, p.numel())
            if g is not None:
                assert p.grad.data_ptr() == addr[i] and int(_bits(p.grad).count_nonzero()) == 0, (j, i)
        # a gradient that was None this time keeps what it held (zeros, from the micro-batch before)
        assert all(v is None or int(_bits(v).count_nonzero()) == 0 for v in case.gviews)
        assert case.borders_intact(), j
        assert opt.pending_micro_batches == j + 1
    assert opt.table_refreshes == 4  # the main table once, the bf16 table per change of the None set
    # zero_grads=False leaves the gradients alone
    grads = case.micro(3)
    opt.accumulate(zero_grads=False)
    torch.cuda.synchronize()
    for i, (p, g) in enumerate(zip(case.params, grads)):
        if g is not None:
            assert torch.equal(_bits(p.grad), _bits(g))
            assert torch.equal(_bits(opt.main_grad(p).reshape(-1)), _bits(want[i] + g.float()))
    assert case.borders_intact() and opt.pending_micro_batches == 4


# ----------------------------------------------------------------------------
# the step

@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("k", [1, 3])
def test_the_step_is_the_reference_step_on_the_scaled_main_gradient(k, step, average):
    sizes = _sizes()
    n = len(sizes)
    case = Case(sizes, seed=10 * k + step % 7 + average, none_at={n - 1: ALWAYS}, groups=_two_groups(n),
                step0=step - 1, max_grad_norm=0.5, main_grads=True, grad_average=average)
    case.cycle(k)
    live = {i for i in range(n) if case.none_at[i] != ALWAYS}
    before = case.snapshot()
    case.opt.step()
    torch.cuda.synchronize()
    scale = 1.0 / k if average else 1.0
    what = f"{k} micro-batches, step {step}, average {average}"
    norm, clip = _norm_check(case, before, scale, live, what), case.opt.clip
    assert norm > 0.5 and clip < 1.0
    assert abs(clip - 0.5 / (norm + 1e-6)) <= 2.0 ** -22 * clip
    _check_step(case, before, step, clip, scale, live, what=what)
    assert case.borders_intact()
    assert torch.equal(before["main_grad"], case.opt._flat["main_grad"])  # the step reads them only
    assert case.opt.step_count == step and case.opt.skipped_steps == 0 and case.opt.pending_micro_batches == 0


def test_a_cycle_of_one_micro_batch_is_bitwise_the_bf16_route():
    """Same ownership, same order of additions, the same update(): with main =
    float(g) and s = 1 every product is the one the bf16 kernels form."""
    from kgs.ops.optim import STATE_MICRO

    sizes = _sizes()
    n = len(sizes)
    kw = dict(seed=20, none_at={n - 1: ALWAYS}, groups=_two_groups(n), max_grad_norm=1.0)
    old, new = Case(sizes, **kw), Case(sizes, main_grads=True, **kw)
    for step in range(3):
        for case in (old, new):
            case.micro(step, special=step == 2, scale=0.5 + step)
        new.opt.accumulate(zero_grads=False)
        old.opt.step()
        new.opt.step()
        torch.cuda.synchronize()
        a, b = old.snapshot(), new.snapshot()
        assert _same(a, b, skip=("state",)), step
        words = [w for w in range(8) if w != STATE_MICRO]
        assert torch.equal(a["state"][words], b["state"][words]), (step, a["state"], b["state"])
        assert new.opt.clip < 1.0
    assert new.opt.step_count == 3 and new.borders_intact()


def test_a_value_that_is_not_finite_skips_the_step_and_the_next_cycle_is_clean():
    sizes = _sizes()[:-1] + [13]
    case = Case(sizes, seed=30, max_grad_norm=1.0, weight_decay=0.1, main_grads=True)
    opt = case.opt
    live = set(range(len(sizes)))
    case.cycle(1)
    opt.step()
    last = len(sizes) - 1
    for j in range(3):
        case.micro(j, special=False, poke=(last, -1, float("inf")) if j == 1 else None)
        opt.accumulate()
    before = case.snapshot()
    assert opt.pending_micro_batches == 3 and not torch.isfinite(opt.main_grad(case.params[last])).all()
    opt.step()
    torch.cuda.synchronize()
    assert _same(before, case.snapshot(), skip=("state",))
    assert opt.step_count == 1 and opt.skipped_steps == 1 and opt.pending_micro_batches == 0
    assert case.borders_intact()
    want = None
    for j in range(2):
        grads = case.micro(j, special=False)
        opt.accumulate()
        want = [g.float() for g in grads] if want is None else [a + g.float() for a, g in zip(want, grads)]
    torch.cuda.synchronize()
    for p, a in zip(case.params, want):
        assert torch.equal(_bits(opt.main_grad(p).reshape(-1)), _bits(a)) and torch.isfinite(a).all()
    before = case.snapshot()
    opt.step()
    torch.cuda.synchronize()
    assert opt.step_count == 2 and opt.skipped_steps == 1
    _check_step(case, before, 2, opt.clip, 0.5, live, what="the step after a skipped one")
    assert case.borders_intact()


def test_two_fresh_runs_are_bitwise_equal():
    runs = []
    for _ in range(2):
        case = Case(_sizes(), seed=40, max_grad_norm=1.0, weight_decay=0.1, lr=1e-2, main_grads=True)
        for k in (2, 3, 1):
            case.cycle(k)
            case.opt.step()
        torch.cuda.synchronize()
        runs.append(case.snapshot())
    assert _same(runs[0], runs[1], skip=()) and torch.equal(runs[0]["state"], runs[1]["state"])
    assert runs[0]["state"][0].item() == 3


# ----------------------------------------------------------------------------
# graph capture

def test_one_captured_accumulate_and_one_captured_step_replay_cycles_of_any_length():
    from kgs.utils.graph_audit import audit

    sizes = _sizes()
    kw = dict(seed=50, max_grad_norm=1.0, weight_decay=0.1, lr=1e-2, main_grads=True)
    eager, graph = Case(sizes, **kw), Case(sizes, **kw)
    grads = [[_grad(_gen(100 + k), n, special=False) for n in eager.numels] for k in range(6)]

    def load(case, k):
        for p, g in zip(case.params, grads[k]):
            if p.grad is None:
                p.grad = torch.empty_like(g)
            p.grad.copy_(g)

    for case in (eager, graph):  # one eager cycle on both: builds the tables, warms up
        load(case, 0)
        case.opt.accumulate()
        case.opt.step()
    torch.cuda.synchronize()
    refreshes = (graph.opt.table_refreshes, graph.opt.group_refreshes)
    ga, gs = torch.cuda.CUDAGraph(keep_graph=True), torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(ga):
        graph.opt.accumulate()
    with torch.cuda.graph(gs):
        graph.opt.step()
    assert (graph.opt.table_refreshes, graph.opt.group_refreshes) == refreshes == (3, 1)
    for g, launches in ((ga, 2), (gs, 3)):  # accumulate + count; norm pass, finalize, update
        a = audit(g)
        print(a)
        assert a["memsets"] == [] and a["types"].get("kernel", 0) == launches
    assert graph.opt.pending_micro_batches == 0  # a capture runs nothing
    k = 1
    for length in (2, 3):
        if length == 3:  # a new lr, no re-capture
            for case in (eager, graph):
                case.opt.param_groups[0]["lr"] = 5e-3
            assert graph.opt.update_groups()
        for _ in range(length):
            load(eager, k)
            eager.opt.accumulate()
            load(graph, k)
            ga.replay()
            k += 1
        assert graph.opt.pending_micro_batches == length
        eager.opt.step()
        gs.replay()
        torch.cuda.synchronize()
        a, b = eager.snapshot(), graph.snapshot()
        assert _same(a, b, skip=("g",)) and torch.equal(a["state"], b["state"]), length
        assert all(int(_bits(p.grad).count_nonzero()) == 0 for p in graph.params)
    assert graph.opt.step_count == 3 and graph.opt.table_refreshes == 3 and graph.borders_intact()
    # a replayed step with nothing accumulated counts as skipped and changes nothing
    before = graph.snapshot()
    gs.replay()
    torch.cuda.synchronize()
    assert _same(before, graph.snapshot(), skip=("state",))
    assert graph.opt.step_count == 3 and graph.opt.skipped_steps == 1
    # the lr did take effect: a third run that keeps 1e-2 ends elsewhere
    third = Case(sizes, **kw)
    for ks in ((0,), (1, 2), (3, 4, 5)):
        for k in ks:
            load(third, k)
            third.opt.accumulate()
        third.opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(third.snapshot()["master"], graph.snapshot()["master"])


# ----------------------------------------------------------------------------
# raw entries

def test_raw_entries_reject_bad_arguments_and_launch_nothing():
    from kgs.ops import _lib
    from kgs.ops.optim import adamw_table, grad_accum_tables_check

    lib = _lib.lib()
    w = torch.full((32,), POISON, dtype=BF, device=DEV)
    f = [torch.full((32,), POISON, device=DEV) for _ in range(4)]
    g = torch.full((32,), POISON, dtype=BF, device=DEV)
    ghost, nchunks = adamw_table([w], [f[0]], [f[1]], [f[2]], [g], [0], 1, pin=False)
    mhost, mchunks = adamw_table([w], [f[0]], [f[1]], [f[2]], [f[3]], [0], 1, pin=False, grad_dtype=torch.float32)
    assert nchunks == mchunks == 1 and torch.equal(ghost[:, 5:], mhost[:, 5:]) and mhost[0, 4] == f[3].data_ptr()
    grad_accum_tables_check(ghost, mhost)
    check = lib.kgs_grad_accum_table_check
    assert check(ghost.data_ptr(), mhost.data_ptr(), 1) == 0
    for word, value, rc in ((4, 0, -2), (4, f[3].data_ptr() + 4, -2), (5, 31, -1), (6, 1, -1), (7, 1, -1)):
        bad = mhost.clone()
        bad[0, word] = value
        assert check(ghost.data_ptr(), bad.data_ptr(), 1) == rc, (word, value)
    bad = ghost.clone()
    bad[0, 4] += 2
    assert check(bad.data_ptr(), mhost.data_ptr(), 1) == -2
    assert check(0, mhost.data_ptr(), 1) == -1 and check(ghost.data_ptr(), mhost.data_ptr(), -1) == -1
    with pytest.raises(_lib.KernelError):
        grad_accum_tables_check(ghost, bad)
    gt, mt = ghost.to(DEV), mhost.to(DEV)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    groups = torch.tensor([[1e-3, 0.0]], device=DEV)
    parts = torch.full((4,), POISON, device=DEV)
    st = _lib.stream_handle(w.device)
    G, M, S, R, P = gt.data_ptr(), mt.data_ptr(), state.data_ptr(), groups.data_ptr(), parts.data_ptr()
    acc = lib.kgs_grad_accumulate
    assert acc(G + 8, M, 1, 1, S, 1, st) == -2 and acc(G, M + 8, 1, 1, S, 1, st) == -2
    assert acc(0, M, 1, 1, S, 1, st) == -2 and acc(G, 0, 1, 1, S, 0, st) == -2
    assert acc(G, M, 1, 1, S + 4, 1, st) == -2 and acc(G, M, 1, 1, 0, 1, st) == -2
    assert acc(G, M, 1, -1, S, 1, st) == -1 and acc(G, M, 0, 1, S, 1, st) == -1 and acc(G, M, -1, 0, S, 1, st) == -1
    assert lib.kgs_main_sumsq(M + 8, 1, 1, P, st) == -2 and lib.kgs_main_sumsq(0, 1, 1, P, st) == -2
    assert lib.kgs_main_sumsq(M, 1, 1, 0, st) == -2 and lib.kgs_main_sumsq(M, 1, 1, P + 2, st) == -2
    assert lib.kgs_main_sumsq(M, 1, -1, P, st) == -1 and lib.kgs_main_sumsq(M, 0, 1, P, st) == -1
    assert lib.kgs_main_sumsq(M, 1, 0, P, st) == 0  # nothing to do, nothing launched
    fin = lib.kgs_main_finalize
    assert fin(P, 1, 1.0, 0.9, 0.95, 1, S + 4, st) == -2 and fin(P, 1, 1.0, 0.9, 0.95, 1, 0, st) == -2
    assert fin(0, 1, 1.0, 0.9, 0.95, 1, S, st) == -2 and fin(P, -1, 1.0, 0.9, 0.95, 1, S, st) == -1
    assert fin(P, 1, 0.0, 0.9, 0.95, 1, S, st) == -3 and fin(P, 1, 1.0, 1.0, 0.95, 1, S, st) == -3
    step = lib.kgs_adamw_step_main
    assert step(M + 8, 1, 1, R, S, 0.9, 0.95, 1e-8, 1, st) == -2 and step(0, 1, 1, R, S, 0.9, 0.95, 1e-8, 1, st) == -2
    assert step(M, 1, 1, R + 4, S, 0.9, 0.95, 1e-8, 1, st) == -2 and step(M, 1, 1, R, S + 4, 0.9, 0.95, 1e-8, 1, st) == -2
    assert step(M, 1, 1, R, S, 0.9, 0.95, -1.0, 1, st) == -3 and step(M, 1, 1, R, S, 0.9, 1.0, 1e-8, 1, st) == -3
    assert step(M, 1, -1, R, S, 0.9, 0.95, 1e-8, 1, st) == -1
    assert step(M, 1, 0, R, S, 0.9, 0.95, 1e-8, 1, st) == 0  # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert (w == POISON).all() and (g == POISON).all() and all((t == POISON).all() for t in f)
    assert (parts == POISON).all() and int(state.count_nonzero()) == 0


# ----------------------------------------------------------------------------
# DecoderLM, end to end

def test_decoder_lm_trains_from_two_micro_batches_per_step():
    """Four clipped AdamW steps of the small DecoderLM of tests/test_optim_gpu.py, its
    batch of 2 x 128 split into two micro-batches of 1 x 128: every step's main
    gradients are bitwise the fp32 sum of the two micro-batches' bf16 gradients, every
    step is within the one-step bounds of the float64 reference, the weights are the
    rounded masters, and the loss falls."""
    from kgs.models.decoder import DecoderLM
    from kgs.optim import AdamW, decay_groups

    vocab, dim, nl, nh, nkv, inter, b, s = 1024, 512, 2, 4, 1, 1536, 2, 128
    g = _gen(11)
    tokens = torch.randint(0, vocab, (b, s), device=DEV, generator=g)
    targets = tokens.roll(-1, 1).clone()
    targets[:, -1] = -100
    lm = DecoderLM(vocab, dim, nl, nh, nkv, inter, backend="kgs", device=DEV)
    opt = AdamW(decay_groups(lm, 0.1), lr=1e-3, betas=BETAS, eps=EPS, max_grad_norm=1.0, backend="kgs",
                main_grads=True)

    class Shim:  # what _check_step and _norm_check read of a Case
        pass

    shim = Shim()
    shim.opt, shim.params, shim.numels = opt, opt._params, [p.numel() for p in opt._params]
    live = set(range(len(opt._params)))
    losses = []
    for step in range(1, 5):
        seen, loss = [], 0.0
        for mb in range(b):
            part = lm.loss(tokens[mb:mb + 1], targets[mb:mb + 1])
            part.backward()
            seen.append([p.grad.clone() for p in opt._params])
            opt.accumulate()
            loss += part.item() / b
        assert opt.pending_micro_batches == b
        for p, g0, g1 in zip(opt._params, *seen):
            assert g0.dtype == BF and torch.equal(_bits(opt.main_grad(p)), _bits(g0.float() + g1.float()))
            assert int(_bits(p.grad).count_nonzero()) == 0
        before = {k: opt._flat[k].clone() for k in KEYS + ("main_grad",)}
        opt.step()
        losses.append(loss)
        clip = opt.clip
        what = f"lm step {step} (clip {clip:.4f})"
        _norm_check(shim, before, 1.0 / b, live, what)
        _check_step(shim, before, step, clip, 1.0 / b, live, what=what)
        assert opt.step_count == step and opt.skipped_steps == 0
    print("loss", [f"{v:.4f}" for v in losses])
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]
    for p in opt._params:
        assert torch.equal(p.detach(), opt.state[p]["master"].to(BF))
