"""CPU tests of the optimizer (the kernels themselves: tests/test_optim_gpu.py): the
float64 references against torch, ``kgs.optim.AdamW(backend="torch")`` (the
kernels' algorithm in torch ops: groups, skipped tensors, skipped steps, master
weights, checkpoints, schedulers), the argument checks of the raw ops, which raise
before the native library is touched, and the kernels' compile-time resources."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import kgs.optim
from kgs.ops.optim import (ROW_WORDS, STATE_WORDS, adamw_step_, adamw_table, grad_norm, ref_adamw_step, ref_clip,
                           ref_grad_norm)
from kgs.optim import AdamW, decay_groups

F64 = torch.float64
BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------
# references

def test_ref_adamw_step_is_torchs_adamw_in_float64():
    g = _gen(1)
    lr, betas, eps, wd = 3e-3, (0.9, 0.95), 1e-8, 0.1
    p = torch.randn(257, generator=g, dtype=F64)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 6):
        q.grad = torch.randn(257, generator=g, dtype=F64)
        p, m, v = ref_adamw_step(p, m, v, q.grad, step, lr, betas, eps, wd)
        opt.step()
        st = opt.state[q]
        for got, want in ((p, q.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert got.dtype == F64 and (got - want).abs().max().item() <= 1e-12
    # clip scales the gradient, nothing else
    a = ref_adamw_step(p, m, v, q.grad, 6, lr, betas, eps, wd, clip=0.25)
    b = ref_adamw_step(p, m, v, 0.25 * q.grad, 6, lr, betas, eps, wd)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("max_norm", [0.5, 1e3])
def test_ref_grad_norm_and_clip_are_clip_grad_norms(max_norm):
    g = _gen(2)
    ps = [torch.zeros(n, dtype=F64).requires_grad_(True) for n in (1, 7, 300)] + [torch.zeros(3, dtype=F64)]
    for p in ps[:3]:
        p.grad = torch.randn(p.shape, generator=g, dtype=F64)
    before = [p.grad.clone() for p in ps[:3]]
    norm = ref_grad_norm([p.grad for p in ps])  # the None entry does not count
    want = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(norm.item() - want.item()) <= 1e-12 * want.item()
    clip = ref_clip(norm, max_norm)
    assert clip.item() <= 1.0 and (clip.item() == 1.0) == (max_norm > norm.item())
    for p, b in zip(ps[:3], before):
        assert (p.grad - clip * b).abs().max().item() <= 1e-12


# ----------------------------------------------------------------------------
# AdamW(backend="torch")

def _params(seed=3, sizes=(5, 64, 130, 9)):
    g = _gen(seed)
    return [torch.randn(n, generator=g).to(BF).requires_grad_(True) for n in sizes]


def _set_grads(ps, seed, skip=()):
    g = _gen(seed)
    for i, p in enumerate(ps):
        gr = torch.randn(p.shape, generator=g).to(BF)
        p.grad = None if i in skip else gr


def _buffers(opt, ps):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [opt.state[p][k].clone() for k in ("master", "exp_avg", "exp_avg_sq")]
    return out


def _same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def test_torch_backend_honours_groups_and_follows_the_reference():
    ps = _params()
    groups = [{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.1}, {"params": ps[2:], "lr": 1e-3, "weight_decay": 0.0}]
    opt = AdamW(groups, betas=(0.9, 0.95), eps=1e-8, backend="torch")
    ref = [(p.detach().double(), torch.zeros_like(p, dtype=F64), torch.zeros_like(p, dtype=F64)) for p in ps]
    for step in (1, 2, 3):
        _set_grads(ps, 10 + step)
        opt.step()
        for i, p in enumerate(ps):
            lr, wd = (1e-2, 0.1) if i < 2 else (1e-3, 0.0)
            ref[i] = ref_adamw_step(*ref[i], p.grad, step, lr, (0.9, 0.95), 1e-8, wd)
            st = opt.state[p]
            assert st["master"].dtype == torch.float32 and p.dtype == BF
            for got, want in zip((st["master"], st["exp_avg"], st["exp_avg_sq"]), ref[i]):
                torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-7)
            assert torch.equal(p.detach(), st["master"].to(BF))
    assert opt.step_count == 3 and opt.skipped_steps == 0 and opt.grad_norm is None and opt.clip == 1.0


def test_flat_state_segments_start_on_64_element_boundaries():
    ps = _params(sizes=(5, 64, 130, 9))
    opt = AdamW(ps, backend="torch")
    assert opt._offsets == [0, 64, 128, 320]
    for p, off in zip(ps, opt._offsets):
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert opt.state[p][k].data_ptr() == opt._flat[k].data_ptr() + 4 * off
        assert torch.equal(opt.state[p]["master"], p.detach().float())  # exactly the bf16 weights


def test_a_none_gradient_leaves_that_tensor_alone():
    ps = _params()
    opt = AdamW(ps, lr=1e-2, backend="torch")
    _set_grads(ps, 20)
    opt.step()
    before = _buffers(opt, ps)
    _set_grads(ps, 21, skip=(1,))
    opt.step()
    after = _buffers(opt, ps)
    n = len(ps)
    for i in range(n):
        mine = [before[i]] + before[n + 3 * i:n + 3 * i + 3], [after[i]] + after[n + 3 * i:n + 3 * i + 3]
        assert _same(*mine) == (i == 1), i
    assert opt.step_count == 2


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_gradient_that_is_not_finite_skips_the_whole_step(bad):
    ps = _params()
    opt = AdamW(ps, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0, backend="torch")
    _set_grads(ps, 30)
    opt.step()
    before, clip = _buffers(opt, ps), opt.clip
    _set_grads(ps, 31)
    ps[-1].grad[-1] = bad
    opt.step()
    assert _same(before, _buffers(opt, ps))
    assert opt.step_count == 1 and opt.skipped_steps == 1 and opt.clip == clip
    _set_grads(ps, 32)
    opt.step()  # the next clean step is step number 2
    assert opt.step_count == 2 and opt.skipped_steps == 1 and not _same(before, _buffers(opt, ps))
    twin = _params()
    other = AdamW(twin, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0, backend="torch")
    for seed in (30, 32):
        _set_grads(twin, seed)
        other.step()
    assert _same(_buffers(opt, ps), _buffers(other, twin))


def test_clipping_scales_the_step_and_without_it_there_is_no_norm_pass(monkeypatch):
    calls = []
    real = kgs.optim._sumsq
    monkeypatch.setattr(kgs.optim, "_sumsq", lambda grads: calls.append(len(grads)) or real(grads))
    ps, qs = _params(), _params()
    plain, clipped = AdamW(ps, lr=1e-2, backend="torch"), AdamW(qs, lr=1e-2, max_grad_norm=0.5, backend="torch")
    _set_grads(ps, 40)
    plain.step()
    assert calls == [] and plain.grad_norm is None
    _set_grads(qs, 40)
    clipped.step()
    assert calls == [4]
    norm = ref_grad_norm([q.grad for q in qs]).item()
    assert norm > 0.5 and abs(clipped.grad_norm - norm) <= 1e-6 * norm
    assert abs(clipped.clip - 0.5 / (norm + 1e-6)) <= 1e-6
    for q in qs:
        zero = torch.zeros_like(q, dtype=F64)  # the first step: m = (1 - b1) clip g
        want = ref_adamw_step(zero, zero, zero, q.grad, 1, 1e-2, (0.9, 0.95), 1e-8, 0.0, clip=clipped.clip)
        torch.testing.assert_close(clipped.state[q]["exp_avg"].double(), want[1], rtol=1e-5, atol=1e-9)
    # without clipping an inf is not looked for: the step is taken
    ps[0].grad[0] = float("inf")
    plain.step()
    assert plain.step_count == 2 and plain.skipped_steps == 0 and calls == [4]


def test_master_weights_move_a_bf16_weight_that_torch_adamw_cannot():
    """A bf16 weight of 1.0, constant gradient +1, lr 1e-3: AdamW's update is -lr per
    step. 1 - 0.001 rounds back to 1.0 in bf16 (the spacing below 1 is 2^-8), so
    torch.optim.AdamW on the bf16 tensor never moves; the fp32 master does, and after
    8 steps it is 0.992, which rounds to 0.9921875."""
    w = torch.ones(16, dtype=BF).requires_grad_(True)
    opt = AdamW([w], lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0, backend="torch")
    stock_w = torch.ones(16, dtype=BF).requires_grad_(True)
    stock = torch.optim.AdamW([stock_w], lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0)
    ref = (torch.ones(16, dtype=F64), torch.zeros(16, dtype=F64), torch.zeros(16, dtype=F64))
    for step in range(1, 9):
        w.grad = torch.ones(16, dtype=BF)
        stock_w.grad = torch.ones(16, dtype=BF)
        opt.step()
        stock.step()
        ref = ref_adamw_step(*ref, w.grad, step, 1e-3, (0.9, 0.95), 1e-8, 0.0)
        if step == 1:
            assert (w.detach() == 1.0).all() and (opt.state[w]["master"] < 1.0).all()
    assert torch.equal(ref[0].to(BF), torch.full((16,), 0.9921875, dtype=BF))
    assert torch.equal(w.detach(), opt.state[w]["master"].to(BF))
    assert (w.detach() == 0.9921875).all()
    assert (stock_w.detach() == 1.0).all()  # what this optimizer exists to fix


def test_state_dict_round_trip_continues_bitwise():
    ps, qs = _params(), _params()
    kw = dict(lr=1e-2, weight_decay=0.1, max_grad_norm=1.0, backend="torch")
    opt = AdamW([{"params": ps[:2]}, {"params": ps[2:], "lr": 3e-3}], **kw)
    for seed in (50, 51):
        _set_grads(ps, seed)
        opt.step()
    sd = opt.state_dict()
    assert set(sd["state"]) == {0, 1, 2, 3}
    for s in sd["state"].values():
        assert set(s) == {"step", "exp_avg", "exp_avg_sq", "master"}
        assert all(t.dtype == torch.float32 for t in s.values()) and float(s["step"]) == 2.0
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    fresh = AdamW([{"params": qs[:2]}, {"params": qs[2:]}], lr=7.0, backend="torch", max_grad_norm=1.0)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[1]["lr"] == 3e-3 and fresh.param_groups[0]["weight_decay"] == 0.1
    assert fresh.step_count == 2
    for o, xs in ((opt, ps), (fresh, qs)):
        _set_grads(xs, 52)
        o.step()
    assert _same(_buffers(opt, ps), _buffers(fresh, qs)) and fresh.step_count == 3


def test_a_torch_adamw_state_loads_and_takes_the_masters_from_the_parameters():
    g = _gen(60)
    fp = [torch.randn(n, generator=g).requires_grad_(True) for n in (5, 70)]
    stock = torch.optim.AdamW(fp, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)
    for _ in range(2):
        for p in fp:
            p.grad = torch.randn(p.shape, generator=g)
        stock.step()
    ps = [p.detach().to(BF).requires_grad_(True) for p in fp]
    opt = AdamW(ps, backend="torch")
    opt.load_state_dict(stock.state_dict())
    assert opt.step_count == 2 and opt.param_groups[0]["lr"] == 1e-2 and opt.param_groups[0]["weight_decay"] == 0.1
    for p, f in zip(ps, fp):
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], stock.state[f]["exp_avg"]) and st["exp_avg"].dtype == torch.float32
        assert torch.equal(st["exp_avg_sq"], stock.state[f]["exp_avg_sq"])
        assert torch.equal(st["master"], p.detach().float())


def test_an_lr_scheduler_sets_the_lr_of_the_next_step():
    w = torch.ones(8, dtype=BF).requires_grad_(True)
    opt = AdamW([w], lr=1e-2, betas=(0.9, 0.95), backend="torch")
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.5 ** epoch)
    ref = (torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(8, dtype=F64))
    for step in (1, 2, 3):
        w.grad = torch.ones(8, dtype=BF)
        opt.step()
        ref = ref_adamw_step(*ref, w.grad, step, 1e-2 * 0.5 ** (step - 1), (0.9, 0.95), 1e-8, 0.0)
        sched.step()
        torch.testing.assert_close(opt.state[w]["master"].double(), ref[0], rtol=1e-6, atol=0)
    assert opt.group_refreshes == 3  # uploaded when it changed, not otherwise
    w.grad = torch.zeros(8, dtype=BF)
    opt.param_groups[0]["lr"] = opt.param_groups[0]["lr"]
    assert opt.update_groups() is True and opt.update_groups() is False


def test_the_optimizer_rejects_what_it_cannot_run():
    w = torch.ones(8, dtype=BF).requires_grad_(True)
    f = torch.ones(8).requires_grad_(True)
    with pytest.raises(ValueError):
        AdamW([{"params": [w]}, {"params": [f], "betas": (0.8, 0.9)}], backend="torch")
    with pytest.raises(ValueError):
        AdamW([{"params": [w]}, {"params": [f], "eps": 1e-6}], backend="torch")
    with pytest.raises(ValueError):
        AdamW([w], amsgrad=True, backend="torch")
    with pytest.raises(ValueError):
        AdamW([w], maximize=True, backend="torch")
    with pytest.raises(ValueError, match="bf16"):
        AdamW([f], backend="kgs")
    with pytest.raises(ValueError):
        AdamW([w], backend="jax")
    with pytest.raises(ValueError):
        AdamW([w], max_grad_norm=0.0, backend="torch")


# ----------------------------------------------------------------------------
# argument checks: raised before the native library is loaded (there is no GPU here)

@pytest.fixture
def no_native(monkeypatch):
    from kgs.ops import _lib

    def boom():
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(_lib, "lib", boom)


def test_adamw_table_checks_its_arguments(no_native):
    w, f = torch.zeros(16, dtype=BF), torch.zeros(16)

    def table(w=w, p=f, m=f, v=f, g=w, group=0, ngroups=1):
        return adamw_table([w], [p], [m], [v], [g], [group], ngroups)

    with pytest.raises(TypeError):
        table(w=f)
    with pytest.raises(TypeError):
        table(p=w)
    with pytest.raises(TypeError):
        table(m=f.double())
    with pytest.raises(TypeError):
        table(v=w)
    with pytest.raises(TypeError):
        table(g=f)
    with pytest.raises(ValueError, match="contiguous"):
        table(w=torch.zeros(32, dtype=BF)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        table(g=torch.zeros(32, dtype=BF)[::2])
    with pytest.raises(ValueError, match="16 elements"):
        table(p=torch.zeros(17))
    with pytest.raises(ValueError, match="16 elements"):
        table(g=torch.zeros(8, dtype=BF))
    with pytest.raises(ValueError, match="group_index"):
        table(group=1)
    with pytest.raises(ValueError):
        adamw_table([w, w], [f], [f], [f], [w], [0], 1)
    with pytest.raises(ValueError):
        adamw_table([], [], [], [], [], [], 1)
    with pytest.raises(ValueError, match="GPU"):
        table()
    with pytest.raises(ValueError, match="GPU"):
        table(g=None)


def test_step_ops_check_their_arguments(no_native):
    table = torch.zeros((2, ROW_WORDS), dtype=torch.int64)
    state = torch.zeros(STATE_WORDS, dtype=torch.int32)
    groups, parts = torch.zeros((1, 2)), torch.zeros(8)
    b = (0.9, 0.95)
    for fn in (lambda t, s: grad_norm(t, 4, s, b, partials=parts, max_norm=1.0),
               lambda t, s: adamw_step_(t, 4, groups, s, b, 1e-8)):
        with pytest.raises(TypeError):
            fn(table.int(), state)
        with pytest.raises(TypeError):
            fn(table, state.float())
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 7), dtype=torch.int64), state)
        with pytest.raises(ValueError):
            fn(table, torch.zeros(4, dtype=torch.int32))
        with pytest.raises(ValueError, match="GPU"):
            fn(table, state)
    with pytest.raises(TypeError):
        grad_norm(table, 4, state, b, partials=parts.double(), max_norm=1.0)
    with pytest.raises(ValueError, match="per chunk"):
        grad_norm(table, 9, state, b, partials=parts, max_norm=1.0)
    with pytest.raises(TypeError):
        adamw_step_(table, 4, groups.double(), state, b, 1e-8)
    with pytest.raises(ValueError):
        adamw_step_(table, 4, torch.zeros(2), state, b, 1e-8)
    with pytest.raises(ValueError, match="GPU"):
        grad_norm(table, 4, state, b)  # no clipping: still a launch


def test_decay_groups_puts_exactly_the_norm_weights_in_the_no_decay_group():
    from kgs.models.decoder import DecoderLM

    lm = DecoderLM(48, 64, 2, 4, 2, 96, backend="torch", dtype=torch.float32)
    decayed, rest = decay_groups(lm, 0.1)
    assert decayed["weight_decay"] == 0.1 and rest["weight_decay"] == 0.0
    names = {id(p): n for n, p in lm.named_parameters()}
    assert sorted(names[id(p)] for p in rest["params"]) == sorted(n for n in names.values() if n.endswith("norm"))
    assert len(rest["params"]) == 2 * 2 + 1
    assert len(decayed["params"]) + len(rest["params"]) == len(names)
    assert all(p.ndim >= 2 for p in decayed["params"])
    opt = AdamW(decay_groups(lm, 0.1), backend="torch")  # the groups are what the optimizer takes
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0]


def test_ops_are_exported_from_kgs_ops():
    import kgs.ops

    for name in ("adamw_table", "adamw_step_", "grad_norm", "adamw_chunk", "ref_adamw_step", "ref_grad_norm",
                 "ref_clip"):
        assert callable(getattr(kgs.ops, name))


# ----------------------------------------------------------------------------
# compile-time resources (hipcc cross-compiles gfx950 without a GPU)

@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_optimizer_kernels_use_no_scratch(tmp_path):
    """A pure HBM stream: no kernel may spill or touch scratch, and the file's kernels
    are the ones it declares (KERNEL_COUNT)."""
    root = Path(__file__).resolve().parents[1]
    src = root / "native/kernels/optimizer.hip"
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", str(root / "native/kernels"),
                          str(src), "-o", str(tmp_path / "optimizer.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=600, cwd=tmp_path)
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
    declared = int(re.search(r"constexpr int KERNEL_COUNT = (\d+);", src.read_text()).group(1))
    assert len(res) == declared, sorted(res)
    assert sum("adamw_step" in n for n in res) == 6 and sum("grad_sumsq" in n for n in res) == 2
    assert all("ScratchSize" in r and "VGPRs Spill" in r and "VGPRs" in r for r in res.values()), res
    bad = {n: r for n, r in res.items() if r["ScratchSize"] or r["VGPRs Spill"]}
    assert not bad, bad
    two = [r for n, r in res.items() if "adamw_step" in n and "Li2E" in n]
    assert len(two) == 4 and all(r["VGPRs"] <= 128 for r in two), two  # the default: four waves per SIMD
