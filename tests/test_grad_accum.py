"""CPU tests of gradient accumulation into fp32 main gradients (the kernels
themselves: tests/test_grad_accum_gpu.py): ``kgs.optim.AdamW(main_grads=True,
backend="torch")``, which is the kernels' bookkeeping in torch ops, the argument
checks that raise before the native library is touched, the kernels' compile-time
resources, and the measurement that motivates the feature."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from kgs.ops.optim import STATE_MICRO, adamw_table, ref_adamw_step, ref_grad_accumulate, ref_grad_norm
from kgs.optim import AdamW

F64 = torch.float64
BF = torch.bfloat16
SIZES = (5, 64, 130, 9)
KW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, backend="torch")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _params(seed=3, dtype=BF):
    g = _gen(seed)
    return [torch.randn(n, generator=g).to(BF).to(dtype).requires_grad_(True) for n in SIZES]


def _grads(seed, none=()):
    g = _gen(seed)
    out = [torch.randn(n, generator=g).to(BF) for n in SIZES]
    return [None if i in none else x for i, x in enumerate(out)]


def _load(ps, grads):
    """What backward() does: allocates a missing .grad, adds into an existing one."""
    for p, g in zip(ps, grads):
        if g is None:
            continue
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.add_(g)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _buffers(opt, ps):
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps
                                               for k in ("master", "exp_avg", "exp_avg_sq")]


def _twin_step(opt_kw, state_of, grads):
    """The existing torch-backend step on fp32 copies of the parameters, fed ``grads``
    (fp32, ``None`` for a tensor without one) and started from the state ``state_of``
    gives: ``(master, exp_avg, exp_avg_sq)`` per tensor after the step, and the optimizer."""
    qs = [m.clone().requires_grad_(True) for m, _, _ in state_of]
    twin = AdamW(qs, **opt_kw)
    for q, (m, a, b) in zip(qs, state_of):
        twin.state[q]["exp_avg"].copy_(a)
        twin.state[q]["exp_avg_sq"].copy_(b)
    twin._state[:7].copy_(state_of.block[:7])  # step count, bias corrections, clip
    for q, g in zip(qs, grads):
        q.grad = g
    twin.step()
    return [(twin.state[q]["master"], twin.state[q]["exp_avg"], twin.state[q]["exp_avg_sq"]) for q in qs], twin


class _State(list):
    block = None


def _state_of(opt, ps):
    out = _State((opt.state[p]["master"].clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                 for p in ps)
    out.block = opt._state.clone()
    return out


# ----------------------------------------------------------------------------
# the torch backend

@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_main_grads_are_the_sequential_fp32_sum_and_the_step_is_the_old_step_on_the_scaled_sum(k, average):
    ps = _params()
    opt = AdamW(ps, max_grad_norm=0.5, main_grads=True, grad_average=average, **KW)
    for cycle in range(2):  # the second cycle starts from moments that are not zero, at step 2
        want, addr = None, None
        for j in range(k):
            grads = _grads(100 * cycle + j)
            _load(ps, grads)
            if addr is None:
                addr = [p.grad.data_ptr() for p in ps]
            opt.accumulate()
            if want is None:
                want = [g.float() for g in grads]
            else:
                for a, g in zip(want, grads):
                    a += g.float()
            assert opt.pending_micro_batches == j + 1
            for p, a, at in zip(ps, want, addr):
                assert _same(opt.main_grad(p), a) and opt.main_grad(p).dtype == torch.float32
                assert p.grad.data_ptr() == at and p.grad.dtype == BF and int(_bits(p.grad).count_nonzero()) == 0
        before = _state_of(opt, ps)
        s = torch.tensor(1.0) / torch.tensor(float(k)) if average else torch.tensor(1.0)
        after, twin = _twin_step(dict(max_grad_norm=0.5, **KW), before, [s * a for a in want])
        opt.step()
        assert opt.step_count == cycle + 1 and opt.skipped_steps == 0 and opt.pending_micro_batches == 0
        assert opt.grad_norm == twin.grad_norm and opt.clip == twin.clip and opt.clip < 1.0
        norm = ref_grad_norm(want, scale=s.item()).item()
        assert abs(opt.grad_norm - norm) <= 1e-6 * norm
        for p, (m, a, b) in zip(ps, after):
            st = opt.state[p]
            assert _same(st["master"], m) and _same(st["exp_avg"], a) and _same(st["exp_avg_sq"], b)
            assert _same(p.detach(), st["master"].to(BF))
    # the scaled fp32 gradient is what the formulas see: float64 on the last cycle's inputs
    for p, g, (m0, a0, b0) in zip(ps, want, before):
        rp, rm, rv = ref_adamw_step(m0, a0, b0, g, 2, 1e-2, (0.9, 0.95), 1e-8, 0.1, clip=opt.clip, scale=s.item())
        st = opt.state[p]
        for got, ref in ((st["master"], rp), (st["exp_avg"], rm), (st["exp_avg_sq"], rv)):
            torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-7)


def test_ref_grad_accumulate_states_the_two_cases():
    a, g = torch.randn(9, generator=_gen(1)), torch.randn(9, generator=_gen(2)).to(BF)
    assert torch.equal(ref_grad_accumulate(a, g, True), g.double())
    assert torch.equal(ref_grad_accumulate(a, g, False), a.double() + g.double())
    assert torch.equal(ref_grad_accumulate(a, None, True), torch.zeros(9, dtype=F64))
    assert torch.equal(ref_grad_accumulate(a, None, False), a.double())
    assert ref_grad_accumulate(a, g, False).dtype == F64


def test_a_parameter_without_a_gradient_in_some_or_all_micro_batches():
    """Tensor 0 never has a gradient: untouched by the step. Tensor 1 has none in the
    first micro-batch only, tensor 2 none in the second only: their main gradients
    are the sums of what there was, and the stale sum of the cycle before is gone."""
    ps = _params()
    opt = AdamW(ps, main_grads=True, **KW)
    for p in ps:  # stale values that a first micro-batch must overwrite
        opt.main_grad(p).fill_(7.0)
    g0, g1 = _grads(1, none=(0, 1)), _grads(2, none=(0, 2))
    _load(ps, g0)
    opt.accumulate()
    assert int(opt.main_grad(ps[0]).count_nonzero()) == 0 and int(opt.main_grad(ps[1]).count_nonzero()) == 0
    assert _same(opt.main_grad(ps[2]), g0[2].float())
    ps[2].grad = None  # no gradient in the second micro-batch
    _load(ps, g1)
    opt.accumulate()
    want = [torch.zeros(SIZES[0]), g1[1].float(), g0[2].float(), g0[3].float() + g1[3].float()]
    for p, a in zip(ps, want):
        assert _same(opt.main_grad(p), a)
    before = _buffers(opt, ps)
    state = _state_of(opt, ps)
    after, _ = _twin_step(KW, state, [None] + [0.5 * a for a in want[1:]])
    opt.step()
    now = _buffers(opt, ps)
    n = len(ps)
    assert all(_same(now[j], before[j]) for j in [0, n, n + 1, n + 2])  # tensor 0: weight, master, moments
    for p, (m, a, b) in list(zip(ps, after))[1:]:
        st = opt.state[p]
        assert _same(st["master"], m) and _same(st["exp_avg"], a) and _same(st["exp_avg_sq"], b)
    assert not _same(now[n + 3], before[n + 3])  # tensor 1's master did move
    # the next cycle gives tensor 0 a gradient and tensor 3 none
    _load(ps, _grads(3, none=(3,)))
    ps[3].grad = None
    opt.accumulate()
    before = _buffers(opt, ps)
    opt.step()
    now = _buffers(opt, ps)
    assert not _same(now[n], before[n]) and _same(now[n + 9], before[n + 9]) and _same(now[3], before[3])
    assert opt.step_count == 2


def test_a_value_that_is_not_finite_skips_the_step_and_does_not_survive_the_cycle():
    ps = _params()
    opt = AdamW(ps, max_grad_norm=1.0, main_grads=True, **KW)
    _load(ps, _grads(10))
    opt.accumulate()
    opt.step()  # step 1, so that the moments are not zero
    before = _buffers(opt, ps)
    clip = opt.clip
    for j in range(3):
        _load(ps, _grads(20 + j))
        if j == 1:
            ps[-1].grad[-1] = float("inf")
        opt.accumulate()
    assert opt.pending_micro_batches == 3 and not torch.isfinite(opt.main_grad(ps[-1])).all()
    opt.step()
    assert all(_same(a, b) for a, b in zip(before, _buffers(opt, ps)))
    assert opt.step_count == 1 and opt.skipped_steps == 1 and opt.clip == clip and opt.pending_micro_batches == 0
    want = []
    for j in range(2):
        grads = _grads(30 + j)
        _load(ps, grads)
        opt.accumulate()
        want = [g.float() if not j else a + g.float() for a, g in zip(want or grads, grads)]
    assert all(torch.isfinite(opt.main_grad(p)).all() and _same(opt.main_grad(p), a) for p, a in zip(ps, want))
    state = _state_of(opt, ps)
    after, twin = _twin_step(dict(max_grad_norm=1.0, **KW), state, [0.5 * a for a in want])
    opt.step()
    assert opt.step_count == 2 and opt.skipped_steps == 1 and twin.step_count == 2
    for p, (m, a, b) in zip(ps, after):
        st = opt.state[p]
        assert _same(st["master"], m) and _same(st["exp_avg"], a) and _same(st["exp_avg_sq"], b)


def test_nothing_changes_without_main_grads_and_checkpoints_do_not_carry_them():
    ps, qs = _params(), _params()
    old, new = AdamW(ps, max_grad_norm=1.0, **KW), AdamW(qs, max_grad_norm=1.0, main_grads=False, **KW)
    assert "main_grad" not in new._flat and set(new._flat) == set(old._flat)
    opt = AdamW(_params(), main_grads=True, **KW)
    assert opt._flat["main_grad"].dtype == torch.float32
    assert opt._flat["main_grad"].shape == opt._flat["master"].shape
    for p, off in zip(opt._params, opt._offsets):
        assert opt.main_grad(p).data_ptr() == opt._flat["main_grad"].data_ptr() + 4 * off and off % 64 == 0
    _load(opt._params, _grads(1))
    opt.accumulate()
    sd = opt.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq", "master"} for s in sd["state"].values())
    opt.load_state_dict(sd)  # resets the cycle
    assert opt.pending_micro_batches == 0
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        opt.step()


# ----------------------------------------------------------------------------
# argument checks

def test_accumulate_and_step_reject_what_they_cannot_do():
    ps = _params()
    plain = AdamW(ps, **KW)
    _load(ps, _grads(1))
    with pytest.raises(RuntimeError, match="main_grads"):
        plain.accumulate()
    with pytest.raises(RuntimeError, match="main_grads"):
        plain.main_grad(ps[0])
    opt = AdamW(_params(), main_grads=True, **KW)
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        opt.step()
    _load(opt._params, _grads(1))
    opt.accumulate()
    opt.step()
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        opt.step()
    assert opt.step_count == 1 and int(opt._state[STATE_MICRO]) == -1


@pytest.fixture
def no_native(monkeypatch):
    from kgs.ops import _lib

    def boom():
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(_lib, "lib", boom)


def test_the_raw_ops_check_dtypes_before_any_device(no_native):
    from kgs.ops.optim import ROW_WORDS, STATE_WORDS, adamw_step_, grad_accum_tables_check, grad_accumulate_, grad_norm

    w, f = torch.zeros(16, dtype=BF), torch.zeros(16)

    def table(g, dtype):
        return adamw_table([w], [f], [f], [f], [g], [0], 1, grad_dtype=dtype)

    with pytest.raises(TypeError):
        table(w, torch.float32)  # a bf16 gradient in the main table
    with pytest.raises(TypeError):
        table(f, torch.bfloat16)  # and the reverse
    with pytest.raises(TypeError):
        table(f, torch.float16)
    with pytest.raises(ValueError, match="16 elements"):
        table(torch.zeros(8), torch.float32)
    with pytest.raises(ValueError, match="GPU"):
        table(f, torch.float32)
    tbl = torch.zeros((2, ROW_WORDS), dtype=torch.int64)
    state = torch.zeros(STATE_WORDS, dtype=torch.int32)
    with pytest.raises(TypeError):
        grad_accumulate_(tbl.int(), tbl, 4, state)
    with pytest.raises(TypeError):
        grad_accumulate_(tbl, tbl.int(), 4, state)
    with pytest.raises(TypeError):
        grad_accumulate_(tbl, tbl, 4, state.float())
    with pytest.raises(ValueError):
        grad_accumulate_(tbl, tbl, -1, state)
    with pytest.raises(ValueError, match="GPU"):
        grad_accumulate_(tbl, tbl, 4, state)
    with pytest.raises(TypeError):
        grad_accum_tables_check(tbl.int(), tbl)
    with pytest.raises(ValueError, match="rows"):
        grad_accum_tables_check(tbl, tbl[:1])
    with pytest.raises(ValueError, match="GPU"):
        grad_norm(tbl, 4, state, (0.9, 0.95), main=True)
    with pytest.raises(ValueError, match="GPU"):
        adamw_step_(tbl, 4, torch.zeros((1, 2)), state, (0.9, 0.95), 1e-8, main=True)


def test_ops_are_exported_from_kgs_ops():
    import kgs.ops

    for name in ("grad_accumulate_", "grad_accum_tables_check", "ref_grad_accumulate", "adamw_table", "grad_norm",
                 "adamw_step_"):
        assert callable(getattr(kgs.ops, name))


# ----------------------------------------------------------------------------
# compile-time resources (hipcc cross-compiles gfx950 without a GPU)

@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_grad_accum_kernels_use_no_scratch(tmp_path):
    """Memory-bound streams: no kernel may spill or touch scratch, the file's kernels
    are the ones it declares (KERNEL_COUNT), and the fp32 step keeps the bf16 step's
    four waves per SIMD (at most 128 VGPRs)."""
    root = Path(__file__).resolve().parents[1]
    src = root / "native/kernels/grad_accum.hip"
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", str(root / "native/kernels"),
                          str(src), "-o", str(tmp_path / "grad_accum.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    for kernel, count in (("grad_accumulate", 2), ("micro_advance", 1), ("main_sumsq", 1), ("finalize_main", 1),
                          ("adamw_step_main", 1)):
        assert sum(kernel in n for n in res) == count, (kernel, sorted(res))
    assert all("ScratchSize" in r and "VGPRs Spill" in r and "VGPRs" in r for r in res.values()), res
    bad = {n: r for n, r in res.items() if r["ScratchSize"] or r["VGPRs Spill"]}
    assert not bad, bad
    (step,) = [r for n, r in res.items() if "adamw_step_main" in n and "Li2E" in n]
    assert step["VGPRs"] <= 128, step


# ----------------------------------------------------------------------------
# why: a bf16 running sum against the fp32 one

def test_eight_micro_batches_the_fp32_sum_is_exact_to_rounding_and_the_bf16_sum_is_not():
    """Eight micro-batches of unit-variance bf16 gradients, 65536 elements. The main
    gradient is within 8 * 2^-24 (seven fp32 adds of at most 2^-24 each, relative to
    partial sums that the 2-norm averages) of the float64 sum in relative 2-norm; the
    bf16 running sum that ``p.grad += ...`` keeps is worse than 1e-3 (3.7e-3 measured)."""
    n, k = 65536, 8
    g = _gen(16)
    p = torch.zeros(n, dtype=BF).requires_grad_(True)
    opt = AdamW([p], main_grads=True, backend="torch")
    exact, running = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=BF)
    for _ in range(k):
        grad = torch.randn(n, generator=g).to(BF)
        exact += grad.double()
        running += grad  # autograd's accumulation: a bf16 add
        p.grad = grad.clone()
        opt.accumulate()
    err_main = ((opt.main_grad(p).double() - exact).norm() / exact.norm()).item()
    err_bf16 = ((running.double() - exact).norm() / exact.norm()).item()
    print(f"relative 2-norm error of the sum of {k}: fp32 main {err_main:.3e}, bf16 running {err_bf16:.3e}")
    assert err_main <= 8 * 2.0 ** -24
    assert err_bf16 > 1e-3
