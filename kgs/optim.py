"""``kgs.optim.AdamW``: AdamW with fp32 master weights for bf16 models, global-norm
gradient clipping and a step that never synchronises with the host.

The parameters stay bf16 (what the kernels of ``kgs.ops`` read); the optimizer
owns an fp32 master copy and fp32 moments, updates those and re-rounds the bf16
weights from the masters every step. A bf16 norm weight of 1.0 with lr 1e-3 never
moves under ``torch.optim.AdamW`` (``1 - 0.001`` rounds back to 1.0); here the
master moves and the weight follows once the master crosses a rounding boundary.

``backend="kgs"`` runs the step of every tensor in three launches of
``native/kernels/optimizer.hip`` (two without clipping) over a device-resident
tensor table; ``backend="torch"`` is the same algorithm in plain torch fp32 ops,
on any device. Both keep lr, the step counter, the clip factor and the skip
decision on the device: nothing in ``step()`` waits for the GPU, and with
``zero_grad(set_to_none=False)`` a step can be captured in ``torch.cuda.graph``.

``main_grads=True`` adds fp32 main gradients for training with micro-batches:
``accumulate()`` after each ``backward()`` folds the bf16 ``.grad`` of every tensor
into them in one launch of ``native/kernels/grad_accum.hip`` (and zeroes ``.grad``
in the same pass), and ``step()`` reads them instead of ``.grad``. A bf16 running
sum, which is what ``p.grad += ...`` keeps, rounds once per micro-batch relative
to the sum; the fp32 sum keeps what the fp32 masters were built to keep.
"""
from __future__ import annotations

from itertools import chain

import torch

from .ops import optim as _ops

_ALIGN = 64  # every tensor's segment of the flat state buffers starts on a multiple of this many elements


def decay_groups(module: torch.nn.Module, weight_decay: float) -> list[dict]:
    """Two parameter groups of ``module``: tensors with ``ndim >= 2`` (matrices,
    embeddings) decayed by ``weight_decay``, the rest (norm weights) not."""
    params = [p for p in module.parameters() if p.requires_grad]
    return [{"params": [p for p in params if p.ndim >= 2], "weight_decay": float(weight_decay)},
            {"params": [p for p in params if p.ndim < 2], "weight_decay": 0.0}]


def _sumsq(grads) -> torch.Tensor:
    """The torch backend's norm pass: fp32 sum of squares of all gradients, in list order."""
    total = torch.zeros((), dtype=torch.float32, device=grads[0].device)
    for g in grads:
        total = total + g.float().pow(2).sum()
    return total


class AdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay) on fp32 masters and moments.

    Per group ``lr`` and ``weight_decay``; ``betas`` and ``eps`` are the same for all
    groups. ``max_grad_norm`` clips the gradients' global 2-norm with
    ``torch.nn.utils.clip_grad_norm_``'s factor, inside the step (the gradients
    themselves are not modified); a norm that is not finite skips the step: no
    buffer changes, ``step_count`` stays and ``skipped_steps`` grows by one. Without
    ``max_grad_norm`` there is no norm pass and no step is skipped. A parameter
    whose ``.grad`` is ``None`` is left alone. There is one step counter for all
    tensors: the bias corrections are those of ``step_count``.

    ``state_dict()`` has torch's layout, per parameter ``step``, ``exp_avg``,
    ``exp_avg_sq`` and ``master``, all fp32; a ``torch.optim.AdamW`` state loads too
    (the masters are then taken from the parameters).

    The kgs backend needs contiguous bf16 parameters and bf16 gradients on one GPU.
    ``step()`` re-reads the groups' ``lr`` / ``weight_decay`` (an LR scheduler works)
    and the parameters' and gradients' addresses, and uploads the group block or the
    tensor table only when they changed. A captured step replays the addresses it
    was captured with; after changing a group's ``lr`` between replays call
    :meth:`update_groups`.

    ``main_grads=True``: a fourth flat fp32 buffer, ``main_grad``, laid out like the
    masters (:meth:`main_grad` is a tensor's view of it). :meth:`accumulate` after
    each micro-batch's ``backward()`` sets it to ``float(grad)`` on the first
    micro-batch of a cycle and adds ``float(grad)`` afterwards, one fp32 add per
    element; ``step()`` then ignores ``.grad`` and takes ``s * main_grad`` as the
    gradient, ``s = 1 / n`` over the ``n`` micro-batches of the cycle with
    ``grad_average`` and 1 without. ``grad_norm`` is the norm of that scaled
    gradient. Applied or skipped, a step consumes the cycle: the next
    ``accumulate()`` starts a fresh sum. A parameter that had no gradient at any
    ``accumulate()`` of the cycle is left alone. The micro-batch count lives in the
    device state block, so one captured ``accumulate()`` and one captured ``step()``
    replay cycles of any length; a replayed step with nothing accumulated counts
    as skipped, an eager one raises. Main gradients are not part of
    ``state_dict()``."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: float | None = None, backend: str = "kgs", amsgrad: bool = False,
                 maximize: bool = False, main_grads: bool = False, grad_average: bool = True):
        if backend not in ("kgs", "torch"):
            raise ValueError(f"backend must be 'kgs' or 'torch', got {backend!r}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive")
        self.backend = backend
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.main_grads, self.grad_average = bool(main_grads), bool(grad_average)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize))
        self._check_groups()
        self._params = list(chain.from_iterable(g["params"] for g in self.param_groups))
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        if not self._params:
            raise ValueError("AdamW got no parameters")
        dev = self._params[0].device
        for p in self._params:
            if p.device != dev:
                raise ValueError("all parameters must be on one device")
            if backend == "kgs" and (p.dtype != torch.bfloat16 or not p.is_contiguous()):
                raise ValueError("the kgs backend needs contiguous bf16 parameters")
            if backend == "torch" and not p.is_floating_point():
                raise ValueError("parameters must be floating point")
        self.device = dev
        # flat fp32 state: master, first and second moment, one segment per tensor
        self._offsets, total = [], 0
        for p in self._params:
            self._offsets.append(total)
            total += -(-p.numel() // _ALIGN) * _ALIGN
        self._flat = {k: torch.zeros(max(total, _ALIGN), dtype=torch.float32, device=dev)
                      for k in ("master", "exp_avg", "exp_avg_sq")}
        for p, off in zip(self._params, self._offsets):
            seg = {k: f[off:off + p.numel()].view(p.shape) for k, f in self._flat.items()}
            seg["master"].copy_(p.detach())  # bf16 -> fp32 is exact
            self.state[p] = {"step": torch.zeros((), dtype=torch.float32), **seg}
        self._main = {}
        if self.main_grads:  # not optimizer state: never checkpointed
            self._flat["main_grad"] = torch.zeros_like(self._flat["master"])
            self._main = {p: self._flat["main_grad"][off:off + p.numel()].view(p.shape)
                          for p, off in zip(self._params, self._offsets)}
        # device blocks: the step's scalars (kgs.ops.optim.STATE_*) and {lr, weight_decay} per group
        self._state = torch.zeros(_ops.STATE_WORDS, dtype=torch.int32, device=dev)
        self._state.view(torch.float32)[_ops.STATE_CLIP] = 1.0
        self._groups = torch.zeros((len(self.param_groups), 2), dtype=torch.float32, device=dev)
        self._group_key = None
        self._table = self._partials = self._table_key = None
        # main gradients: the table of all of them (accumulate) and of those the cycle gave a gradient (step)
        self._main_all = self._main_all_key = self._main_live = self._main_live_key = None
        self._host_tables = {}
        self._host_micro, self._cycle_live = 0, set()  # accumulate() calls since the last step, who had a gradient
        self._nchunks = 0
        self.table_refreshes = 0
        self.group_refreshes = 0

    # ------------------------------------------------------------------ checks

    def _check_groups(self) -> None:
        first = self.param_groups[0]
        for g in self.param_groups:
            if tuple(g["betas"]) != tuple(first["betas"]) or g["eps"] != first["eps"]:
                raise ValueError("betas and eps must be the same for every parameter group")
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("amsgrad and maximize are not supported")
            b1, b2 = g["betas"]
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not g["eps"] >= 0.0:
                raise ValueError("betas must be in [0, 1) and eps must not be negative")
            if not g["lr"] >= 0.0 or not g["weight_decay"] >= 0.0:
                raise ValueError("lr and weight_decay must not be negative")

    def add_param_group(self, param_group):
        if getattr(self, "_flat", None) is not None:
            raise ValueError("parameter groups cannot be added after construction: the state buffers are flat")
        super().add_param_group(param_group)

    @property
    def betas(self):
        return tuple(self.param_groups[0]["betas"])

    @property
    def eps(self) -> float:
        return float(self.param_groups[0]["eps"])

    # ------------------------------------------------------------------ device blocks

    def _upload(self, dst: torch.Tensor, host: torch.Tensor) -> None:
        # a fresh staging tensor per upload: an earlier asynchronous copy may still be reading the last one
        if dst.is_cuda:
            dst.copy_(host if host.is_pinned() else host.pin_memory(), non_blocking=True)
        else:
            dst.copy_(host)

    def update_groups(self) -> bool:
        """Upload the groups' ``lr`` / ``weight_decay`` if they differ from what the
        device holds (``step()`` does this itself). Returns whether it uploaded."""
        key = tuple((float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups)
        if key == self._group_key:
            return False
        self._upload(self._groups, torch.tensor(key, dtype=torch.float32).reshape(-1, 2))
        self._group_key = key
        self.group_refreshes += 1
        return True

    def _update_table(self, which: str = "_table", live=None) -> bool:
        """Upload table ``which`` if an address in it changed; returns whether it did.
        ``_table``: the bf16 ``.grad`` as gradients. ``_main_all`` / ``_main_live``: the
        fp32 main gradients of every tensor / of the tensors in ``live``."""
        if which == "_table":
            grads = [None if p.grad is None else p.grad.reshape(-1) for p in self._params]
        else:
            grads = [self._main[p].reshape(-1) if live is None or i in live else None
                     for i, p in enumerate(self._params)]
        key = tuple((p.data_ptr(), 0 if g is None else g.data_ptr()) for p, g in zip(self._params, grads))
        if key == getattr(self, which + "_key"):
            return False
        st = [self.state[p] for p in self._params]
        host, nchunks = _ops.adamw_table([p.detach().reshape(-1) for p in self._params],
                                         [s["master"].reshape(-1) for s in st],
                                         [s["exp_avg"].reshape(-1) for s in st],
                                         [s["exp_avg_sq"].reshape(-1) for s in st],
                                         grads, self._group_of, len(self.param_groups),
                                         grad_dtype=torch.bfloat16 if which == "_table" else torch.float32)
        if getattr(self, which) is None:
            setattr(self, which, torch.empty_like(host, device=self.device))
        if self._partials is None:
            self._partials = torch.empty(max(nchunks, 4), dtype=torch.float32, device=self.device)
        assert self._nchunks in (0, nchunks)  # numels do not change
        self._nchunks = nchunks
        self._upload(getattr(self, which), host)
        self._host_tables[which] = host
        setattr(self, which + "_key", key)
        self.table_refreshes += 1
        return True

    # ------------------------------------------------------------------ main gradients

    def main_grad(self, p: torch.Tensor) -> torch.Tensor:
        """The fp32 main gradient of parameter ``p``: a view of the flat buffer."""
        if not self.main_grads:
            raise RuntimeError("main_grad() needs AdamW(main_grads=True)")
        return self._main[p]

    @torch.no_grad()
    def accumulate(self, zero_grads: bool = True) -> None:
        """Fold every parameter's ``.grad`` into its fp32 main gradient; call it after
        each micro-batch's ``backward()``. The first call of a cycle overwrites
        (``main = float(grad)``), the later ones add (one fp32 add per element). With
        ``zero_grads`` the gradients are zeroed in the same pass and stay allocated
        where they are, so the next ``backward()`` accumulates into zeros and no
        ``zero_grad()`` is needed. A ``.grad`` that is ``None`` contributes nothing; on
        the first call of a cycle that tensor's main gradient is written as zeros. The
        kgs backend: one launch over the tensor table and a one-thread launch that
        advances the device's micro-batch count, no host synchronisation."""
        if not self.main_grads:
            raise RuntimeError("accumulate() needs AdamW(main_grads=True)")
        live = {i for i, p in enumerate(self._params) if p.grad is not None}
        if self.backend == "kgs":
            self._check_grads()
            a, b = self._update_table(), self._update_table("_main_all")
            if a or b:
                _ops.grad_accum_tables_check(self._host_tables["_table"], self._host_tables["_main_all"])
            _ops.grad_accumulate_(self._table, self._main_all, self._nchunks, self._state, zero_grads=zero_grads)
        else:
            micro = self._state[_ops.STATE_MICRO]
            first = micro <= 0
            for p in self._params:
                a = self._main[p]
                if p.grad is None:
                    a.copy_(torch.where(first, torch.zeros_like(a), a))
                    continue
                g = p.grad.float()
                a.copy_(torch.where(first, g, a + g))
                if zero_grads:
                    p.grad.zero_()
            self._state[_ops.STATE_MICRO] = torch.where(first, torch.ones_like(micro), micro + 1)
        self._cycle_live |= live
        self._host_micro += 1

    def _check_grads(self) -> None:
        for p in self._params:
            if p.grad is not None and (p.grad.dtype != torch.bfloat16 or not p.grad.is_contiguous()):
                raise ValueError("the kgs backend needs contiguous bf16 gradients")

    # ------------------------------------------------------------------ the step

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.main_grads:
            self._step_main()
        elif self.backend == "kgs":
            self._check_grads()
            self._update_table()
            self.update_groups()
            clipping = self.max_grad_norm is not None
            _ops.grad_norm(self._table, self._nchunks, self._state, self.betas,
                           partials=self._partials if clipping else None, max_norm=self.max_grad_norm)
            _ops.adamw_step_(self._table, self._nchunks, self._groups, self._state, self.betas, self.eps)
        else:
            self.update_groups()
            self._step_torch()
        return loss

    def _step_main(self) -> None:
        """A step from the main gradients of the tensors the cycle gave a gradient."""
        if self._host_micro == 0:
            raise RuntimeError("step() with nothing accumulated: call accumulate() after each backward()")
        live = self._cycle_live
        self.update_groups()
        if self.backend == "kgs":
            self._update_table("_main_live", live)
            clipping = self.max_grad_norm is not None
            _ops.grad_norm(self._main_live, self._nchunks, self._state, self.betas,
                           partials=self._partials if clipping else None, max_norm=self.max_grad_norm, main=True,
                           average=self.grad_average)
            _ops.adamw_step_(self._main_live, self._nchunks, self._groups, self._state, self.betas, self.eps,
                             main=True, average=self.grad_average)
        else:
            micro = self._state[_ops.STATE_MICRO]
            has = micro > 0
            s = 1.0 / micro.clamp(min=1).float() if self.grad_average else torch.ones((), device=self.device)
            self._step_torch([(i, p, s * self._main[p]) for i, p in enumerate(self._params) if i in live], has)
            self._state[_ops.STATE_MICRO] = torch.where(has, -micro, micro)
        self._host_micro, self._cycle_live = 0, set()

    def _step_torch(self, live=None, has=None) -> None:
        """The kernels' algorithm in torch fp32 ops; the skip is a select, not a branch.
        ``live``: ``(index, parameter, gradient)`` of the tensors to step, by default
        those with a ``.grad``; ``has``: a device flag that must hold for the step to
        be applied (main gradients: something was accumulated)."""
        if live is None:
            live = [(i, p, p.grad) for i, p in enumerate(self._params) if p.grad is not None]
        sf, si = self._state.view(torch.float32), self._state
        b1, b2 = self.betas
        if self.max_grad_norm is not None and live:
            norm = _sumsq([g for _, _, g in live]).sqrt()
            ok = torch.isfinite(norm)
            clip = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
            sf[_ops.STATE_GRAD_NORM] = norm
        else:
            ok = torch.ones((), dtype=torch.bool, device=self.device)
            clip = torch.ones((), dtype=torch.float32, device=self.device)
        if has is not None:
            ok = ok & has
        si[_ops.STATE_SKIP] = (~ok).to(torch.int32)
        si[_ops.STATE_SKIPPED] += (~ok).to(torch.int32)
        si[_ops.STATE_STEP] += ok.to(torch.int32)
        t = si[_ops.STATE_STEP].double()
        bc1 = (1.0 - torch.pow(torch.tensor(b1, dtype=torch.float64, device=self.device), t)).float()
        bc2 = (1.0 - torch.pow(torch.tensor(b2, dtype=torch.float64, device=self.device), t)).float()
        bc1, bc2 = torch.where(ok, bc1, sf[_ops.STATE_BC1]), torch.where(ok, bc2, sf[_ops.STATE_BC2])
        sf[_ops.STATE_CLIP] = torch.where(ok, clip, sf[_ops.STATE_CLIP])
        sf[_ops.STATE_BC1], sf[_ops.STATE_BC2] = bc1, bc2
        for i, p, grad in live:
            s = self.state[p]
            lr, wd = self._groups[self._group_of[i]]
            g = clip * grad.float()
            m = b1 * s["exp_avg"] + (1 - b1) * g
            v = b2 * s["exp_avg_sq"] + (1 - b2) * g * g
            new = s["master"] * (1 - lr * wd) - lr * (m / bc1) / ((v / bc2).sqrt() + self.eps)
            s["exp_avg"].copy_(torch.where(ok, m, s["exp_avg"]))
            s["exp_avg_sq"].copy_(torch.where(ok, v, s["exp_avg_sq"]))
            s["master"].copy_(torch.where(ok, new, s["master"]))
            p.copy_(torch.where(ok, s["master"].to(p.dtype), p))

    # ------------------------------------------------------------------ what the device knows (one sync each)

    def _word(self, i: int, as_float: bool):
        block = self._state.cpu()
        return float(block.view(torch.float32)[i]) if as_float else int(block[i])

    @property
    def grad_norm(self):
        """The last step's global gradient norm, ``None`` without ``max_grad_norm``."""
        return None if self.max_grad_norm is None else self._word(_ops.STATE_GRAD_NORM, True)

    @property
    def clip(self) -> float:
        """The factor the last applied step scaled its gradients by."""
        return self._word(_ops.STATE_CLIP, True)

    @property
    def step_count(self) -> int:
        return self._word(_ops.STATE_STEP, False)

    @property
    def skipped_steps(self) -> int:
        return self._word(_ops.STATE_SKIPPED, False)

    @property
    def pending_micro_batches(self) -> int:
        """Micro-batches accumulated since the last step, as the device counts them."""
        return max(self._word(_ops.STATE_MICRO, False), 0)

    # ------------------------------------------------------------------ checkpoints

    def state_dict(self):
        step = float(self.step_count)
        for p in self._params:
            self.state[p]["step"] = torch.tensor(step, dtype=torch.float32)
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """torch's layout; ``torch.optim.Optimizer.load_state_dict`` itself would cast
        the fp32 state to the parameters' bf16, so the tensors are copied here. Main
        gradients are not checkpointed: loading resets the accumulation cycle, and
        whatever was accumulated and not yet stepped is dropped."""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(s["params"]) != len(g["params"])
                                                       for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")
        for s, g in zip(saved, self.param_groups):
            g.update({k: v for k, v in s.items() if k != "params"})
            g["betas"] = tuple(g["betas"])
        self._check_groups()
        ids = chain.from_iterable(s["params"] for s in saved)
        steps = set()
        for pid, p in zip(ids, self._params):
            mine, theirs = self.state[p], state_dict["state"].get(pid)
            if theirs is None:
                mine["exp_avg"].zero_()
                mine["exp_avg_sq"].zero_()
                mine["master"].copy_(p)
                continue
            mine["exp_avg"].copy_(theirs["exp_avg"])
            mine["exp_avg_sq"].copy_(theirs["exp_avg_sq"])
            mine["master"].copy_(theirs["master"] if "master" in theirs else p)
            steps.add(int(theirs["step"]))
        if len(steps) > 1:
            raise ValueError(f"one step counter for all tensors, the state dict has {sorted(steps)}")
        block = torch.zeros(_ops.STATE_WORDS, dtype=torch.int32)
        block[_ops.STATE_STEP] = steps.pop() if steps else 0
        block[_ops.STATE_SKIPPED] = self.skipped_steps
        block.view(torch.float32)[_ops.STATE_CLIP] = 1.0
        self._upload(self._state, block)
        self._group_key = None
        self._host_micro, self._cycle_live = 0, set()
