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
    :meth:`update_groups`."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: float | None = None, backend: str = "kgs", amsgrad: bool = False,
                 maximize: bool = False):
        if backend not in ("kgs", "torch"):
            raise ValueError(f"backend must be 'kgs' or 'torch', got {backend!r}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive")
        self.backend = backend
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
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
        # device blocks: the step's scalars (kgs.ops.optim.STATE_*) and {lr, weight_decay} per group
        self._state = torch.zeros(_ops.STATE_WORDS, dtype=torch.int32, device=dev)
        self._state.view(torch.float32)[_ops.STATE_CLIP] = 1.0
        self._groups = torch.zeros((len(self.param_groups), 2), dtype=torch.float32, device=dev)
        self._group_key = None
        self._table = self._partials = self._table_key = None
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

    def _update_table(self) -> None:
        key = tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in self._params)
        if key == self._table_key:
            return
        st = [self.state[p] for p in self._params]
        host, nchunks = _ops.adamw_table([p.detach().reshape(-1) for p in self._params],
                                         [s["master"].reshape(-1) for s in st],
                                         [s["exp_avg"].reshape(-1) for s in st],
                                         [s["exp_avg_sq"].reshape(-1) for s in st],
                                         [None if p.grad is None else p.grad.reshape(-1) for p in self._params],
                                         self._group_of, len(self.param_groups))
        if self._table is None:
            self._table = torch.empty_like(host, device=self.device)
            self._partials = torch.empty(max(nchunks, 4), dtype=torch.float32, device=self.device)
        assert nchunks == self._nchunks or self._table_key is None  # numels do not change
        self._nchunks = nchunks
        self._upload(self._table, host)
        self._table_key = key
        self.table_refreshes += 1

    # ------------------------------------------------------------------ the step

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.backend == "kgs":
            for p in self._params:
                if p.grad is not None and (p.grad.dtype != torch.bfloat16 or not p.grad.is_contiguous()):
                    raise ValueError("the kgs backend needs contiguous bf16 gradients")
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

    def _step_torch(self) -> None:
        """The kernels' algorithm in torch fp32 ops; the skip is a select, not a branch."""
        live = [(i, p) for i, p in enumerate(self._params) if p.grad is not None]
        sf, si = self._state.view(torch.float32), self._state
        b1, b2 = self.betas
        if self.max_grad_norm is not None and live:
            norm = _sumsq([p.grad for _, p in live]).sqrt()
            ok = torch.isfinite(norm)
            clip = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
            sf[_ops.STATE_GRAD_NORM] = norm
        else:
            ok = torch.ones((), dtype=torch.bool, device=self.device)
            clip = torch.ones((), dtype=torch.float32, device=self.device)
        si[_ops.STATE_SKIP] = (~ok).to(torch.int32)
        si[_ops.STATE_SKIPPED] += (~ok).to(torch.int32)
        si[_ops.STATE_STEP] += ok.to(torch.int32)
        t = si[_ops.STATE_STEP].double()
        bc1 = (1.0 - torch.pow(torch.tensor(b1, dtype=torch.float64, device=self.device), t)).float()
        bc2 = (1.0 - torch.pow(torch.tensor(b2, dtype=torch.float64, device=self.device), t)).float()
        bc1, bc2 = torch.where(ok, bc1, sf[_ops.STATE_BC1]), torch.where(ok, bc2, sf[_ops.STATE_BC2])
        sf[_ops.STATE_CLIP] = torch.where(ok, clip, sf[_ops.STATE_CLIP])
        sf[_ops.STATE_BC1], sf[_ops.STATE_BC2] = bc1, bc2
        for i, p in live:
            s = self.state[p]
            lr, wd = self._groups[self._group_of[i]]
            g = clip * p.grad.float()
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

    # ------------------------------------------------------------------ checkpoints

    def state_dict(self):
        step = float(self.step_count)
        for p in self._params:
            self.state[p]["step"] = torch.tensor(step, dtype=torch.float32)
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """torch's layout; ``torch.optim.Optimizer.load_state_dict`` itself would cast
        the fp32 state to the parameters' bf16, so the tensors are copied here."""
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
