"""The sampling stage of a serving step: a step's logits in, its tokens (and the
logprobs some requests asked for) out, on their way to the host.

:class:`Sampler` needs no model and no scheduler: it reads the engine's
``{id: Request}`` dict and a ``[rows, vocab]`` logits tensor. There are two
routes. The torch route (any backend, any device) is a chain of torch ops with
per-request penalties and generators on the host. The device route
(``EngineConfig.device_sampler``, the kgs backend on a GPU) is one
``sample_rows`` launch per step, with ``EngineConfig.device_logit_ops`` also the
penalties from a device count table and the logprobs (k <= 32) in the step's
launches. :class:`PackedStaging` carries what crosses the bus for either:
per-row parameters up, tokens and logprobs down.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from kgs.ops.transformer import LOGPROB_KMAX


@dataclass
class SamplingParams:
    max_tokens: int = 16
    temperature: float = 0.0   # 0 = greedy
    top_k: int = 0             # 0 = full vocabulary
    top_p: float = 1.0         # nucleus: smallest set of tokens whose probability reaches top_p
    ignore_eos: bool = False
    stop_token_ids: tuple = ()
    logprobs: int | None = None  # None: off; k >= 0: the sampled token's logprob + the k most likely
    presence_penalty: float = 0.0   # OpenAI: minus this once for every token already generated
    frequency_penalty: float = 0.0  # OpenAI: minus this times the token's count in the output
    repetition_penalty: float = 1.0  # CTRL/HF: logits of prompt+output tokens divided (>0) / multiplied (<0)
    seed: int | None = None          # per-request sampling generator (reproducible regardless of batch mates)


@dataclass
class Request:
    id: int
    prompt: list
    params: SamplingParams
    output: list = field(default_factory=list)
    finished: bool = False
    finish_reason: str | None = None
    t_arrival: float = 0.0
    t_first: float | None = None
    t_done: float | None = None
    # per output token, when params.logprobs is set: (logprob, [(token, logprob)] top-k),
    # from the model's distribution before temperature / top-k / top-p
    logprobs: list = field(default_factory=list)
    gen: object = None  # torch.Generator of a seeded request
    sampled: int = 0    # tokens sampled so far: the device sampler's Philox counter (carries on across preemption)
    draw: tuple | None = None  # device sampler: (temperature, top_k, top_p, seed), fixed by Sampler.track


def _mix64(seed: int, rid: int) -> int:
    """The sampling seed of a request that gave none: splitmix64's finaliser over
    the engine seed and the request id."""
    m = (1 << 64) - 1
    z = (seed * 0x9E3779B97F4A7C15 + rid + 1) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _i64(v: int) -> int:
    """The low 64 bits of v as a signed integer (an int64 array element)."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


# PackedStaging layouts, (name, dtype[, row width]) in buffer order: what the kernels' pointers rely on
PARAM_FIELDS = (("seed", np.int64), ("counter", np.int64), ("temperature", np.float32), ("top_k", np.int32),
                ("top_p", np.float32))
LOGIT_OP_FIELDS = (("freq", np.float32), ("pres", np.float32), ("rep", np.float32), ("slot", np.int32),
                   ("want", np.int32))  # after PARAM_FIELDS, with device_logit_ops
LOGPROB_FIELDS = (("lp", np.float32), ("top_val", np.float32, LOGPROB_KMAX), ("top_idx", np.int32, LOGPROB_KMAX))
TOKEN_FIELDS = (("tokens", np.int64),)


class PackedStaging:
    """One packed device buffer plus two host buffers (pinned for a GPU) used
    alternately: with overlapped steps the host fills or reads one side while
    the other side's copy may still be queued. ``fields`` are laid out in the
    order given, each ``rows * width * itemsize`` bytes; a view is ``[rows]``
    or ``[rows, width]``. On a CPU device the copies are synchronous."""

    def __init__(self, fields, rows: int, device):
        layout, size = [], 0
        for name, dt, *width in fields:
            dt = np.dtype(dt)
            assert size % dt.itemsize == 0, f"field {name!r} ({dt}) at byte {size} is misaligned"
            layout.append((name, size, torch.from_numpy(np.empty(0, dt)).dtype, (rows, *width)))
            size += math.prod((rows, *width)) * dt.itemsize
        self.offsets = {name: lo for name, lo, _, _ in layout}
        device = torch.device(device)
        self._dev = torch.zeros(size, dtype=torch.uint8, device=device)
        self._host = [torch.zeros(size, dtype=torch.uint8, pin_memory=device.type == "cuda") for _ in range(2)]
        # torch views of the device buffer and of either host side
        self.dev, *self._host_t = [{name: b[lo:lo + math.prod(shape) * tdt.itemsize].view(tdt).reshape(shape)
                                    for name, lo, tdt, shape in layout} for b in (self._dev, *self._host)]
        self._host_np = [{k: v.numpy() for k, v in side.items()} for side in self._host_t]
        self._side = 0

    @property
    def host(self) -> dict:
        """Numpy views of the current host side (the one push() sends)."""
        return self._host_np[self._side]

    def push(self) -> None:
        """Async copy of the current host side to the device; the other side becomes current."""
        self._dev.copy_(self._host[self._side], non_blocking=True)
        self._side ^= 1

    def pull(self, **src) -> dict:
        """Async copy of the device buffer into the current host side, whose
        numpy views are returned (to be read after the caller's event); the other
        side becomes current. A field given by keyword is filled from that
        device tensor's rows instead of from the buffer, and only those fields
        are copied."""
        side, self._side = self._side, self._side ^ 1
        for name, t in src.items():
            self._host_t[side][name][:len(t)].copy_(t, non_blocking=True)
        if not src:
            self._host[side].copy_(self._dev, non_blocking=True)
        return self._host_np[side]


@dataclass
class Sampled:
    """A step's sampled tokens: on the device at once (``tokens``: the next step
    gathers its inputs from them), on the host after ``event``."""
    tokens: torch.Tensor
    event: object        # recorded after the read-back copies; None on a CPU device
    host_tokens: np.ndarray
    lps: dict | None     # the blocking route's rows, already tuples
    lp_rows: dict        # {row: k} of the rows logprob_rows served, their results in host_lp after the event
    host_lp: dict | None

    def result(self):
        """Wait for the read-back; (tokens int32, {row: (logprob, [(token, logprob)] top-k)} or None)."""
        if self.event is not None:
            self.event.synchronize()
        lps = self.lps
        if self.lp_rows:
            lp, tv, ti = (self.host_lp[k] for k in ("lp", "top_val", "top_idx"))
            lps = {**(lps or {}), **{j: (float(lp[j]), list(zip(ti[j, :k].tolist(), tv[j, :k].tolist())))
                                     for j, k in self.lp_rows.items()}}
        return self.host_tokens.astype(np.int32), lps


class Sampler:
    """The sampling stage and its per-request state. ``cfg``: the EngineConfig;
    ``requests``: the engine's own {id: Request}, held by reference."""

    def __init__(self, cfg, device, backend: str, vocab: int, requests: dict):
        if cfg.device_logit_ops and not cfg.device_sampler:
            raise ValueError("device_logit_ops=True needs device_sampler=True: the penalised logits and the count "
                             "table are consumed and updated by the device sampler's step")
        self.cfg, self.device, self.backend, self.vocab = cfg, torch.device(device), backend, vocab
        self.requests = requests
        # like paged_prefill, only the kgs backend on a GPU has the kernel; the logit ops only where it runs
        self.device_sampler = cfg.device_sampler and backend == "kgs" and self.device.type == "cuda"
        self.device_logit_ops = cfg.device_logit_ops and self.device_sampler
        self.gen = torch.Generator(device=self.device).manual_seed(cfg.seed)  # the unseeded requests' stream
        self.counts = None  # CountTable: the penalised requests' token-count rows on the device (device_logit_ops)
        # requests that need per-row work around the draw (the common greedy / plain-sampling batch skips those scans)
        self._want_lp: set = set()
        self._want_pen: set = set()
        self._seeded: set = set()
        self._lp_big: set = set()  # device_logit_ops: logprobs > LOGPROB_KMAX, the blocking torch route
        mb = cfg.max_batch
        self.tokens = PackedStaging(TOKEN_FIELDS, mb, self.device)  # only pulled, from each step's own tokens
        self.params = self.lp = None
        self._pen_buf = None  # [max_batch, vocab] bf16: the step's penalised logits (device_logit_ops)
        if self.device_sampler:
            self.params = PackedStaging(PARAM_FIELDS + (LOGIT_OP_FIELDS if self.device_logit_ops else ()), mb,
                                        self.device)
        if self.device_logit_ops:
            self.lp = PackedStaging(LOGPROB_FIELDS, mb, self.device)  # logprob_rows' outputs

    def track(self, r: Request) -> None:
        p = r.params
        if self.device_sampler:
            seed = p.seed if p.seed is not None else _mix64(self.cfg.seed, r.id)
            r.draw = (float(p.temperature), min(max(int(p.top_k), 0), 2**31 - 1), float(p.top_p), _i64(int(seed)))
        if p.logprobs is not None:
            self._want_lp.add(r.id)
            if self.device_logit_ops and p.logprobs > LOGPROB_KMAX:
                self._lp_big.add(r.id)
        if p.presence_penalty or p.frequency_penalty or p.repetition_penalty != 1.0:
            self._want_pen.add(r.id)
        if p.seed is not None:
            self._seeded.add(r.id)

    def forget(self, rid: int) -> None:
        """A finished or aborted request leaves the per-step scans and gives its count-table slot back."""
        for s in (self._want_lp, self._want_pen, self._seeded, self._lp_big):
            s.discard(rid)
        if self.counts is not None:
            self.counts.release(rid)

    def can_overlap(self) -> bool:
        """Whether the next step may be planned before the current one's tokens
        are known: logprobs, penalties and seeded sampling read per-step host
        state (the output so far, per-request generators), so a batch holding
        any of them runs one step at a time. The device sampler draws a seeded
        row from (seed, tokens sampled so far), both known ahead of the tokens:
        with it seeded requests overlap like any other. With device_logit_ops
        penalties read a count table the sampling step itself updates and
        logprobs (k <= 32) ride the token read-back: only a request asking for
        more than 32 logprobs still takes the blocking route."""
        if self.device_logit_ops:
            return not self._lp_big
        return not (self._want_lp or self._want_pen or (self._seeded and not self.device_sampler))

    def sample(self, ids, logits: torch.Tensor) -> Sampled:
        """One step: penalties, the draw, then the logprobs, and the launch of the
        read-back of tokens and device logprobs under one event. Logprob rows
        the kernel does not serve take a blocking torch route here (the logits
        are a graph output the next step overwrites); there are such rows only
        while can_overlap() is false, so an overlapped step never blocks."""
        reqs = [self.requests[int(r)] for r in ids]
        if self.device_sampler:
            toks, lp_rows = self._draw_device(reqs, logits)
        else:
            toks, lp_rows = self._draw_torch(reqs, logits), {}
        lps = self._logprobs_torch(reqs, logits, toks, lp_rows)
        host_tokens = self.tokens.pull(tokens=toks)["tokens"][:len(reqs)]
        host_lp = self.lp.pull() if lp_rows else None
        event = None
        if toks.is_cuda:
            event = torch.cuda.Event()
            event.record()
        return Sampled(toks, event, host_tokens, lps, lp_rows, host_lp)

    # ------------------------------------------------------------ torch route
    def _penalized_rows(self, reqs, logits: torch.Tensor):
        """(rows, their logits in fp32 after the penalties) for the rows whose
        request asks for presence / frequency / repetition penalties (a per-row
        token-count vector built from that request's tokens); ([], None) when
        none does."""
        rows = [j for j, r in enumerate(reqs) if r.id in self._want_pen] if self._want_pen else []
        if not rows:
            return [], None
        sub = logits[rows].float()
        vocab = sub.shape[1]
        for n, j in enumerate(rows):
            r = reqs[j]
            p = r.params
            if r.output and (p.presence_penalty or p.frequency_penalty):
                cnt = torch.bincount(torch.as_tensor(r.output, device=logits.device), minlength=vocab)[:vocab]
                sub[n] -= p.frequency_penalty * cnt + p.presence_penalty * (cnt > 0)
            if p.repetition_penalty != 1.0:
                seen = torch.as_tensor(sorted(set(r.prompt) | set(r.output)), device=logits.device)
                v = sub[n, seen]
                sub[n, seen] = torch.where(v > 0, v / p.repetition_penalty, v * p.repetition_penalty)
        return rows, sub

    def _draw_torch(self, reqs, logits: torch.Tensor) -> torch.Tensor:
        rows, sub = self._penalized_rows(reqs, logits)
        if rows:
            logits = logits.float().clone()
            logits[rows] = sub
        ps = [r.params for r in reqs]
        if all(p.temperature <= 0 for p in ps):
            return self._argmax(logits)
        lf = logits.float()
        temp = torch.tensor([max(p.temperature, 1e-5) for p in ps], device=lf.device)[:, None]
        lf = lf / temp
        ks = [p.top_k for p in ps]
        if any(k > 0 for k in ks):
            kmax = max(ks)
            vals, _ = lf.topk(kmax, dim=-1)
            kth = torch.tensor([k if k > 0 else kmax for k in ks], device=lf.device)[:, None] - 1
            thr = vals.gather(1, kth)
            full = torch.tensor([k <= 0 for k in ks], device=lf.device)[:, None]
            lf = torch.where(full | (lf >= thr), lf, torch.full_like(lf, float("-inf")))
        tp = [p.top_p for p in ps]
        if any(0.0 < t < 1.0 for t in tp):
            # nucleus: keep the highest-probability tokens until their mass reaches
            # top_p (the token that crosses it included); rows with top_p >= 1 keep all
            srt, idx = torch.sort(lf, dim=-1, descending=True)
            cum = torch.softmax(srt, dim=-1).cumsum(dim=-1)
            tpv = torch.tensor([t if 0.0 < t < 1.0 else 1.0 for t in tp], device=lf.device)[:, None]
            drop = (cum - torch.softmax(srt, dim=-1)) >= tpv  # mass before this token already reached top_p
            srt = srt.masked_fill(drop, float("-inf"))
            lf = torch.full_like(lf, float("-inf")).scatter(1, idx, srt)
        probs = torch.softmax(lf, dim=-1)
        sampled = torch.multinomial(probs, 1, generator=self.gen).squeeze(1)
        for j, req in enumerate(reqs if self._seeded else ()):  # seeded requests: their own generator
            if req.params.seed is not None and req.params.temperature > 0:
                if req.gen is None:
                    req.gen = torch.Generator(device=lf.device).manual_seed(int(req.params.seed))
                sampled[j] = torch.multinomial(probs[j], 1, generator=req.gen)[0]
        greedy = torch.tensor([p.temperature <= 0 for p in ps], device=lf.device)
        return torch.where(greedy, self._argmax(logits), sampled)

    def _argmax(self, logits: torch.Tensor) -> torch.Tensor:
        """Greedy pick: the native row argmax for bf16 GPU logits of the kgs
        backend (torch's generic reduce takes ~40 us for one 128k-vocab row)."""
        if self.backend == "kgs" and logits.is_cuda and logits.dtype == torch.bfloat16 and \
                logits.dim() == 2 and logits.shape[-1] % 8 == 0 and logits.stride(-1) == 1 and \
                logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0:
            from kgs.ops.transformer import argmax_rows

            return argmax_rows(logits)
        return logits.argmax(dim=-1)

    def _logprobs_torch(self, reqs, logits: torch.Tensor, toks: torch.Tensor, served: dict):
        """{row: (logprob of the sampled token, [(token, logprob)] top-k)} for the
        rows whose request asked for logprobs and that logprob_rows did not serve
        (``served``); None when there is none. Blocks on the device."""
        if not self._want_lp:
            return None
        rows = [j for j, r in enumerate(reqs) if r.id in self._want_lp and j not in served]
        if not rows:
            return None
        sel = torch.as_tensor(rows, device=logits.device)
        lp = torch.log_softmax(logits[sel].float(), dim=-1)
        chosen = lp.gather(1, toks[sel].long()[:, None])[:, 0].cpu().tolist()
        k = max(reqs[j].params.logprobs for j in rows)
        top_v, top_i = (lp.topk(k, dim=-1) if k > 0 else (lp[:, :0], lp[:, :0].long()))
        top_v, top_i = top_v.cpu().tolist(), top_i.cpu().tolist()
        out = {}
        for n, j in enumerate(rows):
            kj = reqs[j].params.logprobs
            out[j] = (chosen[n], list(zip(top_i[n][:kj], top_v[n][:kj])))
        return out

    # ----------------------------------------------------------- device route
    def _draw_device(self, reqs, logits: torch.Tensor):
        """EngineConfig.device_sampler: the whole step's tokens from one
        sample_rows launch, greedy rows included; returns (tokens, {row: k} of
        the rows logprob_rows served). The per-row parameters go through one
        packed staging buffer and one async copy. Row j draws with (its
        request's seed, the number of tokens that request has sampled): neither
        depends on its batch mates or on a token not yet read back. Penalised
        rows are computed in fp32 as on the torch route and rounded back to
        bf16 (one extra rounding of those rows' logits); every row then takes
        the kernel. With EngineConfig.device_logit_ops the penalties are three
        launches around the sampler instead, whatever the number of penalised
        rows: penalize_rows writes the step's penalised logits into a buffer of
        the sampler's from the device count table (kgs.serve.count_table),
        sample_rows draws from that buffer, token_counts_add counts the drawn
        tokens. A step without a penalised row is unchanged. Then one
        logprob_rows launch on the step's raw logits for the rows that want at
        most 32 logprobs; its results stay on the device until sample() pulls
        them with the tokens."""
        from kgs.ops.transformer import logprob_rows, penalize_rows, sample_rows, token_counts_add

        if not (logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2):
            raise RuntimeError(f"device_sampler needs bf16 GPU logits [rows, vocab], got {logits.dtype} "
                               f"{tuple(logits.shape)} on {logits.device}")
        raw = logits
        if not self.device_logit_ops:
            rows, sub = self._penalized_rows(reqs, logits)
            if rows:
                logits = logits.clone()
                logits[rows] = sub.to(torch.bfloat16)
        n, hn = len(reqs), self.params.host
        draws = [r.draw for r in reqs]
        hn["temperature"][:n] = [w[0] for w in draws]
        hn["top_k"][:n] = [w[1] for w in draws]
        hn["top_p"][:n] = [w[2] for w in draws]
        hn["seed"][:n] = [w[3] for w in draws]
        hn["counter"][:n] = [r.sampled for r in reqs]
        for r in reqs:
            r.sampled += 1
        pen, lp_rows = self._stage_logit_ops(reqs, hn) if self.device_logit_ops else (False, {})
        self.params.push()
        v = self.params.dev
        if pen:
            if self._pen_buf is None:
                self._pen_buf = torch.empty((self.cfg.max_batch, self.vocab), dtype=torch.bfloat16, device=self.device)
            logits = penalize_rows(logits, v["freq"][:n], v["pres"][:n], v["rep"][:n], v["slot"][:n],
                                   self.counts.table, out=self._pen_buf[:n])
        toks = sample_rows(logits, v["temperature"][:n], v["top_k"][:n], v["top_p"][:n], v["seed"][:n],
                           v["counter"][:n])
        if pen:  # the sampled tokens join their requests' counts before the next step reads them
            token_counts_add(self.counts.table, toks, v["slot"][:n])
        if lp_rows:
            out = self.lp.dev
            logprob_rows(raw, toks, v["want"][:n], out["lp"][:n], out["top_val"][:n], out["top_idx"][:n])
        return toks, lp_rows

    def _stage_logit_ops(self, reqs, hn):
        """The step's per-row penalty parameters, count-table slots and logprob
        wishes into the packed parameter buffer; a penalised request takes its
        slot here, the first time it is sampled. Returns (whether any row is
        penalised, {row: k} of the rows that want at most 32 logprobs)."""
        n = len(reqs)
        hn["slot"][:n] = -1
        hn["want"][:n] = -1
        pen, lp_rows = False, {}
        for j, r in enumerate(reqs if (self._want_pen or self._want_lp) else ()):
            p = r.params
            if r.id in self._want_pen:
                if self.counts is None:
                    from .count_table import CountTable

                    self.counts = CountTable(self.vocab, self.device)
                hn["slot"][j] = self.counts.acquire(r.id, r.prompt, r.output)
                hn["freq"][j], hn["pres"][j], hn["rep"][j] = p.frequency_penalty, p.presence_penalty, \
                    p.repetition_penalty
                pen = True
            if r.id in self._want_lp and r.id not in self._lp_big:
                hn["want"][j] = lp_rows[j] = int(p.logprobs)
        return pen, lp_rows
