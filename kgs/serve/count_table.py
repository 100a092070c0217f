"""Per-request token-count rows for the device penalties
(``EngineConfig.device_logit_ops``): an int32 ``[slots, vocab]`` table on the
sampler's device and the bookkeeping of which request holds which row.

A count word ``w``: ``w & COUNT_MASK`` is the token's count in the request's
output, ``w & COUNT_PROMPT`` marks a prompt token
(:func:`kgs.ops.transformer.penalize_rows` reads them). A request takes a slot
the first time one of its rows reaches the sampler; the row is built once from
the host's lists and from then on the step that samples a token counts it
(:func:`kgs.ops.transformer.token_counts_add`), so the host never has to know
the pending token. The slot stays with the request across preemption and is
released when it finishes or is aborted.

The table costs ``4 * vocab`` bytes per slot (513 KB at the Llama-3
vocabulary). It starts with a few slots and doubles when they run out; it is
not taken out of the KV budget. Everything here is plain torch, so the class
works on CPU tensors as well (the CPU tests drive it that way).
"""
from __future__ import annotations

import torch

from kgs.ops.transformer import COUNT_MASK, COUNT_PROMPT  # noqa: F401  (re-exported: the word format)


class CountTable:
    def __init__(self, vocab: int, device="cpu", slots: int = 4):
        self.vocab = int(vocab)
        self.device = torch.device(device)
        self.table = torch.zeros((max(1, int(slots)), self.vocab), dtype=torch.int32, device=self.device)
        self._slot_of: dict[int, int] = {}
        self._free = list(range(self.table.shape[0] - 1, -1, -1))  # popped from the end: lowest slot first

    @property
    def slots(self) -> int:
        return self.table.shape[0]

    @property
    def used(self) -> int:
        return len(self._slot_of)

    def slot(self, rid: int) -> int:
        """The request's slot, -1 when it holds none."""
        return self._slot_of.get(rid, -1)

    def acquire(self, rid: int, prompt, output) -> int:
        """The request's slot; on first use a free one, its row built from the
        request's prompt (the prompt bit) and its output so far (the counts)."""
        s = self._slot_of.get(rid)
        if s is not None:
            return s
        if not self._free:
            self._grow()
        s = self._slot_of[rid] = self._free.pop()
        row = self.table[s]
        row.zero_()
        seen = sorted({int(t) for t in prompt if 0 <= int(t) < self.vocab})
        if seen:
            row.index_fill_(0, torch.as_tensor(seen, dtype=torch.int64, device=self.device), COUNT_PROMPT)
        out = [int(t) for t in output if 0 <= int(t) < self.vocab]
        if out:
            row.index_add_(0, torch.as_tensor(out, dtype=torch.int64, device=self.device),
                           torch.ones(len(out), dtype=torch.int32, device=self.device))
        return s

    def release(self, rid: int) -> None:
        """Give the request's slot back (a request without one: nothing). The
        row is zeroed by the next request that takes the slot."""
        s = self._slot_of.pop(rid, None)
        if s is not None:
            self._free.append(s)

    def _grow(self) -> None:
        old = self.table
        n = old.shape[0]
        self.table = torch.zeros((2 * n, self.vocab), dtype=torch.int32, device=self.device)
        self.table[:n].copy_(old)
        self._free.extend(range(2 * n - 1, n - 1, -1))
