"""Logit penalties (the ``repetition_penalty=`` / ``frequency_penalty=`` / ``presence_penalty=`` keywords of the engines'
generate and generate_batch).

While any of them is on, every pick - prompt pass or decode step, single or batched, eager or graph-replayed, JSON mode and
nucleus sampling included - is handed the row vis_penalize_f32 wrote instead of the model's raw logits.  For one sequence
with prompt ids P and c[v] = times id v was generated so far:

    seen = v in P or c[v] > 0
    y = x[v]                                  if not seen or r == 1
    y = x[v] * r if x[v] < 0 else x[v] / r    (transformers' RepetitionPenaltyLogitsProcessor)
    y = y - f * c[v] - q * (c[v] > 0)         (OpenAI's frequency / presence penalties)

on the raw logits, before temperature, the JSON mask and the nucleus cut.  The raw row stays where it is (logprobs keep
reading it).  The values (r, f, q) live in device memory, one triple per slot, so requests of one batch may differ and a
captured decode graph serves any values.  ``penalize_ref`` is the float64 reference the tests compare the kernel against."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip

NEUTRAL = (1.0, 0.0, 0.0)


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating)) and math.isfinite(float(x))


def check_repetition_penalty(r) -> Optional[float]:
    """None (off) or a finite number > 0 (transformers' condition)."""
    if r is None:
        return None
    if not _number(r) or not float(r) > 0.0:
        raise ValueError("repetition_penalty must be None or a finite number above 0")
    return float(r)


def _check_openai(x, name: str) -> Optional[float]:
    if x is None:
        return None
    if not _number(x) or not -2.0 <= float(x) <= 2.0:
        raise ValueError(f"{name} must be None or a number in [-2, 2]")
    return float(x)


def check_frequency_penalty(f) -> Optional[float]:
    """None (off) or a finite number in [-2, 2] (OpenAI's range)."""
    return _check_openai(f, "frequency_penalty")


def check_presence_penalty(q) -> Optional[float]:
    """None (off) or a finite number in [-2, 2] (OpenAI's range)."""
    return _check_openai(q, "presence_penalty")


def per_request(value, n: int, check, name: str) -> list:
    """``value`` - None, a number, or a sequence with one entry (number or None) per request - as a checked list of n."""
    if value is None or not isinstance(value, (Sequence, np.ndarray)) or isinstance(value, (str, bytes)):
        return [check(value)] * n
    if len(value) != n:
        raise ValueError(f"{name} must be a number or a list of {n} numbers, one per request")
    return [check(v) for v in value]


def check_penalties(repetition_penalty, frequency_penalty, presence_penalty, n: int) -> Optional[list]:
    """The (r, f, q) triple of each of n requests with the neutral value in place of None, or None when every request has the
    neutral triple (penalties off: the engines launch what they launch without the keywords)."""
    rs = per_request(repetition_penalty, n, check_repetition_penalty, "repetition_penalty")
    fs = per_request(frequency_penalty, n, check_frequency_penalty, "frequency_penalty")
    qs = per_request(presence_penalty, n, check_presence_penalty, "presence_penalty")
    out = [(NEUTRAL[0] if r is None else r, NEUTRAL[1] if f is None else f, NEUTRAL[2] if q is None else q)
           for r, f, q in zip(rs, fs, qs)]
    return None if all(t == NEUTRAL for t in out) else out


def penalize_ref(logits, prompt_ids, generated_ids, r: float = 1.0, f: float = 0.0, q: float = 0.0) -> np.ndarray:
    """Float64 reference of vis_penalize_f32 for one row -> [V].  r, f, q are rounded to f32 first (what the device sees);
    ids outside [0, V) are ignored."""
    x = np.asarray(logits, dtype=np.float64).reshape(-1)
    V = x.size
    r, f, q = (float(np.float32(t)) for t in (r, f, q))

    def inside(ids):
        a = np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids, dtype=np.int64).reshape(-1)
        return a[(a >= 0) & (a < V)]

    c = np.bincount(inside(generated_ids), minlength=V).astype(np.float64)
    seen = c > 0
    seen[inside(prompt_ids)] = True
    y = x.copy()
    if r != 1.0:
        y = np.where(seen, np.where(x < 0, x * r, x / r), x)
    return y - f * c - q * (c > 0)


def error_bound(logits, generated_ids, r: float, f: float, q: float) -> np.ndarray:
    """|vis_penalize_f32 - penalize_ref| <= 2^-23 (|x| max(r, 1 / r) + |f| c + |q|) per id.  The kernel rounds three times: the
    multiply or divide (<= 2^-24 |x| max(r, 1 / r)), f c + q as one fma (<= 2^-24 (|f| c + |q|)) and their difference
    (<= 2^-24 of a result no larger than the bracket) - together at most 2^-23 of the bracket."""
    x = np.abs(np.asarray(logits, dtype=np.float64).reshape(-1))
    V = x.size
    a = np.asarray(list(generated_ids), dtype=np.int64).reshape(-1)
    c = np.bincount(a[(a >= 0) & (a < V)], minlength=V).astype(np.float64)
    r, f, q = (float(np.float32(t)) for t in (r, f, q))
    return 2.0 ** -23 * (x * max(r, 1.0 / r) + abs(f) * c + abs(q))


class PenaltyBuffers:
    """One engine's device state of vis_penalize_f32, one row per slot (prompt passes of different slots may run on different
    streams): the token statistics, the (r, f, q) triples and the penalised logits the pick kernels read."""

    def __init__(self, slots: int, vocab: int, device):
        self.state = hip.penalty_state(vocab, slots, device)
        self.params = torch.zeros((slots, 3), dtype=torch.float32, device=device)
        self.params[:, 0] = 1.0
        self.out = torch.empty((slots, vocab), dtype=torch.float32, device=device)
        self.slots, self.vocab = slots, vocab

    def begin(self, slot: int, prompt_ids: torch.Tensor, r: float, f: float, q: float) -> None:
        """A new request in ``slot``, on the current stream ahead of its prompt pass's pick: fresh statistics, its triple,
        its prompt ids (int32 on the device) marked."""
        self.state[slot].zero_()
        for i, v in enumerate((r, f, q)):
            self.params[slot, i].fill_(float(v))
        hip.penalty_prompt(self.state[slot], self.vocab, prompt_ids)

    def apply(self, logits: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, slot: int = 0) -> torch.Tensor:
        """The penalised rows of slots slot .. slot + B - 1 (logits [V] or [B, V]; the raw rows are left intact)."""
        if logits.dim() == 2:
            B = logits.shape[0]
            out = self.out[slot:slot + B]
        else:
            B, out = 1, self.out[slot]
        hip.penalize(logits, self.state[slot:slot + B], self.params[slot:slot + B], tokens, step, out)
        return out
