"""Logit shaping (the ``top_k=`` / ``min_p=`` / ``logit_bias=`` keywords of the engines' generate and generate_batch).

While any of them is on, every pick - prompt pass or decode step, single or batched, eager or graph-replayed, JSON mode,
nucleus sampling and penalties included - is handed the row vis_shape_f32 wrote instead of the logits it would have read.
For one sequence with logits x (the penalised row while penalties are on) and allowed set A (every id, or the grammar mask's):

    y[v] = x[v] + logit_bias[v]              (OpenAI's logit_bias: one f32 add on the ids named, before temperature)
    t    = the top_k-th largest y over A     (transformers' TopKLogitsWarper: ties at t all stay; k >= |A| cuts nothing)
    m    = max y over A
    keep = v in A and y[v] >= t and not (y[v] - m) < delta,   delta = float32(ln(min_p) / inv_temp)
                                             (transformers' MinPLogitsWarper: p[v] >= min_p * p[max] in the logit domain)
    out[v] = y[v] if keep else -inf

and the pick that follows (the Gumbel argmax, or top_p's cut and draw) sees only the survivors.  A greedy request is
affected by logit_bias alone.  The raw row stays where it is (logprobs keep reading it).  k, delta and the bias list live in
device memory, one row per slot, so requests of one batch may differ and a captured decode graph serves any values.
``reference_shape`` is the numpy restatement the tests compare the kernel against, bit for bit."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .penalties import per_request

MAX_BIAS = hip.SHAPE_MAX_BIAS       # OpenAI's limit for logit_bias
NEUTRAL = (None, None, None)        # (top_k, min_p, bias list) of a request that asks for none of them


def check_top_k(k) -> Optional[int]:
    """None (off) or an integer >= 1."""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError("top_k must be None or an integer >= 1")
    return int(k)


def check_min_p(min_p) -> Optional[float]:
    """None (off) or a real number in [0, 1]."""
    if min_p is None:
        return None
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(min_p) <= 1.0:       # NaN fails the comparison
        raise ValueError("min_p must be None or a number in [0, 1]")
    return float(min_p)


def check_logit_bias(logit_bias, vocab: Optional[int] = None) -> Optional[Tuple[Tuple[int, float], ...]]:
    """None (off) or a dict of at most 300 entries {token id: bias}: ids are ints or decimal strings (OpenAI's JSON keys) in
    [0, vocab), distinct after conversion; values are finite numbers in [-100, 100].  Returns ((id, bias), ...) in the
    dict's order, or None for None and for an empty dict.  vocab None: only id >= 0 is asked here and the upper bound
    when the request is switched on (check_vocab) - the engines check their arguments before they look at the model."""
    if logit_bias is None:
        return None
    if not isinstance(logit_bias, dict):
        raise ValueError("logit_bias must be None or a dict {token id: bias}")
    if len(logit_bias) > MAX_BIAS:
        raise ValueError(f"logit_bias holds {len(logit_bias)} entries, at most {MAX_BIAS} are allowed")
    out, seen = [], set()
    for key, val in logit_bias.items():
        if isinstance(key, str) and key.isascii() and key.isdigit():
            tid = int(key)
        elif not isinstance(key, bool) and isinstance(key, (int, np.integer)):
            tid = int(key)
        else:
            raise ValueError(f"logit_bias: token id {key!r} is not an integer or a decimal string")
        if tid < 0 or (vocab is not None and tid >= vocab):
            raise ValueError(f"logit_bias: token id {tid} is outside the vocabulary [0, {'...' if vocab is None else vocab})")
        if tid in seen:
            raise ValueError(f"logit_bias: token id {tid} is given twice")
        seen.add(tid)
        if isinstance(val, bool) or not isinstance(val, (int, float, np.integer, np.floating)) \
                or not -100.0 <= float(val) <= 100.0:    # NaN and the infinities fail the comparison
            raise ValueError(f"logit_bias: the bias of token {tid} must be a finite number in [-100, 100]")
        out.append((tid, float(val)))
    return tuple(out) or None


def _biases(value, n: int, vocab: Optional[int]) -> list:
    """``logit_bias`` of a group - None, one dict for all, or a sequence with one entry (dict or None) per request."""
    if value is None or isinstance(value, dict):
        return [check_logit_bias(value, vocab)] * n
    if isinstance(value, (str, bytes)) or not isinstance(value, Sequence) or len(value) != n:
        raise ValueError(f"logit_bias must be a dict or a list of {n} dicts, one per request")
    return [check_logit_bias(v, vocab) for v in value]


def check_shaping(top_k, min_p, logit_bias, n: int, vocab: Optional[int] = None) -> Optional[list]:
    """The (top_k, min_p, bias list) of each of n requests - each keyword one value for the group or one per request - or
    None when no request asks for any of them (shaping off: the engines launch what they launch without the keywords).
    min_p = 0 and an empty dict are the off values; top_k has none (an integer >= 1 is a request to cut)."""
    ks = per_request(top_k, n, check_top_k, "top_k")
    ps = [p or None for p in per_request(min_p, n, check_min_p, "min_p")]
    bs = _biases(logit_bias, n, vocab)
    out = list(zip(ks, ps, bs))
    return None if all(t == NEUTRAL for t in out) else out


def check_vocab(shaping: Optional[list], vocab: int) -> None:
    """The upper bound of the bias ids of check_shaping's result, for a caller that checked without a vocabulary size."""
    for _, _, bias in shaping or ():
        for tid, _ in bias or ():
            if tid >= vocab:
                raise ValueError(f"logit_bias: token id {tid} is outside the vocabulary [0, {vocab})")


def shaping_kwargs(shaping: Optional[list]) -> dict:
    """The first request of check_shaping's result as the keywords of a single-request call ({} when off)."""
    if shaping is None:
        return {}
    k, p, bias = shaping[0]
    return {"top_k": k, "min_p": p, "logit_bias": dict(bias) if bias else None}


def min_p_delta(min_p: Optional[float], temperature: float) -> float:
    """delta = float32(ln(min_p) / inv_temp) with inv_temp = 1 / temperature as the pick kernels get it; -inf (off) for
    min_p None or 0 and for a greedy request."""
    if not min_p or not temperature > 0:
        return -math.inf
    return float(np.float32(math.log(float(min_p)) / (1.0 / float(temperature))))


class ShapeRef(NamedTuple):
    out: np.ndarray      # [V] f32: y for survivors, -inf elsewhere
    nkept: int


def reference_shape(logits, k: int = 0, delta: float = -math.inf, bias: Sequence[Tuple[int, float]] = (), allow=None) -> ShapeRef:
    """vis_shape_f32 for one row in numpy, bit for bit.  k: 0 = off; delta: min_p_delta's value; bias: (id, value) pairs (ids
    outside [0, V) are skipped, the first entry of an id counts); allow: None (every id) or a [V] bool array."""
    x = np.asarray(logits, dtype=np.float32).reshape(-1)
    V = x.size
    y = x.copy()
    done = set()
    for tid, val in bias:
        if 0 <= tid < V and tid not in done:
            done.add(tid)
            y[tid] = np.float32(x[tid] + np.float32(val))
    in_a = np.ones(V, dtype=bool) if allow is None else np.asarray(allow, dtype=bool).reshape(-1)[:V].copy()
    out = np.full(V, -np.inf, dtype=np.float32)
    n_a = int(in_a.sum())
    if n_a == 0:
        return ShapeRef(out, 0)
    ya = y[in_a]
    keep = in_a.copy()
    if 0 < k < n_a:
        t = np.sort(ya)[n_a - k]                         # the k-th largest; float order: both zeros compare equal
        keep &= y >= t
    delta = np.float32(delta)
    if delta > -np.inf:
        m = ya.max()
        keep &= ~((y - m).astype(np.float32) < delta)
    out[keep] = y[keep]
    return ShapeRef(out, int(keep.sum()))


class ShapeBuffers:
    """One engine's device state of vis_shape_f32, one row per slot (prompt passes of different slots may run on different
    streams): the parameters (k, delta, the bias list), the shaped logits the pick kernels read, the survivor counts and the
    workspace with the launch's record per row."""

    def __init__(self, slots: int, vocab: int, device):
        self.k = torch.zeros(slots, dtype=torch.int32, device=device)
        self.delta = torch.full((slots,), -math.inf, dtype=torch.float32, device=device)
        self.nbias = torch.zeros(slots, dtype=torch.int32, device=device)
        self.bias_ids = torch.zeros((slots, MAX_BIAS), dtype=torch.int32, device=device)
        self.bias_vals = torch.zeros((slots, MAX_BIAS), dtype=torch.float32, device=device)
        self.out = torch.empty((slots, vocab), dtype=torch.float32, device=device)
        self.nkept = torch.zeros(slots, dtype=torch.int32, device=device)
        self.ws = hip.shape_ws(vocab, slots, device)
        self.slots, self.vocab = slots, vocab

    def begin(self, slot: int, top_k: Optional[int], min_p: Optional[float], bias, temperature: float) -> None:
        """A new request in ``slot``, on the current stream ahead of its prompt pass's pick: its k, its delta at the
        temperature it runs at, and its bias list (check_logit_bias' result or None)."""
        self.k[slot].fill_(min(int(top_k), self.vocab) if top_k else 0)
        self.delta[slot].fill_(min_p_delta(min_p, temperature))
        bias = bias or ()
        self.nbias[slot].fill_(len(bias))
        if bias:
            ids = torch.tensor([b[0] for b in bias], dtype=torch.int32)
            vals = torch.tensor([b[1] for b in bias], dtype=torch.float32)
            self.bias_ids[slot, :len(bias)].copy_(ids)
            self.bias_vals[slot, :len(bias)].copy_(vals)

    def apply(self, logits: torch.Tensor, slot: int = 0, allow: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The shaped rows of slots slot .. slot + B - 1 (logits [V] or [B, V]; left intact)."""
        if logits.dim() == 2:
            B = logits.shape[0]
            out = self.out[slot:slot + B]
        else:
            B, out = 1, self.out[slot]
        s = slice(slot, slot + B)
        hip.shape_logits(logits, self.k[s], self.delta[s], self.nbias[s], self.bias_ids[s], self.bias_vals[s], out,
                         self.nkept[s], self.ws[s], allow=allow)
        return out
