"""Nucleus (top_p) sampling and per-request seeds (the ``top_p=`` / ``seeds=`` keywords of the engines' generate_batch,
``top_p=`` of generate).

While either is on, every pick - prompt pass or decode step, single or batched, eager or graph-replayed, JSON mode
included - runs vis_sample_f32: the Gumbel-max of vis_argmax_f32 restricted to the nucleus K, the shortest prefix of the
(logit desc, id asc) order that holds top_p of the temperature-scaled probability mass.  Row seeds come from a device
buffer written before the request runs: the request's own seed (mod 2^32) or the slot-derived default
``seed + 0x9E3779B9 * slot`` that vis_argmax_f32 uses, so top_p = 1 with derived seeds picks what the plain kernel picks.
``nucleus_ref`` is the float64 reference of K the tests compare the kernel against."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import hip

SLOT_SEED_STRIDE = 0x9E3779B9      # vis_argmax_f32's per-row seed offset


def check_top_p(top_p) -> Optional[float]:
    """None (off) or a real number in [0, 1]."""
    if top_p is None:
        return None
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(top_p) <= 1.0:       # NaN fails the comparison
        raise ValueError("top_p must be None or a number in [0, 1]")
    return float(top_p)


def check_seed(seed) -> Optional[int]:
    """None or an integer (used mod 2^32)."""
    if seed is None:
        return None
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("seed must be None or an integer")
    return int(seed)


def check_seeds(seeds, n: int) -> Optional[list]:
    """None or one integer seed per request."""
    if seeds is None:
        return None
    if isinstance(seeds, (str, bytes)) or not isinstance(seeds, Sequence) or len(seeds) != n:
        raise ValueError(f"seeds must be None or a list of {n} integers, one per request")
    if any(s is None for s in seeds):
        raise ValueError("seeds must hold one integer per request")
    return [check_seed(s) for s in seeds]


def row_seed(seed: int) -> int:
    """The uint32 a seed becomes on the device."""
    return int(seed) & 0xFFFFFFFF


class NucleusRef(NamedTuple):
    keep: np.ndarray     # [V] bool: the kept set K
    nkeep: int           # |K|
    order: np.ndarray    # the allowed ids by (logit desc, id asc)
    cum: np.ndarray      # cumulative mass along ``order``, divided by Z (cum[-1] == 1)


def nucleus_ref(logits, temperature: float, top_p: float, allow=None) -> NucleusRef:
    """Float64 reference of vis_sample_f32's kept set for one row.  allow: None (every id) or a [V] bool array.
    temperature 0 keeps the greedy token alone."""
    x = np.asarray(logits, dtype=np.float64).reshape(-1)
    V = x.size
    ids = np.arange(V) if allow is None else np.flatnonzero(np.asarray(allow, dtype=bool).reshape(-1)[:V])
    keep = np.zeros(V, dtype=bool)
    if ids.size == 0:
        return NucleusRef(keep, 0, ids, np.zeros(0))
    order = ids[np.lexsort((ids, -x[ids]))]          # last key primary: logit descending, then id ascending
    if temperature <= 0:
        keep[order[0]] = True
        return NucleusRef(keep, 1, order, np.ones(1))
    w = np.exp((x[order] - x[order[0]]) / float(temperature))
    cum = np.cumsum(w)
    cum /= cum[-1]
    n = V if top_p >= 1.0 else int(np.searchsorted(cum, top_p, side="left")) + 1
    n = max(1, min(n, order.size))
    keep[order[:n]] = True
    return NucleusRef(keep, n, order, cum)


class SampleBuffers:
    """One engine's device state of vis_sample_f32: the row seeds [slots] and the workspace, one row per slot, so that
    prompt passes of different slots may run on different streams."""

    def __init__(self, slots: int, vocab: int, device):
        self.seeds = torch.zeros(slots, dtype=torch.int32, device=device)
        self.ws = hip.sample_ws(vocab, slots, device)
        self.slots = slots

    def set_slot(self, slot: int, seed: int) -> None:
        """Row seed of one slot, written on the current stream ahead of its prompt pass's pick."""
        v = row_seed(seed)
        self.seeds[slot].fill_(v - (1 << 32) if v >= 1 << 31 else v)

    def pick(self, logits, tokens, cur_token, step, temperature: float, top_p: float, slot: int = 0, allow=None) -> None:
        """The pick of slots slot .. slot + B - 1."""
        B = logits.shape[0] if logits.dim() == 2 else 1
        hip.sample(logits, tokens, cur_token, step, self.seeds[slot:slot + B], self.ws[slot:slot + B], temperature,
                   1.0 if top_p is None else top_p, allow=allow)
