"""Lossless n-gram speculative decoding of one greedy request: the request's switch and what it excludes, the prompt-lookup
drafter as a numpy reference (``propose``; vis_spec_draft equals it exactly), a numpy restatement of the accept step
(``accept_ref``; vis_spec_accept), and the device buffers of the speculative step (DecodeStage._decode_step_spec).

A step feeds R = 1 + k rows - the current token and up to k drafted ones - through every projection in ONE pass over the
weights (vis_gemv_*_rows: each row's arithmetic is the single-row kernel's, bit for bit) and through
vis_decode_attn_draft (row r bit-identical to a plain attention launch at its position).  Row r's logits therefore are
the logits the plain step would have computed after the drafts in front of it - when those drafts are what the plain
step would have picked.  The accept step keeps exactly that prefix, so the reply is the plain reply token for token."""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

MAX_K = 3            # R = k + 1 <= 4 rows: the bound of the multi-row GEMVs (hip.SPEC_MAX_ROWS)
MAX_LOOKUP = 8       # hip.SPEC_MAX_LOOKUP
ROWS_LDS_MAX = 152 * 1024      # GV_ROWS_LDS_MAX of csrc/decode.hip: the input rows of a multi-row GEMV live in LDS


class SpecConfig(NamedTuple):
    k: int               # num_speculative_tokens
    lookup_max: int      # prompt_lookup_max
    lookup_min: int      # prompt_lookup_min

    @property
    def rows(self) -> int:
        return self.k + 1


def _int(v, name: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"speculative: {name} must be an integer in {lo}..{hi}")
    return v


def check_speculative(speculative) -> Optional[SpecConfig]:
    """None (off), the integer k, or {"method": "ngram", "num_speculative_tokens": k[, "prompt_lookup_max": 4,
    "prompt_lookup_min": 2]} (vLLM's names) -> SpecConfig or None; ValueError otherwise."""
    if speculative is None:
        return None
    if isinstance(speculative, SpecConfig):
        speculative = {"method": "ngram", "num_speculative_tokens": speculative.k, "prompt_lookup_max": speculative.lookup_max,
                       "prompt_lookup_min": speculative.lookup_min}
    if isinstance(speculative, int) and not isinstance(speculative, bool):
        speculative = {"method": "ngram", "num_speculative_tokens": speculative}
    if not isinstance(speculative, dict):
        raise ValueError("speculative must be None, an integer k or a dict with 'method' and 'num_speculative_tokens'")
    unknown = set(speculative) - {"method", "num_speculative_tokens", "prompt_lookup_max", "prompt_lookup_min"}
    if unknown:
        raise ValueError(f"speculative: unknown keys {sorted(unknown)}")
    if speculative.get("method", "ngram") != "ngram":
        raise ValueError("speculative: the only method is 'ngram' (prompt lookup; there is no draft model)")
    if "num_speculative_tokens" not in speculative:
        raise ValueError("speculative: num_speculative_tokens is required")
    k = _int(speculative["num_speculative_tokens"], "num_speculative_tokens", 1, MAX_K)
    hi = _int(speculative.get("prompt_lookup_max", 4), "prompt_lookup_max", 1, MAX_LOOKUP)
    lo = _int(speculative.get("prompt_lookup_min", min(2, hi)), "prompt_lookup_min", 1, hi)
    return SpecConfig(k, hi, lo)


def check_exclusive(cfg: Optional[SpecConfig], temperature: float = 0.0, seed=None, **switches) -> None:
    """What a speculative request may not carry: every switch that is a per-step device state machine advancing one token
    at a time, and everything that samples.  ``switches``: name -> value as the caller got it (None / neutral = off).
    ValueError naming the conflict."""
    if cfg is None:
        return
    if temperature:
        raise ValueError("speculative together with temperature > 0 is not supported: acceptance is defined for the greedy pick")
    if seed:
        raise ValueError("speculative together with a seed is not supported: a greedy request has nothing to seed")
    neutral = {"top_p": (None, 1, 1.0), "repetition_penalty": (None, 1, 1.0), "frequency_penalty": (None, 0, 0.0),
               "presence_penalty": (None, 0, 0.0), "top_k": (None, 0), "min_p": (None, 0, 0.0), "logit_bias": (None, {}),
               "no_repeat_ngram_size": (None, 0), "bad_words": (None, [], ()), "min_tokens": (None, 0),
               "json_mode": (None, False), "json_schema": (None,), "response_format": (None, {"type": "text"}), "stop": (None, [], ()),
               "stream": (None, False), "on_stream": (None,), "logprobs": (None, False), "top_logprobs": (None,),
               "n": (None, 1), "seeds": (None,)}
    for name, value in switches.items():
        off = neutral.get(name, (None,))
        if not any(value is o or (type(value) is type(o) and value == o) for o in off):
            raise ValueError(f"speculative together with {name} is not supported: it is a per-step state of the pick, and a "
                             "speculative step yields several tokens")


def from_env() -> Optional[SpecConfig]:
    """VIS_SPECULATIVE=k (1..3; unset, empty or 0 = off): the agents pass it on requests without an excluded switch."""
    v = os.environ.get("VIS_SPECULATIVE", "").strip()
    if v in ("", "0"):
        return None
    try:
        k = int(v)
    except ValueError:
        raise ValueError("VIS_SPECULATIVE must be an integer in 0..3") from None
    return check_speculative(k)


def check_rows_fit(cfg_model, rows: int) -> None:
    """The multi-row GEMVs keep their input rows in LDS: the widest projection input of the model must fit."""
    width = max(cfg_model.intermediate, cfg_model.hidden)
    if width * 2 * (1 if rows == 1 else 2 if rows == 2 else 4) > ROWS_LDS_MAX:
        raise ValueError(f"speculative: {rows} rows of {width} inputs do not fit the multi-row GEMV's LDS")


# ----------------------------------------------------------------------------------------------------- references
def propose(history: Sequence[int], k: int, lookup_max: int = 4, lookup_min: int = 2) -> List[int]:
    """Prompt lookup: for m from lookup_max down to lookup_min, the LATEST earlier occurrence of the last m ids of
    ``history`` that has at least one id behind it; the first m that has one gives the up to k ids that followed it.
    No match: []."""
    h = list(history)
    L = len(h)
    for m in range(lookup_max, lookup_min - 1, -1):
        if L <= m:
            continue
        tail = h[L - m:]
        for j in range(L - m - 1, -1, -1):
            if h[j:j + m] == tail:
                return h[j + m:j + m + k]
    return []


def accept_ref(logits: np.ndarray, draft: Sequence[int], d: int, step: int, limit: int, tokens: np.ndarray,
               counters: Sequence[int]):
    """vis_spec_accept restated: returns (tokens, cur_token or None, step, counters) after the call."""
    tokens, counters = np.array(tokens), list(counters)
    R = logits.shape[0]
    if step < 0 or step > min(limit, len(tokens) - 1):
        return tokens, None, step, counters
    # np.argmax ignores nothing: restate the comparison (first maximum among the comparable values)
    picks = []
    for r in range(R):
        row = np.asarray(logits[r], dtype=np.float32)
        ok = ~np.isnan(row)
        picks.append(int(np.flatnonzero(ok & (row == row[ok].max()))[0]) if ok.any() else 0)
    d = min(max(d, 0), R - 1)
    a = 0
    while a < d and draft[a] == picks[a]:
        a += 1
    a = min(a, min(limit, len(tokens) - 1) - step)
    tokens[step:step + a + 1] = picks[:a + 1]
    return tokens, picks[a], step + a + 1, [counters[0] + 1, counters[1] + d, counters[2] + a]


# --------------------------------------------------------------------------------------------------- device buffers
class SpecBuffers:
    """What the speculative step of one engine owns: its own activation rows (an engine built with max_batch=1 has no
    batched buffers), the attention workspace for 4 rows, the f32 logits of 4 rows, the id row [cur, drafts], the request's
    prompt ids and the small device ints the launches read (draft count, limit, prompt length, start of the reply in the
    token row, counters)."""

    def __init__(self, cfg, n_split: int, max_ctx: int, device):
        bf, dev, R = torch.bfloat16, device, MAX_K + 1
        nq = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        self.x = torch.empty((R, cfg.hidden), dtype=bf, device=dev)
        self.x2 = torch.empty((R, cfg.hidden), dtype=bf, device=dev)
        self.qkv = torch.empty((R, nq), dtype=bf, device=dev)
        self.attn = torch.zeros((R, cfg.heads * cfg.head_dim), dtype=bf, device=dev)     # a row past the cache is never written
        self.act = torch.empty((R, cfg.intermediate), dtype=bf, device=dev)
        self.logits = torch.empty((R, cfg.vocab), dtype=torch.float32, device=dev)
        self.part_o = torch.empty(R * cfg.heads * n_split * cfg.head_dim, dtype=torch.float32, device=dev)
        self.part_ml = torch.empty(R * cfg.heads * n_split * 2, dtype=torch.float32, device=dev)
        self.ws_val = torch.empty(256 * R, dtype=torch.float32, device=dev)
        self.ws_idx = torch.empty(256 * R, dtype=torch.int32, device=dev)
        self.ids = torch.zeros(R, dtype=torch.int32, device=dev)           # [cur, draft 0 .. draft k-1]
        self.prompt = torch.zeros(max_ctx, dtype=torch.int32, device=dev)
        ints = torch.zeros(8, dtype=torch.int32, device=dev)
        self.n_draft, self.limit, self.prompt_len, self.gen_start = ints[0:1], ints[1:2], ints[2:3], ints[3:4]
        self.counters = ints[4:7]                                           # steps, proposed, accepted
        self._ints = ints

    @property
    def cur(self) -> torch.Tensor:
        return self.ids[0:1]

    @property
    def draft(self) -> torch.Tensor:
        return self.ids[1:]

    def begin(self, cur_token: torch.Tensor, prompt_ids: torch.Tensor, step0: int, limit: int) -> None:
        """A request starts behind its prompt pass: the first token, the prompt's ids, no drafts yet, counters at zero.
        ``step0``: the index of the token row the prompt pass's pick went to; ``limit``: the last one the reply may use."""
        n = prompt_ids.numel()
        self.prompt[:n].copy_(prompt_ids)
        self.ids.zero_()
        self.ids[0:1].copy_(cur_token)
        self._ints.copy_(torch.tensor([0, limit, n, step0, 0, 0, 0, 0], dtype=torch.int32), non_blocking=False)

    def read_counters(self) -> List[int]:
        return [int(v) for v in self.counters.cpu().tolist()]
