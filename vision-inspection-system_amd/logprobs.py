"""Token log-probabilities of generated tokens (the ``logprobs=`` keyword of the engines' generate / generate_batch).

After every pick - prompt pass or decode step, single or batched, eager or graph-replayed - the engine launches
vis_logprobs_f32 on the step's logits: the log-softmax of the RAW logits (temperature 1, no Gumbel noise; vLLM's default
"raw logprobs"), so the same prefix gives the same numbers at every temperature.  Results stay on the device, indexed by
absolute position like the token buffer, until the request ends."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip

MAX_TOP_LOGPROBS = hip.LOGPROBS_MAX_K


class TokenLogprobs(NamedTuple):
    """One request's record, cut like its returned token list (n == len(tokens))."""
    token_logprobs: np.ndarray    # [n] f32: log-probability of each returned token
    top_ids: np.ndarray           # [n, k] int32: the k most likely tokens at that position, most likely first
    top_logprobs: np.ndarray      # [n, k] f32: their log-probabilities


def check_k(logprobs: Optional[int]) -> Optional[int]:
    """None (off) or the number of alternatives per token, 0..20."""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or not 0 <= logprobs <= MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs must be None or an integer in 0..{MAX_TOP_LOGPROBS}")
    return int(logprobs)


class LogprobsBuffers:
    """Device buffers of one engine: lp [slots, T, 21] f32, top_ids [slots, T, 20] int32 (T = the token buffer's length) and
    the kernel's workspace, one row per slot, so that prompt passes of different slots may run on different streams."""

    def __init__(self, slots: int, max_tokens: int, vocab: int, device):
        k = MAX_TOP_LOGPROBS
        self.lp = torch.zeros((slots, max_tokens, k + 1), dtype=torch.float32, device=device)
        self.top_ids = torch.zeros((slots, max_tokens, k), dtype=torch.int32, device=device)
        self.ws = hip.logprobs_ws(vocab, slots, device)

    def launch(self, logits: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, k: int, slot: int = 0) -> None:
        """After the pick of slots slot .. slot + B - 1 (logits [B, V], tokens [B, T], step [B])."""
        B = logits.shape[0]
        hip.logprobs(logits, tokens, step, k, self.lp[slot:slot + B], self.top_ids[slot:slot + B], self.ws[slot:slot + B])

    def record(self, slot: int, start: int, n: int, k: int) -> TokenLogprobs:
        """Positions start .. start + n - 1 of ``slot`` (call after the stream has drained)."""
        lp = self.lp[slot, start:start + n].cpu().numpy()
        ids = self.top_ids[slot, start:start + n, :k].cpu().numpy()
        return TokenLogprobs(lp[:, 0].copy(), ids.copy(), lp[:, 1:1 + k].copy())
