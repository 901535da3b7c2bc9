"""JSON mode on the device (the ``json_mode=`` keyword of the engines' generate / generate_batch).

Before every pick of a JSON-mode request - prompt pass or decode step, single or batched, eager or graph-replayed - the
engine launches vis_json_mask (fold the tokens picked since the last launch into the sequence's grammar state, write the
bitmask of the tokens the grammar allows next) and then the masked form of its pick (vis_argmax_masked_f32, or
vis_gemv_bf16_argmax_masked in the fused lm_head epilogue).  The grammar is json_grammar's.  State and mask have one row
per slot, so prompt passes of different slots may run on different streams; a slot's state is zeroed before its prompt
pass, outside any captured graph."""
from __future__ import annotations

import time

import torch

from . import hip
from .json_grammar import ERR, SLOT_INTS, STATE_INTS, TokenTable, build_token_table

assert STATE_INTS == hip.JSON_STATE_INTS


class JsonModeError(RuntimeError):
    """The vocabulary could not continue the JSON text (no token was allowed): the request failed instead of returning text
    that is not JSON."""


class JsonBuffers:
    """One engine's device token table (built on its first JSON-mode request), grammar states [slots, 32] int32 and allowed-
    token masks [slots, ceil(V / 64)] int64."""

    def __init__(self, tokenizer, vocab: int, eos_ids, slots: int, device):
        t0 = time.perf_counter()
        table = build_token_table(tokenizer, vocab, eos_ids)
        self.table_build_s = time.perf_counter() - t0      # host side; reported by tools/json_mode_bench.py
        self.table: TokenTable = table
        self.off = torch.from_numpy(table.off).to(device)
        self.data = torch.from_numpy(table.data).to(device)
        self.flags = torch.from_numpy(table.flags).to(device)
        self.eos = torch.from_numpy(table.eos_ids).to(device)
        self.state = torch.zeros((slots, STATE_INTS), dtype=torch.int32, device=device)
        self.allow = torch.zeros((slots, (vocab + 63) // 64), dtype=torch.int64, device=device)

    def reset(self, slot: int) -> None:
        """A fresh grammar state for ``slot`` (on the current stream, before the slot's prompt-pass pick)."""
        self.state[slot].zero_()

    def mask(self, tokens: torch.Tensor, step: torch.Tensor, slot: int = 0) -> torch.Tensor:
        """vis_json_mask for slots slot .. slot + B - 1 (tokens [B, T] or [T], step [B]); returns their mask rows."""
        t2 = tokens if tokens.dim() == 2 else tokens.view(1, -1)
        B = t2.shape[0]
        hip.json_mask(self.state[slot:slot + B], t2, step, self.off, self.data, self.flags, self.eos,
                      self.allow[slot:slot + B])
        return self.allow[slot:slot + B]

    def failed(self, slots) -> list:
        """Error bit of each slot (either state slot: the bit is sticky); synchronises."""
        st = self.state.cpu()
        return [bool(st[s, ERR] or st[s, SLOT_INTS + ERR]) for s in slots]


def engine_tokenizer(engine):
    tok = getattr(engine, "tokenizer", None)
    if tok is None or not hasattr(tok, "token_bytes"):
        raise ValueError("json_mode needs the engine's tokenizer (engine.tokenizer with token_bytes); "
                         "the client sets it when it loads a model")
    return tok
