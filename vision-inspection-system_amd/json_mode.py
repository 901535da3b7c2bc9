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
from . import json_schema as schema
from .json_grammar import ERR, SLOT_INTS, STATE_INTS, TokenTable, build_token_table

assert STATE_INTS == hip.JSON_STATE_INTS == schema.STATE_INTS


class JsonModeError(RuntimeError):
    """The vocabulary could not continue the JSON text (no token was allowed): the request failed instead of returning text
    that is not JSON."""


class JsonBuffers:
    """One engine's device token table (built on its first JSON-mode request), grammar states [slots, 32] int32 and allowed-
    token masks [slots, ceil(V / 64)] int64."""

    def __init__(self, tokenizer, vocab: int, eos_ids, slots: int, device, share=None):
        if share is not None:       # the engine's other mask already built the token table: one table, host and device
            self.table_build_s = 0.0
            self.table, self.off, self.data, self.flags, self.eos = share.table, share.off, share.data, share.flags, share.eos
        else:
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


class SchemaBuffers(JsonBuffers):
    """JsonBuffers for a compiled schema (the ``json_schema=`` keyword): the same token table (shared with the engine's
    JsonBuffers, whichever came first), states and mask rows, plus the DFA in device tables of fixed capacity
    (SCHEMA_MAX_STATES x SCHEMA_MAX_CLASSES) and the header vis_schema_mask sizes them from.  ``load`` overwrites them per
    request group; a captured decode graph holds only their addresses, so it serves every schema."""

    def __init__(self, tokenizer, vocab: int, eos_ids, slots: int, device, share=None):
        super().__init__(tokenizer, vocab, eos_ids, slots, device, share)
        self.header = torch.zeros(schema.HEADER_INTS, dtype=torch.int32, device=device)
        # u16 bits in an int16 tensor (-1 = DEAD)
        self.trans = torch.full((schema.SCHEMA_MAX_STATES, schema.SCHEMA_MAX_CLASSES), -1, dtype=torch.int16, device=device)
        self.byte_class = torch.zeros(256, dtype=torch.uint8, device=device)
        self.state_flags = torch.zeros(schema.SCHEMA_MAX_STATES, dtype=torch.uint8, device=device)
        self.dfa = None
        # the speculative step under the schema (spec.py "grammar"): slot 0's record and allow rows of vis_schema_mask_rows,
        # and schema_draft's jump tables next to ``trans`` - overwritten with the schema, so a captured step serves the next one
        self.rows_record = torch.zeros(hip.SCHEMA_ROWS_RECORD_INTS, dtype=torch.int32, device=device)
        self.rows_allow = torch.zeros((hip.SPEC_MAX_ROWS, (vocab + 63) // 64), dtype=torch.int64, device=device)
        self.jump_tok = torch.full((schema.SCHEMA_MAX_STATES,), -1, dtype=torch.int32, device=device)
        self.jump_next = torch.full((schema.SCHEMA_MAX_STATES,), -1, dtype=torch.int32, device=device)
        self._jump_dfa = None
        self._token_index = None

    def load(self, dfa, streams=()) -> None:
        """Make ``dfa`` the schema of the launches that follow.  Called before a request group's first prompt pass, outside
        any captured graph: the copies run on the current stream once everything queued on ``streams`` (the streams that
        launched masks for the previous group) has finished, and those streams then wait for the copies."""
        if not isinstance(dfa, schema.SchemaDFA):
            raise ValueError("json_schema must be a SchemaDFA (json_schema.compile_schema)")
        n, c = dfa.trans.shape
        if not (1 <= n <= schema.SCHEMA_MAX_STATES and 1 <= c <= schema.SCHEMA_MAX_CLASSES and 0 <= dfa.start < n):
            raise ValueError(f"json_schema: {n} states x {c} classes exceed the device tables "
                             f"({schema.SCHEMA_MAX_STATES} x {schema.SCHEMA_MAX_CLASSES})")
        if dfa.trans.dtype != schema.np.uint16 or dfa.byte_class.shape != (256,) or dfa.state_flags.shape != (n,) \
                or int(dfa.byte_class.max()) >= c or bool(((dfa.trans >= n) & (dfa.trans != schema.DEAD)).any()):
            raise ValueError("json_schema: inconsistent DFA tables")
        if dfa is self.dfa:
            return
        cur = torch.cuda.current_stream(self.header.device)
        for s in streams:
            cur.wait_stream(s)
        packed = torch.from_numpy(schema.np.ascontiguousarray(dfa.trans).reshape(-1).view(schema.np.int16))
        self.trans.view(-1)[:n * c].copy_(packed)
        self.byte_class.copy_(torch.from_numpy(schema.np.ascontiguousarray(dfa.byte_class)))
        self.state_flags[:n].copy_(torch.from_numpy(schema.np.ascontiguousarray(dfa.state_flags)))
        self.header.copy_(torch.tensor([n, c, dfa.start, 0], dtype=torch.int32))
        for s in streams:
            s.wait_stream(cur)
        self.dfa = dfa

    def mask(self, tokens: torch.Tensor, step: torch.Tensor, slot: int = 0) -> torch.Tensor:
        """vis_schema_mask for slots slot .. slot + B - 1 (tokens [B, T] or [T], step [B]); returns their mask rows."""
        t2 = tokens if tokens.dim() == 2 else tokens.view(1, -1)
        B = t2.shape[0]
        hip.schema_mask(self.state[slot:slot + B], t2, step, self.off, self.data, self.flags, self.eos,
                        self.allow[slot:slot + B], self.header, self.trans, self.byte_class, self.state_flags)
        return self.allow[slot:slot + B]

    def failed(self, slots) -> list:
        st = self.state.cpu()
        return [bool(st[s, schema.ERR] or st[s, schema.SLOT_INTS + schema.ERR]) for s in slots]

    # ---- the speculative step of slot 0 under the schema
    def begin_rows(self, start: int, drafts: bool) -> None:
        """Behind the prompt pass's masked pick of a speculative request: the rows record says "the start state in front of
        tokens[start]" (the pick's own index), and with ``drafts`` the loaded schema's jump tables are on the device
        (built once per schema and vocabulary).  Outside any captured graph."""
        self.rows_record.copy_(torch.tensor([0, 0, start, 0] + [0] * (hip.SCHEMA_ROWS_RECORD_INTS - 4), dtype=torch.int32))
        if drafts and self._jump_dfa is not self.dfa:
            from . import schema_draft
            if self._token_index is None:
                self._token_index = schema_draft.token_index(self.table)
            t = schema_draft.build(self.dfa, self.table, self._token_index)
            self.jump_tok.copy_(torch.from_numpy(t.jump_tok))
            self.jump_next.copy_(torch.from_numpy(t.jump_next))
            self._jump_dfa = self.dfa

    def mask_rows(self, tokens: torch.Tensor, step: torch.Tensor, draft: torch.Tensor, n_draft: torch.Tensor,
                  rows: int) -> torch.Tensor:
        """vis_schema_mask_rows for the ``rows`` rows of slot 0's step; returns them."""
        allow = self.rows_allow[:rows]
        hip.schema_mask_rows(self.rows_record, tokens, step, draft, n_draft, self.off, self.data, self.flags, self.eos, allow,
                             self.header, self.trans, self.byte_class, self.state_flags)
        return allow

    def draft(self, tokens: torch.Tensor, step: torch.Tensor, k: int, draft: torch.Tensor, n_draft: torch.Tensor) -> None:
        """vis_spec_draft_schema behind the accept of slot 0's step (or behind the prompt pass's pick)."""
        hip.spec_draft_schema(self.rows_record, tokens, step, self.off, self.data, self.flags, self.header, self.trans,
                              self.byte_class, self.state_flags, self.jump_tok, self.jump_next, k, draft, n_draft)

    def reply_failed(self, toks, ended_on_eos: bool) -> bool:
        """The failure outcome of a speculative reply, decided as the plain loop's error bit is: a reply the vocabulary
        could not continue took a forced EOS in a state that does not accept, and the fold sets the bit for exactly that
        token - one json_schema.advance over the returned tokens, and, where the reply was cut in front of the EOS that
        ended it, that EOS."""
        st = schema.initial_state(self.dfa)
        for t in toks:
            schema.advance(self.dfa, st, int(t), self.table)
            if st[1]:
                return True
        return ended_on_eos and not self.dfa.state_flags[st[0]] & schema.STATE_ACCEPT


def engine_tokenizer(engine):
    tok = getattr(engine, "tokenizer", None)
    if tok is None or not hasattr(tok, "token_bytes"):
        raise ValueError("json_mode needs the engine's tokenizer (engine.tokenizer with token_bytes); "
                         "the client sets it when it loads a model")
    return tok


def check_schema(json_mode, json_schema) -> None:
    """Argument check of the engines' ``json_schema=`` keyword (None = off)."""
    if json_schema is None:
        return
    if not isinstance(json_schema, schema.SchemaDFA):
        raise ValueError("json_schema must be a SchemaDFA (json_schema.compile_schema) or None")
    if json_mode:
        raise ValueError("json_mode and json_schema are two grammars for one reply: give one of them")

