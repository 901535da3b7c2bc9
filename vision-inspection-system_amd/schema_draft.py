"""The schema as a drafter of the speculative step (spec.py "grammar" / "schema_drafts"): host tables and the numpy
definitions the device launch (vis_spec_draft_schema) must equal.

A large share of a schema-constrained reply is decided before the model is asked: key names in fixed order, punctuation,
the tail of an enum literal once its first bytes are out.  The compiled DFA (json_schema.SchemaDFA) knows these bytes:
wherever a state has ONE live byte, that byte is the reply's next byte.  Where whitespace is the only alternative the
compact spelling is taken - a guess the model may decline, in which case the draft is simply not accepted.

``build`` turns this into two int32 tables over the DFA's states for one vocabulary: ``jump_tok[s]``, the longest token
that spells a non-empty prefix of the forced path P(s), and ``jump_next[s]``, the state behind it.  A draft is a walk
through the tables (``propose``): no lookup, no history, and it exists from the reply's first token on.  ``simulate`` walks
a plain reply the way the speculative steps take it and gives the counters a run must report."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import json_schema as S
from . import spec
from .json_grammar import FLAG_EOS, TokenTable

MAX_PATH = 48        # bytes of a forced path: longer than any token worth drafting in one jump
_WS = (0x20, 0x09, 0x0A, 0x0D)


class DraftTables(NamedTuple):
    jump_tok: np.ndarray       # int32 [SCHEMA_MAX_STATES]: token id, -1 = no draft in this state (and for states past n_states)
    jump_next: np.ndarray      # int32 [SCHEMA_MAX_STATES]: the DFA state behind that token, -1 where jump_tok is


def forced_bytes(dfa: S.SchemaDFA) -> np.ndarray:
    """int32 [n_states]: the byte a state forces, -1 where it forces none.  With L the bytes that have a live transition:
    the one byte of L; else the one byte of L that is no JSON whitespace, when L also held whitespace (the compact
    spelling).  An accepting state forces nothing."""
    live = dfa.trans[:, dfa.byte_class] != S.DEAD                      # [n_states, 256]
    ws = np.zeros(256, dtype=bool)
    ws[list(_WS)] = True
    n_all, n_ws = live.sum(axis=1), (live & ws).sum(axis=1)
    solid = live & ~ws
    first_all, first_solid = live.argmax(axis=1), solid.argmax(axis=1)
    out = np.where(n_all == 1, first_all, np.where((n_all - n_ws == 1) & (n_ws > 0), first_solid, -1)).astype(np.int32)
    out[(dfa.state_flags & S.STATE_ACCEPT) != 0] = -1
    return out


def forced_path(dfa: S.SchemaDFA, state: int, forced: Optional[np.ndarray] = None) -> bytes:
    """P(state): forced bytes from ``state`` on, until a state forces none, is accepting or was visited, or MAX_PATH bytes."""
    forced = forced_bytes(dfa) if forced is None else forced
    out, seen, s = bytearray(), set(), int(state)
    while len(out) < MAX_PATH and s not in seen and forced[s] >= 0:
        seen.add(s)
        out.append(int(forced[s]))
        s = int(dfa.trans[s, dfa.byte_class[out[-1]]])
    return bytes(out)


def token_index(table: TokenTable) -> dict:
    """bytes -> the lowest id of a non-EOS token with those (non-empty) bytes."""
    index: dict = {}
    for t in range(table.vocab - 1, -1, -1):
        b = table.tokens[t]
        if b and not table.flags[t] & FLAG_EOS:
            index[b] = t
    return index


def build(dfa: S.SchemaDFA, table: TokenTable, index: Optional[dict] = None) -> DraftTables:
    """The jump tables of ``dfa`` over ``table``'s vocabulary.  ``index``: token_index(table), when the caller keeps it."""
    index = token_index(table) if index is None else index
    forced = forced_bytes(dfa)
    longest = max((len(b) for b in index), default=0)
    jump_tok = np.full(S.SCHEMA_MAX_STATES, -1, dtype=np.int32)
    jump_next = np.full(S.SCHEMA_MAX_STATES, -1, dtype=np.int32)
    for s in range(dfa.n_states):
        if forced[s] < 0:
            continue
        path = forced_path(dfa, s, forced)
        for n in range(min(len(path), longest), 0, -1):
            t = index.get(path[:n])
            if t is not None:
                jump_tok[s], jump_next[s] = t, S.walk(dfa, s, path[:n])
                break
    return DraftTables(jump_tok, jump_next)


def propose(dfa: S.SchemaDFA, tables: DraftTables, state: int, k: int) -> List[int]:
    """The drafts in DFA state ``state``: jump_tok / jump_next followed up to k times, ending at the first -1."""
    out, s = [], int(state)
    while len(out) < k and 0 <= s < dfa.n_states and tables.jump_tok[s] >= 0:
        out.append(int(tables.jump_tok[s]))
        s = int(tables.jump_next[s])
    return out


def simulate(dfa: S.SchemaDFA, tables: DraftTables, table: TokenTable, reply_ids: Sequence[int], cfg: "spec.SpecConfig",
             prompt: Sequence[int] = (), max_new_tokens: Optional[int] = None) -> dict:
    """What a run with ``speculative=cfg`` (``grammar`` on) must report, without a model: the scheme is lossless, so the pick
    behind any accepted prefix is the plain reply's next token.  ``reply_ids``: the plain schema-constrained reply, run to
    its length limit.  Each step's drafts are the prompt lookup's over ``prompt`` + reply (spec.propose), replaced by the
    schema's (``propose`` in the state behind the reply so far) where ``cfg.schema_drafts`` is on and it has any.  Returns
    {"reply", "spec_steps", "spec_proposed", "spec_accepted", "schema_proposed"} (the last: drafts that came from the schema)."""
    plain = [int(t) for t in reply_ids]
    N = len(plain) if max_new_tokens is None else min(len(plain), max_new_tokens)
    st, folded = S.initial_state(dfa), 0
    steps = proposed = accepted = from_schema = 0
    n = 1
    while True:
        for t in plain[folded:n]:
            S.advance(dfa, st, t, table)
        folded = n
        draft = spec.propose(list(prompt) + plain[:n], cfg.k, cfg.lookup_max, cfg.lookup_min)
        draft = [min(max(t, 0), table.vocab - 1) for t in draft]
        own = propose(dfa, tables, st[0], cfg.k) if cfg.schema_drafts and not st[1] else []
        if own:
            draft = own
        if n >= N:
            break
        a = 0
        while a < len(draft) and n + a < N - 1 and draft[a] == plain[n + a]:
            a += 1
        steps, proposed, accepted = steps + 1, proposed + len(draft), accepted + a
        from_schema += len(own)
        n += a + 1
    return {"reply": plain[:n], "spec_steps": steps, "spec_proposed": proposed, "spec_accepted": accepted,
            "schema_proposed": from_schema}
