"""JSON mode (``response_format={"type": "json_object"}``): the byte-level grammar the decode loop enforces on the GPU.

This module is the reference implementation; ``csrc/json_mask.hip`` (vis_json_mask) is a line-by-line transliteration of
``step`` below and must stay byte-exact with it (tests/test_json_grammar.py, tests/test_json_mode_gpu.py).

The language is RFC 8259 JSON whose top-level value is an object, as in OpenAI's JSON mode:
  * before the object only whitespace and ``{``; after the top-level ``}`` no byte at all (only an EOS token);
  * strings: no raw control bytes (< 0x20); escapes ``\\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX``; non-ASCII bytes must form
    well-formed UTF-8 (Unicode Table 3-7: no overlong forms, no surrogates, nothing above U+10FFFF), so the output
    always decodes strictly; outside strings only ASCII;
  * numbers ``-?(0|[1-9][0-9]*)(\\.[0-9]+)?([eE][+-]?[0-9]+)?``, ``true`` / ``false`` / ``null``;
  * at most MAX_DEPTH open containers (at the cap ``{`` and ``[`` are refused) and at most MAX_WS consecutive whitespace
    bytes (a sampler cannot loop on whitespace for ever).

A token is allowed when the grammar accepts its WHOLE byte string from the current state.  Tokens with no bytes (specials,
image pads, ids past the tokenizer's vocabulary) are never allowed; EOS ids are allowed in the DONE state and nowhere else.
When no token at all is allowed (a vocabulary that lacks a byte the grammar needs) the EOS ids are allowed and the error
bit is set: the engine then reports the request as failed instead of returning text that is not JSON.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_DEPTH = 32          # JG_MAX_DEPTH of csrc/json_mask.hip
MAX_WS = 16             # JG_MAX_WS

# lexer states (JG_* in csrc/json_mask.hip)
(START, OBJ_FIRST, OBJ_KEY, COLON, VALUE, ARR_FIRST, AFTER, STR, ESC, HEX, LIT_T, LIT_F, LIT_N,
 N_MINUS, N_ZERO, N_INT, N_DOT, N_FRAC, N_EXP, N_EXP_SIGN, N_EXP_DIG, DONE) = range(22)
STRUCTURAL = (START, OBJ_FIRST, OBJ_KEY, COLON, VALUE, ARR_FIRST, AFTER)
_LITS = {LIT_T: b"true", LIT_F: b"false", LIT_N: b"null"}

# words of one grammar state (int32): lexer state, open containers, container kinds (bit d = 1: level d is an array),
# whitespace run, pending UTF-8 continuation bytes | lower bound << 8 | upper bound << 16, position in a literal or \u
# escape, "the open string is a key", error bit, next token position to fold in, anchored (pos is valid)
LEX, DEPTH, STACK, WS, UTF, AUX, KEY, ERR, POS, ANCHOR = range(10)
LEX_WORDS = 8           # the grammar proper; POS / ANCHOR only track the device-side token buffer
SLOT_INTS = 12          # one state slot
STATE_INTS = 32         # per sequence on the device: two slots (parity of the step) + the mask launch's counters
COUNT_WORD, TICKET_WORD = 24, 25

FLAG_EOS = 1            # the token is one of the engine's EOS ids
FLAG_PLAIN = 2          # non-empty, every byte printable ASCII 0x20..0x7e and neither '"' nor '\\': accepted whole inside a string

_WS = (0x20, 0x09, 0x0A, 0x0D)


def initial_state() -> List[int]:
    return [0] * SLOT_INTS


def _push(st: List[int], is_array: bool) -> bool:
    d = st[DEPTH]
    if d >= MAX_DEPTH:
        return False
    if is_array:
        st[STACK] |= 1 << d
    else:
        st[STACK] &= ~(1 << d) & 0xFFFFFFFF
    st[DEPTH] = d + 1
    st[LEX] = ARR_FIRST if is_array else OBJ_FIRST
    return True


def _top_is_array(st: List[int]) -> bool:
    return bool((st[STACK] >> (st[DEPTH] - 1)) & 1)


def _pop(st: List[int]) -> None:
    st[DEPTH] -= 1
    st[LEX] = DONE if st[DEPTH] == 0 else AFTER


def _value_start(st: List[int], b: int) -> bool:
    if b == 0x7B:
        return _push(st, False)
    if b == 0x5B:
        return _push(st, True)
    if b == 0x22:
        st[LEX], st[KEY], st[UTF] = STR, 0, 0
        return True
    if b == 0x2D:
        st[LEX] = N_MINUS
    elif b == 0x30:
        st[LEX] = N_ZERO
    elif 0x31 <= b <= 0x39:
        st[LEX] = N_INT
    elif b == 0x74:
        st[LEX], st[AUX] = LIT_T, 1
    elif b == 0x66:
        st[LEX], st[AUX] = LIT_F, 1
    elif b == 0x6E:
        st[LEX], st[AUX] = LIT_N, 1
    else:
        return False
    return True


def step(st: List[int], b: int) -> bool:
    """Advance the grammar state ``st`` (a list of at least LEX_WORDS ints, modified in place) by the byte ``b``.
    Returns False when the grammar rejects ``b``; ``st`` is then unspecified (callers walk a copy)."""
    if st[ERR]:
        return False
    lex = st[LEX]
    if lex == STR:
        pend = st[UTF] & 0xFF
        if pend:
            if not ((st[UTF] >> 8) & 0xFF) <= b <= ((st[UTF] >> 16) & 0xFF):
                return False
            st[UTF] = (pend - 1) | (0x80 << 8) | (0xBF << 16) if pend > 1 else 0
            return True
        if b == 0x22:
            st[LEX] = COLON if st[KEY] else AFTER
            st[KEY] = 0
            return True
        if b == 0x5C:
            st[LEX] = ESC
            return True
        if b < 0x20:
            return False
        if b < 0x80:
            return True
        # UTF-8 lead byte (Unicode Table 3-7): continuation count and the range of the FIRST continuation byte
        if 0xC2 <= b <= 0xDF:
            st[UTF] = 1 | (0x80 << 8) | (0xBF << 16)
        elif b == 0xE0:
            st[UTF] = 2 | (0xA0 << 8) | (0xBF << 16)
        elif 0xE1 <= b <= 0xEC or b == 0xEE or b == 0xEF:
            st[UTF] = 2 | (0x80 << 8) | (0xBF << 16)
        elif b == 0xED:
            st[UTF] = 2 | (0x80 << 8) | (0x9F << 16)
        elif b == 0xF0:
            st[UTF] = 3 | (0x90 << 8) | (0xBF << 16)
        elif 0xF1 <= b <= 0xF3:
            st[UTF] = 3 | (0x80 << 8) | (0xBF << 16)
        elif b == 0xF4:
            st[UTF] = 3 | (0x80 << 8) | (0x8F << 16)
        else:
            return False
        return True
    if lex == ESC:
        if b in (0x22, 0x5C, 0x2F, 0x62, 0x66, 0x6E, 0x72, 0x74):
            st[LEX] = STR
            return True
        if b == 0x75:
            st[LEX], st[AUX] = HEX, 0
            return True
        return False
    if lex == HEX:
        if not (0x30 <= b <= 0x39 or 0x41 <= b <= 0x46 or 0x61 <= b <= 0x66):
            return False
        st[AUX] += 1
        if st[AUX] == 4:
            st[LEX], st[AUX] = STR, 0
        return True
    if lex in (LIT_T, LIT_F, LIT_N):
        lit = _LITS[lex]
        if b != lit[st[AUX]]:
            return False
        st[AUX] += 1
        if st[AUX] == len(lit):
            st[LEX], st[AUX] = AFTER, 0
        return True
    digit = 0x30 <= b <= 0x39
    if lex == N_MINUS:
        if b == 0x30:
            st[LEX] = N_ZERO
        elif digit:
            st[LEX] = N_INT
        else:
            return False
        return True
    if lex == N_DOT:
        if not digit:
            return False
        st[LEX] = N_FRAC
        return True
    if lex == N_EXP:
        if b == 0x2B or b == 0x2D:
            st[LEX] = N_EXP_SIGN
        elif digit:
            st[LEX] = N_EXP_DIG
        else:
            return False
        return True
    if lex == N_EXP_SIGN:
        if not digit:
            return False
        st[LEX] = N_EXP_DIG
        return True
    if lex in (N_ZERO, N_INT, N_FRAC, N_EXP_DIG):
        if digit and lex != N_ZERO:
            return True
        if b == 0x2E and lex in (N_ZERO, N_INT):
            st[LEX] = N_DOT
            return True
        if (b == 0x65 or b == 0x45) and lex != N_EXP_DIG:
            st[LEX] = N_EXP
            return True
        if digit:           # a digit after a leading zero
            return False
        st[LEX] = lex = AFTER       # the number ends here: the byte is read as what follows a value
    if lex == DONE:
        return False
    # structural states
    if b in _WS:
        st[WS] += 1
        return st[WS] <= MAX_WS
    st[WS] = 0
    if lex == START:
        return b == 0x7B and _push(st, False)
    if lex == OBJ_FIRST or lex == OBJ_KEY:
        if b == 0x22:
            st[LEX], st[KEY], st[UTF] = STR, 1, 0
            return True
        if b == 0x7D and lex == OBJ_FIRST:
            _pop(st)
            return True
        return False
    if lex == COLON:
        if b != 0x3A:
            return False
        st[LEX] = VALUE
        return True
    if lex == VALUE or lex == ARR_FIRST:
        if b == 0x5D and lex == ARR_FIRST:
            _pop(st)
            return True
        return _value_start(st, b)
    # AFTER
    arr = _top_is_array(st)
    if b == 0x2C:
        st[LEX] = VALUE if arr else OBJ_KEY
        return True
    if (b == 0x5D and arr) or (b == 0x7D and not arr):
        _pop(st)
        return True
    return False


def accepts(st: Sequence[int], data: bytes) -> Optional[List[int]]:
    """The state after ``data`` from ``st`` (not modified), or None if the grammar rejects some byte of it."""
    s = list(st)
    for b in data:
        if not step(s, b):
            return None
    return s


def feed(data: bytes) -> Tuple[str, int]:
    """Walk ``data`` from the initial state: ("done", n) if it ends exactly in DONE, ("progress", n) if every byte was
    accepted and the object is still open, ("reject", i) at the first rejected byte i."""
    s = initial_state()
    for i, b in enumerate(data):
        if not step(s, b):
            return "reject", i
    return ("done" if s[LEX] == DONE else "progress"), len(data)


# ----------------------------------------------------------------------------- token table
class TokenTable(NamedTuple):
    """CSR byte table of a vocabulary: token t's bytes are data[off[t]:off[t + 1]]; EOS tokens hold no bytes."""
    off: np.ndarray         # int32 [V + 1]
    data: np.ndarray        # uint8 [off[V] + 4] (4 zero bytes of padding: the kernel reads aligned dwords)
    flags: np.ndarray       # uint8 [V]
    eos_ids: np.ndarray     # int32 [n_eos]
    tokens: tuple           # bytes per token (host reference)

    @property
    def vocab(self) -> int:
        return len(self.flags)


def build_token_table(tokenizer, V: int, eos_ids: Sequence[int]) -> TokenTable:
    """The table of ids 0..V-1 from ``tokenizer.token_bytes`` (empty for ids it does not know)."""
    eos = sorted({int(e) for e in eos_ids if 0 <= int(e) < V})
    if not eos:
        raise ValueError("JSON mode needs at least one EOS id inside the vocabulary")
    eos_set = set(eos)
    toks = []
    for t in range(V):
        if t in eos_set:
            toks.append(b"")
            continue
        try:
            b = tokenizer.token_bytes(t)
        except Exception:           # noqa: BLE001 - ids past the tokenizer's vocabulary
            b = b""
        toks.append(bytes(b or b""))
    lens = np.fromiter((len(b) for b in toks), dtype=np.int64, count=V)
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 2 ** 31 - 8:
        raise ValueError("token table too large")
    data = np.zeros(int(off[-1]) + 4, dtype=np.uint8)
    data[:off[-1]] = np.frombuffer(b"".join(toks), dtype=np.uint8)
    flags = np.zeros(V, dtype=np.uint8)
    flags[eos] = FLAG_EOS
    plain = bytes(c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C))
    strip = bytes.maketrans(b"", b"")
    for t, b in enumerate(toks):
        if b and not b.translate(strip, plain):
            flags[t] |= FLAG_PLAIN
    return TokenTable(off.astype(np.int32), data, flags, np.asarray(eos, dtype=np.int32), tuple(toks))


def advance(st: List[int], token: int, table: TokenTable) -> None:
    """Fold one picked token into ``st`` (in place): its bytes, or for an EOS id nothing in DONE.  A token the grammar
    does not accept (or an EOS id before DONE) sets the error bit and leaves the other words as they were."""
    if st[ERR]:
        return
    if not 0 <= token < table.vocab:
        st[ERR] = 1
        return
    if table.flags[token] & FLAG_EOS:
        if st[LEX] != DONE:
            st[ERR] = 1
        return
    s = accepts(st, table.tokens[token]) if table.tokens[token] else None
    if s is None:
        st[ERR] = 1
    else:
        st[:LEX_WORDS] = s[:LEX_WORDS]


def allowed(st: Sequence[int], table: TokenTable) -> Tuple[np.ndarray, bool]:
    """(bool [V]: the tokens allowed in ``st``, error): error is True when no token was allowed and the EOS ids were
    allowed in their place (the kernel then sets the error bit)."""
    V = table.vocab
    ok = np.zeros(V, dtype=bool)
    if not st[ERR]:
        if st[LEX] == DONE:
            ok[table.eos_ids] = True
        else:
            # bytes a token may start with: everything else is rejected at its first byte
            first = {b for b in range(256) if accepts(st, bytes([b])) is not None}
            plain = st[LEX] == STR and (st[UTF] & 0xFF) == 0
            for t, b in enumerate(table.tokens):
                if not b or b[0] not in first:
                    continue
                if plain and table.flags[t] & FLAG_PLAIN:
                    ok[t] = True
                else:
                    ok[t] = accepts(st, b) is not None
    if ok.any():
        return ok, False
    ok[table.eos_ids] = True
    return ok, True


def mask_words(ok: np.ndarray) -> np.ndarray:
    """bool [V] -> the kernel's u64 words [ceil(V / 64)] (bit i of word w: token 64 w + i), as int64."""
    V = len(ok)
    padded = np.zeros(((V + 63) // 64) * 64, dtype=bool)
    padded[:V] = ok
    bits = np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1, 8)
    return bits.view("<u8").reshape(-1).view(np.int64)
