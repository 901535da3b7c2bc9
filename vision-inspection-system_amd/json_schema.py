"""Schema-constrained decoding (``response_format={"type": "json_schema", ...}``): a JSON Schema compiled to a byte-level
DFA, and the CPU reference of the mask the decode loop enforces on the GPU.

This module is the reference implementation; ``csrc/schema_mask.hip`` (vis_schema_mask) walks the same tables and must stay
bit-exact with ``allowed`` / ``advance`` below (tests/test_json_schema.py, tests/test_json_schema_gpu.py).

A non-recursive schema whose objects emit their keys in ``properties`` order describes a regular language, so the whole
grammar is one table: ``state = trans[state][byte_class[byte]]``, 0xFFFF = dead.  Supported subset (everything pydantic's
``model_json_schema()`` emits for this project's report models):
  * ``type: object`` with ``properties`` / ``required`` / ``additionalProperties`` absent or false: keys in ``properties``
    order, a key outside ``required`` may be left out, commas are right for every subset of present keys;
  * ``type: array`` with ``items`` (any length, ``[]`` included);
  * ``type: string`` (json_grammar's string: escapes, \\uXXXX, strict UTF-8 per Unicode Table 3-7, no raw control bytes),
    ``number`` (json_grammar's number), ``integer`` (no fraction, no exponent), ``boolean``, ``null``; a list of types;
  * ``enum`` / ``const`` of strings, numbers, booleans and null, matched as their exact JSON encoding;
  * ``anyOf`` whose alternatives start with distinct bytes (``Optional[X]``);
  * ``$ref`` into ``#/$defs/...`` / ``#/definitions/...``, expanded inline (a recursive one is refused);
  * the annotations in ANNOTATIONS are ignored; ANY other keyword is a ValueError that names it.
The top level must be ``type: object``.  Nothing may precede ``{`` and no byte may follow the top-level ``}`` (only an EOS
token).  Between structural tokens at most SCHEMA_MAX_WS bytes of space / tab / LF / CR are accepted.

A token is allowed when the DFA survives its WHOLE byte string from the current state; tokens without bytes never are; EOS
ids only in an accepting state.  When no token is allowed the EOS ids are allowed and the error bit is set, as in JSON mode.
"""
from __future__ import annotations

import json
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .json_grammar import FLAG_EOS, FLAG_PLAIN, TokenTable, mask_words

# Whitespace between structural tokens: json.dumps' ", " / ": " need one byte, pydantic's compact form none.  Every
# whitespace position costs SCHEMA_MAX_WS states (a counted run is a chain), and whitespace positions are about a third of
# a compiled report schema, so the cap is kept at one more than json.dumps needs: schemas.REPORT_SCHEMA compiles to 414
# states at 0, 481 at 1, 548 at 2, 682 at 4 and 1486 at 16 (JSON mode's cap) - 67 states per byte of the cap.  At 2 its
# table (548 x 64 classes x 2 bytes = 70144) still fits the 72 KiB the kernel stages in LDS.
SCHEMA_MAX_WS = 2
SCHEMA_MAX_STATES = 4096        # SM_MAX_STATES of csrc/schema_mask.hip: sizes the device tables of SchemaBuffers
SCHEMA_MAX_CLASSES = 256        # one class per byte value at most
DEAD = 0xFFFF                   # SM_DEAD

STATE_ACCEPT = 1                # state_flags bit 0: EOS ids are allowed here (after the top-level '}') and nowhere else
STATE_PLAIN = 2                 # bit 1: every printable ASCII byte except '"' and '\\' loops here (a string body)

# words of one state slot (int32), SW_* in csrc/schema_mask.hip: DFA state, error bit, next token position to fold in,
# anchored (the slot has been written: all zero = a fresh sequence in the DFA's start state)
STATE, ERR, POS, ANCHOR = range(4)
SLOT_INTS = 12                  # json_grammar's slot pitch, so both masks share one [slots, 32] layout
STATE_INTS = 32
COUNT_WORD, TICKET_WORD = 24, 25
HEADER_INTS = 4                 # device header: n_states, n_classes, start, 0

ANNOTATIONS = ("title", "description", "default", "examples", "format", "$schema")
_WS = (0x20, 0x09, 0x0A, 0x0D)
_TYPES = ("object", "array", "string", "number", "integer", "boolean", "null")


class SchemaDFA(NamedTuple):
    trans: np.ndarray           # uint16 [n_states, n_classes], DEAD = no transition
    byte_class: np.ndarray      # uint8 [256]
    state_flags: np.ndarray     # uint8 [n_states]: STATE_ACCEPT | STATE_PLAIN
    start: int

    @property
    def n_states(self) -> int:
        return self.trans.shape[0]

    @property
    def n_classes(self) -> int:
        return self.trans.shape[1]

    @property
    def table_bytes(self) -> int:
        return self.trans.nbytes + self.byte_class.nbytes + self.state_flags.nbytes


# ----------------------------------------------------------------------------- compiler
class _Builder:
    """Deterministic automaton under construction: one {byte: state} dict per state.  A value is compiled against its
    ``follow`` map - the transitions available right after it - because a number ends only at the byte that follows it."""

    def __init__(self, root: dict, max_ws: int):
        self.t: List[Dict[int, int]] = []
        self.root = root
        self.max_ws = max_ws

    def new(self, trans: Optional[Dict[int, int]] = None) -> int:
        self.t.append(dict(trans or {}))
        return len(self.t) - 1

    @staticmethod
    def merge(into: Dict[int, int], more: Dict[int, int], what: str) -> None:
        for b, s in more.items():
            if b in into and into[b] != s:
                raise ValueError(f"json_schema: ambiguous {what}: two alternatives may start with byte {bytes([b])!r}")
            into[b] = s

    def ws(self, m: Dict[int, int]) -> Dict[int, int]:
        """``m`` after at most max_ws whitespace bytes."""
        cur = dict(m)
        for _ in range(self.max_ws):
            s = self.new(cur)
            cur = dict(m)
            for b in _WS:
                cur[b] = s
        return cur

    def chain(self, data: bytes, last: int) -> Dict[int, int]:
        """The bytes of ``data`` in a row, the last one entering state ``last``."""
        nxt = last
        for b in reversed(data[1:]):
            nxt = self.new({b: nxt})
        return {data[0]: nxt}

    def trie(self, words: Dict[bytes, Dict[int, int]], what: str) -> Dict[int, int]:
        """First-byte map of a set of byte strings; after the whole of ``word`` the transitions ``words[word]`` apply."""
        root: Dict[int, int] = {}
        node_of = {b"": None}
        for word in sorted(words):
            for i in range(1, len(word) + 1):
                pre = word[:i]
                if pre not in node_of:
                    node_of[pre] = self.new()
                    parent = root if i == 1 else self.t[node_of[word[:i - 1]]]
                    parent[word[i - 1]] = node_of[pre]
        for word, follow in words.items():
            self.merge(self.t[node_of[word]], follow, what)
        return root

    # -- values
    def string(self, follow: Dict[int, int]) -> Dict[int, int]:
        body = self.new()
        t = self.t[body]
        for b in range(0x20, 0x80):
            t[b] = body
        t[0x22] = self.new(follow)
        hexd = b"0123456789abcdefABCDEF"
        nxt = body
        for _ in range(4):
            nxt = self.new({h: nxt for h in hexd})
        esc = self.new({b: body for b in b'"\\/bfnrt'})
        self.t[esc][0x75] = nxt
        t[0x5C] = esc

        def cont(lo: int, hi: int, to: int) -> int:
            return self.new({b: to for b in range(lo, hi + 1)})
        c1 = cont(0x80, 0xBF, body)
        c2 = cont(0x80, 0xBF, c1)
        for lo, hi, to in ((0xC2, 0xDF, c1), (0xE0, 0xE0, cont(0xA0, 0xBF, c1)), (0xE1, 0xEC, c2), (0xED, 0xED, cont(0x80, 0x9F, c1)),
                           (0xEE, 0xEF, c2), (0xF0, 0xF0, cont(0x90, 0xBF, c2)), (0xF1, 0xF3, cont(0x80, 0xBF, c2)),
                           (0xF4, 0xF4, cont(0x80, 0x8F, c2))):
            for b in range(lo, hi + 1):
                t[b] = to
        return {0x22: body}

    def number(self, follow: Dict[int, int], integer: bool) -> Dict[int, int]:
        digits = b"0123456789"
        zero, intg = self.new(follow), self.new(follow)
        for d in digits:
            self.t[intg][d] = intg
        if not integer:
            frac, expd = self.new(follow), self.new(follow)
            for d in digits:
                self.t[frac][d] = frac
                self.t[expd][d] = expd
            dot = self.new({d: frac for d in digits})
            sign = self.new({d: expd for d in digits})
            exp = self.new({d: expd for d in digits})
            self.t[exp][0x2B] = self.t[exp][0x2D] = sign
            for s in (zero, intg):
                self.t[s][0x2E] = dot
            for s in (zero, intg, frac):
                self.t[s][0x65] = self.t[s][0x45] = exp
        first = {0x30: zero}
        for d in digits[1:]:
            first[d] = intg
        first[0x2D] = self.new(dict(first))
        return first

    def literals(self, values: Sequence, follow: Dict[int, int]) -> Dict[int, int]:
        words: Dict[bytes, Dict[int, int]] = {}
        for v in values:
            if not (v is None or isinstance(v, (str, bool, int, float))):
                raise ValueError(f"json_schema: enum / const value {v!r} is unsupported (strings, numbers, booleans, null)")
            if isinstance(v, float) and (v != v or v in (float("inf"), float("-inf"))):
                raise ValueError(f"json_schema: enum / const value {v!r} has no JSON encoding")
            for ascii_only in (False, True):
                words[json.dumps(v, ensure_ascii=ascii_only).encode("utf-8")] = follow
        return self.trie(words, "enum")

    def array(self, node: dict, follow: Dict[int, int], path: str, refs: tuple) -> Dict[int, int]:
        if "items" not in node:
            raise ValueError(f"json_schema: {path}: an array needs 'items'")
        end = self.new(follow)
        comma = self.new()
        first = self.value(node["items"], self.ws({0x2C: comma, 0x5D: end}), path + "/items", refs)
        self.t[comma].update(self.ws(first))
        opened = dict(first)
        self.merge(opened, {0x5D: end}, "array item")
        return {0x5B: self.new(self.ws(opened))}

    def object(self, node: dict, follow: Dict[int, int], path: str, refs: tuple) -> Dict[int, int]:
        props = node.get("properties", {})
        if not isinstance(props, dict):
            raise ValueError(f"json_schema: {path}: 'properties' must be an object")
        if node.get("additionalProperties", False) is not False:
            raise ValueError(f"json_schema: {path}: additionalProperties other than false is unsupported")
        names = list(props)
        required = node.get("required", [])
        if not isinstance(required, list) or any(r not in props for r in required):
            raise ValueError(f"json_schema: {path}: 'required' must list declared properties")
        optional = [n not in required for n in names]
        end = self.new(follow)
        n = len(names)

        def candidates(i0: int) -> Tuple[List[int], bool]:
            """Keys that may come next when keys i0.. are still open, and whether the object may close instead."""
            out = []
            for i in range(i0, n):
                out.append(i)
                if not optional[i]:
                    return out, False
            return out, True

        key_done: Dict[int, int] = {}
        for i in reversed(range(n)):
            nxt, may_close = candidates(i + 1)
            after: Dict[int, int] = {}
            if nxt:
                after[0x2C] = self.new(self.ws(self.keys(names, nxt, key_done)))
            if may_close:
                after[0x7D] = end
            first = self.value(props[names[i]], self.ws(after), f"{path}/properties/{names[i]}", refs)
            key_done[i] = self.new(self.ws({0x3A: self.new(self.ws(first))}))
        nxt, may_close = candidates(0)
        opened = self.keys(names, nxt, key_done) if nxt else {}
        if may_close:
            opened[0x7D] = end
        return {0x7B: self.new(self.ws(opened))}

    def keys(self, names: List[str], which: List[int], key_done: Dict[int, int]) -> Dict[int, int]:
        words: Dict[bytes, Dict[int, int]] = {}
        for i in which:
            for ascii_only in (False, True):
                words[json.dumps(names[i], ensure_ascii=ascii_only).encode("utf-8")] = self.t[key_done[i]]
        return self.trie(words, "property names")

    def value(self, node, follow: Dict[int, int], path: str, refs: tuple = ()) -> Dict[int, int]:
        if not isinstance(node, dict):
            raise ValueError(f"json_schema: {path}: a schema must be an object (true / false schemas are unsupported)")
        known = {"type", "properties", "required", "additionalProperties", "items", "enum", "const", "anyOf", "$ref",
                 "$defs", "definitions"}
        for k in node:
            if k not in known and k not in ANNOTATIONS:
                raise ValueError(f"json_schema: {path}: unsupported keyword {k!r}")
        if "$ref" in node:
            ref = node["$ref"]
            parts = ref.split("/") if isinstance(ref, str) else []
            if len(parts) != 3 or parts[0] != "#" or parts[1] not in ("$defs", "definitions"):
                raise ValueError(f"json_schema: {path}: unsupported $ref {ref!r} (only #/$defs/NAME and #/definitions/NAME)")
            if ref in refs:
                raise ValueError(f"json_schema: {path}: recursive $ref {ref!r} (a recursive schema is not a regular language)")
            target = self.root.get(parts[1], {}).get(parts[2].replace("~1", "/").replace("~0", "~"))
            if target is None:
                raise ValueError(f"json_schema: {path}: unresolved $ref {ref!r}")
            if any(k in node for k in ("type", "enum", "const", "anyOf", "properties", "items")):
                raise ValueError(f"json_schema: {path}: keywords next to $ref are unsupported")
            return self.value(target, follow, ref, refs + (ref,))
        if "anyOf" in node:
            alts = node["anyOf"]
            if not isinstance(alts, list) or not alts or any(k in node for k in ("type", "enum", "const")):
                raise ValueError(f"json_schema: {path}: anyOf must be a non-empty list with no type / enum next to it")
            out: Dict[int, int] = {}
            for i, alt in enumerate(alts):
                self.merge(out, self.value(alt, follow, f"{path}/anyOf/{i}", refs), f"anyOf at {path}")
            return out
        types = node.get("type")
        if types is not None:
            types = types if isinstance(types, list) else [types]
            for ty in types:
                if ty not in _TYPES:
                    raise ValueError(f"json_schema: {path}: unsupported type {ty!r}")
        if "enum" in node or "const" in node:
            values = list(node["enum"]) if "enum" in node else [node["const"]]
            if "enum" in node and "const" in node:
                values = [v for v in values if v == node["const"] and type(v) is type(node["const"])]
            if types is not None:
                values = [v for v in values if any(_is_type(v, ty) for ty in types)]
            if not values:
                raise ValueError(f"json_schema: {path}: enum / const allows no value")
            return self.literals(values, follow)
        if types is None:
            raise ValueError(f"json_schema: {path}: a schema without 'type' (any value) is unsupported")
        out = {}
        for ty in dict.fromkeys(types):
            if ty == "integer" and "number" in types:
                continue
            self.merge(out, self.typed(ty, node, follow, path, refs), f"type list at {path}")
        return out

    def typed(self, ty: str, node: dict, follow: Dict[int, int], path: str, refs: tuple) -> Dict[int, int]:
        if ty == "object":
            return self.object(node, follow, path, refs)
        if ty == "array":
            return self.array(node, follow, path, refs)
        if ty == "string":
            return self.string(follow)
        if ty in ("number", "integer"):
            return self.number(follow, ty == "integer")
        if ty == "boolean":
            return self.literals([True, False], follow)
        return self.literals([None], follow)


def _is_type(v, ty: str) -> bool:
    if ty == "null":
        return v is None
    if ty == "boolean":
        return isinstance(v, bool)
    if ty == "string":
        return isinstance(v, str)
    if ty == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if ty == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if ty == "object":
        return isinstance(v, dict)
    return isinstance(v, list)


def _minimise(t: np.ndarray, accept: np.ndarray, start: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Moore partition refinement of a complete byte-level table (int32 [n, 256], -1 = dead); unreachable states and states
    that cannot reach an accepting one are dropped first.  States keep the order of their first member."""
    n = len(t)
    src, byte = np.nonzero(t >= 0)
    edges = np.unique(np.stack([src, t[src, byte]], axis=1), axis=0)
    succ: Dict[int, List[int]] = {}
    pred: Dict[int, List[int]] = {}
    for a, b in edges.tolist():
        succ.setdefault(a, []).append(b)
        pred.setdefault(b, []).append(a)

    def closure(seeds: List[int], step: Dict[int, List[int]]) -> np.ndarray:
        seen = np.zeros(n, dtype=bool)
        seen[seeds] = True
        todo = list(seeds)
        while todo:
            for d in step.get(todo.pop(), ()):
                if not seen[d]:
                    seen[d] = True
                    todo.append(d)
        return seen

    reach = closure([start], succ)
    live = closure(np.flatnonzero(accept).tolist(), pred)
    keep = reach & live
    if not keep[start]:
        raise ValueError("json_schema: the schema accepts no document")
    t = np.where((t >= 0) & keep[np.where(t >= 0, t, 0)], t, -1)
    idx = np.flatnonzero(keep)
    renum = np.full(n + 1, -1, dtype=np.int64)
    renum[idx] = np.arange(len(idx))
    t = renum[t[idx]]                       # -1 indexes the spare last entry: stays -1
    accept = accept[idx]
    start = int(renum[start])
    block = accept.astype(np.int64)
    nblocks = 0
    while True:
        sig = np.concatenate([block[:, None], np.where(t >= 0, block[np.where(t >= 0, t, 0)], -1)], axis=1)
        _, first, inv = np.unique(sig, axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        order = np.argsort(first, kind="stable")            # blocks in order of their first member
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        block = rank[inv]
        if len(first) == nblocks:
            break
        nblocks = len(first)
    rep = np.sort(first)
    t2 = np.where(t[rep] >= 0, block[np.where(t[rep] >= 0, t[rep], 0)], -1)
    return t2, accept[rep], int(block[start])


def compile_schema(schema: dict, max_ws: int = SCHEMA_MAX_WS) -> SchemaDFA:
    """JSON Schema (the subset of the module docstring) -> SchemaDFA.  ValueError, naming the cause, for anything else.
    ``max_ws`` other than SCHEMA_MAX_WS is for measuring the cap's cost in states."""
    if not isinstance(schema, dict):
        raise ValueError("json_schema: the schema must be a JSON object")
    try:
        json.dumps(schema)
    except (TypeError, ValueError) as e:
        raise ValueError(f"json_schema: the schema is not JSON: {e}") from None
    if schema.get("type") != "object" and "$ref" not in schema:
        raise ValueError("json_schema: the top level must be 'type': 'object'")
    b = _Builder(schema, max_ws)
    first = b.value(schema, {}, "#")         # the top level's follow map is empty: no byte after its '}'
    if set(first) != {0x7B}:
        raise ValueError("json_schema: the top level must be 'type': 'object'")
    start = b.new(first)
    n = len(b.t)
    full = np.full((n, 256), -1, dtype=np.int32)
    for s, tr in enumerate(b.t):
        for byte, d in tr.items():
            full[s, byte] = d
    # every other value has a follow map, so the only state without transitions is the one the top-level '}' enters
    accept = np.array([not tr for tr in b.t], dtype=bool)
    t, accept, start = _minimise(full, accept, start)
    n = len(t)
    if n > SCHEMA_MAX_STATES:
        raise ValueError(f"json_schema: the schema compiles to {n} states; the cap is {SCHEMA_MAX_STATES}")
    cols, cls = np.unique(t, axis=1, return_inverse=True)
    cls = cls.reshape(-1)
    # classes in order of their first byte, so the table does not depend on numpy's column sort
    firsts = np.array([int(np.flatnonzero(cls == c)[0]) for c in range(cols.shape[1])])
    rank = np.empty(len(firsts), dtype=np.int64)
    rank[np.argsort(firsts)] = np.arange(len(firsts))
    byte_class = rank[cls].astype(np.uint8)
    trans = np.empty((n, len(firsts)), dtype=np.uint16)
    trans[:, rank] = np.where(cols >= 0, cols, DEAD).astype(np.uint16)
    plain = [c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)]
    flags = accept.astype(np.uint8) * STATE_ACCEPT
    flags |= ((t[:, plain] == np.arange(n)[:, None]).all(axis=1)).astype(np.uint8) * STATE_PLAIN
    return SchemaDFA(np.ascontiguousarray(trans), byte_class, flags, start)


def canonical(schema: dict) -> str:
    """The text compiled DFAs are cached by.  Key order is kept: the order of ``properties`` is the order of the reply's keys."""
    return json.dumps(schema, separators=(",", ":"), ensure_ascii=True)


# ----------------------------------------------------------------------------- reference walk
def step(dfa: SchemaDFA, state: int, byte: int) -> int:
    """The state after ``byte``, DEAD when the DFA rejects it (or ``state`` is DEAD already)."""
    if state == DEAD:
        return DEAD
    return int(dfa.trans[state, dfa.byte_class[byte]])


def walk(dfa: SchemaDFA, state: int, data: bytes) -> int:
    for b in data:
        state = step(dfa, state, b)
        if state == DEAD:
            break
    return state


def accepts(dfa: SchemaDFA, data: bytes) -> bool:
    """``data`` is a whole document of the schema."""
    s = walk(dfa, dfa.start, data)
    return s != DEAD and bool(dfa.state_flags[s] & STATE_ACCEPT)


def initial_state(dfa: SchemaDFA) -> List[int]:
    """[DFA state, error bit] of a fresh sequence."""
    return [dfa.start, 0]


def advance(dfa: SchemaDFA, st: List[int], token: int, table: TokenTable) -> None:
    """Fold one picked token into ``st`` = [state, error bit] (in place): its bytes, or for an EOS id nothing in an accepting
    state.  A token the DFA rejects (or an EOS id elsewhere, or a token without bytes) sets the error bit only."""
    if st[1]:
        return
    if not 0 <= token < table.vocab:
        st[1] = 1
        return
    if table.flags[token] & FLAG_EOS:
        if not dfa.state_flags[st[0]] & STATE_ACCEPT:
            st[1] = 1
        return
    s = walk(dfa, st[0], table.tokens[token]) if table.tokens[token] else DEAD
    if s == DEAD:
        st[1] = 1
    else:
        st[0] = s


def allowed(dfa: SchemaDFA, st: Sequence[int], table: TokenTable) -> Tuple[np.ndarray, bool]:
    """(bool [V]: the tokens allowed in ``st`` = [state, error bit], error): error is True when no token was allowed and the
    EOS ids were allowed in their place (the kernel then sets the error bit).  All tokens walk at once, a byte per round."""
    V = table.vocab
    ok = np.zeros(V, dtype=bool)
    if not st[1]:
        flags = int(dfa.state_flags[st[0]])
        off = table.off.astype(np.int64)
        lens = off[1:] - off[:-1]
        cur = np.full(V, st[0], dtype=np.int64)
        ids = np.flatnonzero(lens > 0)
        if flags & STATE_PLAIN:             # the kernel's shortcut: PLAIN tokens are taken without a walk
            ok[(table.flags & FLAG_PLAIN) != 0] = True
            ids = ids[(table.flags[ids] & FLAG_PLAIN) == 0]
        trans = dfa.trans.astype(np.int64)
        j = 0
        while len(ids):
            nxt = trans[cur[ids], dfa.byte_class[table.data[off[ids] + j]]]
            cur[ids] = nxt
            ids = ids[nxt != DEAD]
            j += 1
            fin = lens[ids] == j
            ok[ids[fin]] = True
            ids = ids[~fin]
        if flags & STATE_ACCEPT:
            ok[table.eos_ids] = True
    if ok.any():
        return ok, False
    ok[table.eos_ids] = True
    return ok, True


def allowed_mask(dfa: SchemaDFA, state: int, table: TokenTable) -> np.ndarray:
    """The kernel's row for DFA state ``state``: uint64 words [ceil(V / 64)], bit i of word w = token 64 w + i."""
    return mask_words(allowed(dfa, [state, 0], table)[0]).view(np.uint64)


# ----------------------------------------------------------------------------- validation of parsed documents
def validate(schema: dict, obj, _root: Optional[dict] = None) -> bool:
    """``obj`` (parsed JSON) satisfies ``schema``, for the supported subset.  Key order is not part of JSON Schema and is not
    checked here; the DFA is stricter."""
    root = schema if _root is None else _root
    if "$ref" in schema:
        _, where, name = schema["$ref"].split("/")
        return validate(root[where][name], obj, root)
    if "anyOf" in schema:
        return any(validate(alt, obj, root) for alt in schema["anyOf"])
    types = schema.get("type")
    types = None if types is None else (types if isinstance(types, list) else [types])
    if types is not None and not any(_is_type(obj, ty) for ty in types):
        return False
    same = lambda a, b: a == b and isinstance(a, bool) == isinstance(b, bool)      # noqa: E731 - 1 is not true
    if "const" in schema and not same(obj, schema["const"]):
        return False
    if "enum" in schema and not any(same(obj, v) for v in schema["enum"]):
        return False
    if isinstance(obj, dict) and (types is None or "object" in types) and "properties" in schema or \
            isinstance(obj, dict) and "required" in schema:
        props = schema.get("properties", {})
        if any(k not in props for k in obj) or any(r not in obj for r in schema.get("required", [])):
            return False
        return all(validate(props[k], v, root) for k, v in obj.items())
    if isinstance(obj, list) and "items" in schema:
        return all(validate(schema["items"], v, root) for v in obj)
    return True
