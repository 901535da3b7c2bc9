"""Stop sequences on the device (the ``stop=`` keyword of the engines' generate / generate_batch) and how a reply ended.

While a request carries stop strings, every pick - prompt pass or decode step, single or batched, eager or graph-replayed -
is followed by one vis_stop_scan launch: it folds the bytes of the tokens picked since its last launch through a byte-level
Aho-Corasick automaton of the stop strings and keeps one sticky record per slot (open / ended on EOS / ended on a stop
string, how many tokens to keep, the byte offset where the matched string starts).  The host's ``check_every`` poll reads
those records - [B, 8] ints - instead of the token rows, so a match that starts in the middle of one token and ends in the
middle of another needs no detokenising on the host.

Which match wins: over the byte stream of the generated tokens, the stop string with the smallest end offset
``find(s) + len(s)``; of several ending there, the one that starts first (the longest).  The text is cut at its start.  An
EOS token ends the stream before any later byte.  ``scan`` restates the kernel in Python, token by token; ``find_oracle`` is
the same rule written with ``bytes.find``."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_STOPS = 4               # OpenAI's limit
MAX_STOP_BYTES = 64
MAX_STATES = MAX_STOPS * MAX_STOP_BYTES + 1      # SS_MAX_STATES of csrc/stop_scan.hip
MAX_CLASSES = 256                                # SS_MAX_CLASSES
HEADER_INTS = 4                                  # n_states, n_classes, 0, 0
HIT = 0x8000                # device table only: the target state of this transition ends a stop string

# words of one slot's record (SS_* of csrc/stop_scan.hip); an all-zero row is a fresh sequence
STATE, POS, BYTES, REASON, N_TOKENS, CUT, WHICH, ANCHOR = range(8)
STATE_INTS = 8
OPEN, EOS, STOP = 0, 1, 2
REASONS = {OPEN: "length", EOS: "eos", STOP: "stop"}     # a row still open when the run ends was cut by a length limit


def check_stop(stop) -> Optional[Tuple[bytes, ...]]:
    """Argument check of ``stop=``: None (off), one str, or a sequence of 1..4 str / bytes, each 1..64 bytes as UTF-8.
    Returns the distinct strings as bytes in the order given, or None."""
    if stop is None:
        return None
    if isinstance(stop, str):
        stop = [stop]
    if isinstance(stop, (bytes, bytearray)) or not isinstance(stop, (list, tuple)):
        raise ValueError("stop must be None, a string or a list of 1 to 4 strings")
    if not 1 <= len(stop) <= MAX_STOPS:
        raise ValueError(f"stop must hold 1 to {MAX_STOPS} strings")
    out: List[bytes] = []
    for s in stop:
        if isinstance(s, str):
            b = s.encode("utf-8")
        elif isinstance(s, (bytes, bytearray)):
            b = bytes(s)
        else:
            raise ValueError("stop entries must be strings")
        if not 1 <= len(b) <= MAX_STOP_BYTES:
            raise ValueError(f"a stop string must be 1 to {MAX_STOP_BYTES} bytes of UTF-8")
        if b not in out:
            out.append(b)
    return tuple(out)


class StopDFA(NamedTuple):
    """Aho-Corasick automaton of a stop set with the failure links resolved: one lookup per byte, state 0 = start."""
    stops: Tuple[bytes, ...]
    trans: np.ndarray           # uint16 [n_states, n_classes]
    byte_class: np.ndarray      # uint8 [256]; the last class holds every byte that occurs in no stop string
    hit_len: np.ndarray         # uint8 [n_states]: length of the longest stop string that is a suffix here, 0 = none
    hit_id: np.ndarray          # uint8 [n_states]: that string's index in ``stops``


def compile_stop(stops) -> StopDFA:
    stops = check_stop(stops)
    if stops is None:
        raise ValueError("stop must name a string to compile")
    used = sorted({b for s in stops for b in s})
    n_classes = len(used) + (1 if len(used) < 256 else 0)
    byte_class = np.full(256, n_classes - 1, dtype=np.uint8)
    for c, b in enumerate(used):
        byte_class[b] = c
    # the trie
    goto: List[dict] = [{}]
    hit_len, hit_id = [0], [0]
    for i, s in enumerate(stops):
        st = 0
        for b in s:
            c = int(byte_class[b])
            nxt = goto[st].get(c)
            if nxt is None:
                nxt = len(goto)
                goto[st][c] = nxt
                goto.append({})
                hit_len.append(0)
                hit_id.append(0)
            st = nxt
        hit_len[st], hit_id[st] = len(s), i          # distinct strings end in distinct nodes
    n = len(goto)
    trans = np.zeros((n, n_classes), dtype=np.uint16)
    fail = [0] * n
    order = []
    for c, t in goto[0].items():                     # breadth first: a state's failure state is shallower, so done before it
        trans[0, c] = t
        order.append(t)
    for st in order:
        f = fail[st]
        if hit_len[st] == 0 and hit_len[f]:          # the longest suffix that is a stop string: the own one, else the link's
            hit_len[st], hit_id[st] = hit_len[f], hit_id[f]
        trans[st] = trans[f]
        for c, t in goto[st].items():
            fail[t] = int(trans[f, c])
            trans[st, c] = t
            order.append(t)
    assert n <= MAX_STATES and n_classes <= MAX_CLASSES
    return StopDFA(stops, trans, byte_class, np.asarray(hit_len, dtype=np.uint8), np.asarray(hit_id, dtype=np.uint8))


def empty_dfa() -> StopDFA:
    """The automaton of no stop string at all: the start state alone.  vis_stop_scan then counts bytes and finds EOS only
    (what streaming needs of it when the request names no stop string)."""
    return StopDFA((), np.zeros((1, 1), dtype=np.uint16), np.zeros(256, dtype=np.uint8), np.zeros(1, dtype=np.uint8),
                   np.zeros(1, dtype=np.uint8))


def depths(dfa: StopDFA) -> np.ndarray:
    """uint8 [n_states]: the depth of every state in the trie - the length of the longest suffix of the text read so far
    that is a prefix of a stop string.  Every transition leads at most one level down and the trie edge into a state comes
    from the level above it, so the depth is the breadth-first distance from the start state."""
    n = dfa.trans.shape[0]
    depth = np.full(n, -1, dtype=np.int64)
    depth[0] = 0
    frontier = [0]
    while frontier:
        nxt = []
        for st in frontier:
            for t in np.unique(dfa.trans[st]):
                if depth[t] < 0:
                    depth[t] = depth[st] + 1
                    nxt.append(int(t))
        frontier = nxt
    assert depth.min() >= 0 and depth.max() <= MAX_STOP_BYTES
    return depth.astype(np.uint8)


def scan(stops, token_bytes_seq: Sequence[bytes], eos_flags: Optional[Sequence[bool]] = None) -> dict:
    """vis_stop_scan in Python over a whole reply: the bytes of each generated token in turn (``eos_flags[i]``: token i is
    an EOS id).  Returns the record as a dict of reason / n_tokens / cut / which / bytes_so_far / state."""
    dfa = stops if isinstance(stops, StopDFA) else compile_stop(stops)
    st = nbytes = ntok = 0
    for i, tb in enumerate(token_bytes_seq):
        if eos_flags is not None and eos_flags[i]:
            return dict(reason=EOS, n_tokens=ntok, cut=nbytes, which=0, bytes_so_far=nbytes, state=st)
        ntok += 1
        for b in bytes(tb):
            st = int(dfa.trans[st, dfa.byte_class[b]])
            nbytes += 1
            if dfa.hit_len[st]:
                return dict(reason=STOP, n_tokens=ntok, cut=nbytes - int(dfa.hit_len[st]), which=int(dfa.hit_id[st]),
                            bytes_so_far=nbytes, state=st)
    return dict(reason=OPEN, n_tokens=ntok, cut=0, which=0, bytes_so_far=nbytes, state=st)


def find_oracle(stops, token_bytes_seq: Sequence[bytes], eos_flags: Optional[Sequence[bool]] = None) -> dict:
    """The rule of the module docstring with ``bytes.find`` -> reason / n_tokens / cut / which."""
    stops = check_stop(stops)
    toks = [bytes(t) for t in token_bytes_seq]
    n_eos = next((i for i in range(len(toks)) if eos_flags is not None and eos_flags[i]), None)
    if n_eos is not None:
        toks = toks[:n_eos]
    stream = b"".join(toks)
    best = None
    for i, s in enumerate(stops):
        at = stream.find(s)
        if at >= 0 and (best is None or (at + len(s), at) < (best[0], best[1])):
            best = (at + len(s), at, i)
    if best is None:
        if n_eos is not None:
            return dict(reason=EOS, n_tokens=n_eos, cut=len(stream), which=0)
        return dict(reason=OPEN, n_tokens=len(toks), cut=0, which=0)
    ends = np.cumsum([len(t) for t in toks])
    return dict(reason=STOP, n_tokens=int(np.searchsorted(ends, best[0], side="left")) + 1, cut=best[1], which=best[2])


def finish_of(record) -> tuple:
    """One slot's record (the STATE_INTS words) as the engines' ``last_finish`` entry: (reason, cut) with reason one of
    "eos" / "stop" / "length" and cut the byte offset of the matched stop string, None unless reason is "stop"."""
    r = int(record[REASON])
    return (REASONS[r], int(record[CUT]) if r == STOP else None)


def host_finish(tokens: Sequence[int], eos_ids, ignore_eos: bool) -> tuple:
    """``last_finish`` entry of a request that ran without stop strings, from what the host holds anyway: "eos" when an EOS
    id lies within the tokens generated (and the run looked for one), else "length"."""
    if not ignore_eos and any(t in eos_ids for t in tokens):
        return ("eos", None)
    return ("length", None)


class StopBuffers:
    """One engine's device state of vis_stop_scan: the token table (shared with the engine's grammar masks, whichever came
    first), the records [slots, 8] int32 and the automaton in tables of fixed capacity with the header the kernel sizes them
    from.  ``load`` overwrites the tables per request group; a captured decode graph holds only their addresses, so it
    serves every stop set."""

    def __init__(self, tokenizer, vocab: int, eos_ids, slots: int, device, share=None):
        import torch
        if share is not None:
            self.table, self.off, self.data, self.flags, self.eos = share.table, share.off, share.data, share.flags, share.eos
        else:
            from .json_grammar import build_token_table
            table = build_token_table(tokenizer, vocab, eos_ids)
            self.table = table
            self.off = torch.from_numpy(table.off).to(device)
            self.data = torch.from_numpy(table.data).to(device)
            self.flags = torch.from_numpy(table.flags).to(device)
            self.eos = torch.from_numpy(table.eos_ids).to(device)
        self.state = torch.zeros((slots, STATE_INTS), dtype=torch.int32, device=device)
        self.header = torch.zeros(HEADER_INTS, dtype=torch.int32, device=device)
        self.trans = torch.zeros((MAX_STATES, MAX_CLASSES), dtype=torch.int16, device=device)      # u16 bits
        self.byte_class = torch.zeros(256, dtype=torch.uint8, device=device)
        self.hits = torch.zeros((MAX_STATES, 2), dtype=torch.uint8, device=device)                 # (hit_len, hit_id)
        self.stops: Optional[tuple] = None
        self.dfa: Optional[StopDFA] = None      # the automaton last loaded

    def load(self, stops, streams=()) -> StopDFA:
        """Make ``stops`` the stop set of the launches that follow.  Called before a request group's first prompt pass,
        outside any captured graph: the copies run on the current stream once everything queued on ``streams`` (the streams
        that launched scans for the previous group) has finished, and those streams then wait for the copies."""
        import torch
        dfa = stops if isinstance(stops, StopDFA) else compile_stop(stops)
        self.dfa = dfa
        n, c = dfa.trans.shape
        if not (1 <= n <= MAX_STATES and 1 <= c <= MAX_CLASSES):
            raise ValueError(f"stop: {n} states x {c} classes exceed the device tables ({MAX_STATES} x {MAX_CLASSES})")
        if dfa.stops == self.stops:
            return dfa
        packed = dfa.trans | np.where(dfa.hit_len[dfa.trans] != 0, HIT, 0).astype(np.uint16)
        cur = torch.cuda.current_stream(self.header.device) if self.header.is_cuda else None
        for s in streams if cur is not None else ():
            cur.wait_stream(s)
        self.trans.view(-1)[:n * c].copy_(torch.from_numpy(np.ascontiguousarray(packed).reshape(-1).view(np.int16)))
        self.byte_class.copy_(torch.from_numpy(np.ascontiguousarray(dfa.byte_class)))
        self.hits[:n].copy_(torch.from_numpy(np.stack([dfa.hit_len, dfa.hit_id], axis=1)))
        self.header.copy_(torch.tensor([n, c, 0, 0], dtype=torch.int32))
        for s in streams if cur is not None else ():
            s.wait_stream(cur)
        self.stops = dfa.stops
        return dfa

    def reset(self, slot: int) -> None:
        """A fresh record for ``slot`` (on the current stream, before the slot's prompt-pass pick)."""
        self.state[slot].zero_()

    def scan(self, tokens, step, slot: int = 0, eos_on: bool = True) -> None:
        """vis_stop_scan for slots slot .. slot + B - 1 (tokens [B, T] or [T], step [B]), after their pick."""
        from . import hip
        t2 = tokens if tokens.dim() == 2 else tokens.view(1, -1)
        B = t2.shape[0]
        hip.stop_scan(self.state[slot:slot + B], t2, step, self.off, self.data, self.flags, self.header, self.trans,
                      self.byte_class, self.hits, eos_on)

    def records(self, slots) -> list:
        """The records of ``slots`` as lists of STATE_INTS ints: one small D2H; synchronises."""
        slots = list(slots)
        lo, hi = min(slots), max(slots) + 1
        st = self.state[lo:hi].cpu().tolist()
        return [st[s - lo] for s in slots]
