"""Token-by-token replies (``stream=True`` of the client, ``on_stream=`` of the engines' generate / generate_batch).

While a request streams, every pick - prompt pass or decode step, single, batched or forked, eager or graph-replayed - is
followed by vis_stop_scan and then one vis_stream_publish launch: it appends one 16-byte record {token id, safe_bytes,
status, cut} per row to HOST memory the GPU writes coherently and then stores the row's ``count`` word with a system-scope
release store.  The decode loop keeps its ``check_every`` launch-ahead: nothing here synchronises.  A ``StreamReader`` on
another thread polls ``count`` (a plain aligned int32 read), takes the new records and hands out text.

Records are indexed like the token row (the token picked at position p has record p); ``start`` is the position of the first
generated token.  Nothing published is ever rewritten, so the reader needs no seqlock and a slow reader loses nothing.
``safe_bytes`` is how much of the reply's byte stream can no longer be taken back: for an open row the bytes so far minus
the depth of the stop automaton's state (text that may still turn out to be the start of a stop string is held back), on EOS
the bytes in front of the EOS token, on a stop match the offset where the match starts.  ``publish_ref`` restates the kernel
in Python, token by token, on ``stop.scan``."""
from __future__ import annotations

import codecs
import threading
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import stop as S

TOKEN, SAFE, STATUS, CUT = range(4)      # words of one record
RECORD_INTS = 4
OPEN, EOS, STOP = S.OPEN, S.EOS, S.STOP


def check_stream(stream) -> bool:
    """Argument check of ``stream=``: None or False (off) or True."""
    if stream is None:
        return False
    if not isinstance(stream, bool):
        raise ValueError("stream must be True, False or None")
    return stream


def check_stream_options(stream_options, streaming: bool) -> bool:
    """OpenAI's ``stream_options`` -> whether a last chunk with the usage is asked for."""
    if stream_options is None:
        return False
    if not streaming:
        raise ValueError("stream_options needs stream=True")
    if not isinstance(stream_options, dict) or set(stream_options) - {"include_usage"} \
            or not isinstance(stream_options.get("include_usage", False), bool):
        raise ValueError("stream_options: only {'include_usage': True or False} is known")
    return bool(stream_options.get("include_usage", False))


def publish_ref(stops, token_bytes_seq: Sequence[bytes], eos_flags: Optional[Sequence[bool]] = None) -> List[Tuple[int, int, int]]:
    """vis_stream_publish in Python over a whole reply: one (safe_bytes, status, cut) per generated token, in order, ending
    with the record of the token that ended the row (an EOS token, or the one that completed a stop string); tokens behind
    it get none.  ``stops``: a stop set, a StopDFA, or None / () for no stop string."""
    if isinstance(stops, S.StopDFA):
        dfa = stops
    else:
        dfa = S.compile_stop(stops) if stops else S.empty_dfa()
    depth = S.depths(dfa)
    out = []
    for i in range(len(token_bytes_seq)):
        r = S.scan(dfa, token_bytes_seq[:i + 1], None if eos_flags is None else eos_flags[:i + 1])
        if r["reason"] == OPEN:
            out.append((r["bytes_so_far"] - int(depth[r["state"]]), OPEN, 0))
        else:
            out.append((r["cut"], r["reason"], r["cut"]))
            break
    return out


class StreamBuffers:
    """One engine's state of vis_stream_publish: the host arrays (records [slots, T, 4], count [slots], start [slots] int32 in
    ONE coherent allocation the engine keeps for its lifetime - captured graphs hold its address), the depth table of the
    stop automaton on the device and the device mirror of count."""

    def __init__(self, slots: int, T: int, device):
        import torch
        from . import hip
        self.slots, self.T = slots, T
        rec_bytes = slots * T * RECORD_INTS * 4
        self.mem = hip.HostCoherent(rec_bytes + 2 * slots * 4)
        self.records = self.mem.array(0, (slots, T, RECORD_INTS))
        self.count = self.mem.array(rec_bytes, (slots,))
        self.start = self.mem.array(rec_bytes + slots * 4, (slots,))
        self._rec_off, self._count_off, self._start_off = 0, rec_bytes, rec_bytes + slots * 4
        self.depth = torch.zeros(S.MAX_STATES, dtype=torch.uint8, device=device)
        self.pub = torch.zeros(slots, dtype=torch.int32, device=device)
        self._dfa = None

    def load(self, dfa: S.StopDFA) -> None:
        """The depth table of ``dfa`` for the launches that follow.  Called before a request group's first prompt pass,
        outside any captured graph and with the device idle (PickStage._begin_stream synchronises around it)."""
        import torch
        if dfa is self._dfa:
            return
        d = np.zeros(S.MAX_STATES, dtype=np.uint8)
        dd = S.depths(dfa)
        d[:len(dd)] = dd
        self.depth.copy_(torch.from_numpy(d))
        self._dfa = dfa

    def reset(self, slot: int) -> None:
        """A fresh row for ``slot``: on the host at once (no launch that writes the slot is in flight: the previous request
        has drained), the device mirror on the current stream, before the slot's prompt-pass pick."""
        self.count[slot] = 0
        self.start[slot] = 0
        self.pub[slot:slot + 1].zero_()

    def launch(self, stop_state, tokens, step, slot: int = 0) -> None:
        """vis_stream_publish for slots slot .. slot + B - 1 (their stop-scan records, token rows and steps), after the
        stop scan of their pick."""
        from . import hip
        t2 = tokens if tokens.dim() == 2 else tokens.view(1, -1)
        B = t2.shape[0]
        dev = self.mem.dev_ptr
        hip.stream_publish(stop_state, t2, step, self.depth, self.pub[slot:slot + B],
                           dev + self._rec_off + slot * self.T * RECORD_INTS * 4, self.T,
                           dev + self._count_off + slot * 4, dev + self._start_off + slot * 4)


class StreamEvent(NamedTuple):
    request: int        # index of the request in the caller's call (StreamReader.requests maps the engine's index)
    choice: int         # index of the choice within the request
    text: str


class _Row:
    """The reader's state of one slot: the reply's bytes as far as they are known, how many records were taken, how many
    bytes went into the decoder."""

    def __init__(self, request: int, choice: int):
        self.request, self.choice = request, choice
        self.decoder = codecs.getincrementaldecoder("utf-8")(errors="replace")
        self.buf = bytearray()
        self.taken = 0          # records taken (position of the next one; 0 = none yet)
        self.safe = 0
        self.status = OPEN
        self.fed = 0            # bytes handed to the decoder
        self.served = b""       # what had been handed out when the slot was reset for a re-served request


class StreamReader:
    """The reader side: created by the caller, handed to an engine as ``on_stream=``, polled from another thread while the
    engine call runs.  ``poll()`` returns the text that became final since the last call as StreamEvents; it reads host
    memory only - it never blocks on the GPU and never calls a HIP function.  Bytes go through an incremental UTF-8 decoder
    (``errors="replace"``), so a character split across tokens comes out once and whole, and the text handed out is what the
    one-shot decode of the finished reply gives.  ``cancel()`` makes the engine's loop end at its next ``check_every``
    boundary; the rows then end as "length".

    The engine drives the rest: ``_attach`` (the buffers), ``_bind`` (slot -> request, choice), ``_reset`` (a slot starts
    over), ``_end_group`` (the engine call has returned and the device is idle: the rest of every row is handed out - up to
    the end for a row that ended on EOS or was cut by a length limit, nothing behind the cut for a stop match).
    A request served again from the start (ChainStalled) resets its slot: the tokens of the second run are identical by
    construction, so the reader checks the new bytes against what it had handed out and continues behind them; nothing is
    delivered twice.  Were they to differ, poll() raises RuntimeError."""

    def __init__(self, tokenizer):
        self.tokenizer = tokenizer
        self.requests: Optional[List[int]] = None      # request j of the engine call under way is this request of the caller's
        self._lock = threading.Lock()
        self._cancel = threading.Event()
        self._buffers: Optional[StreamBuffers] = None
        self._rows: Dict[int, _Row] = {}
        self._queue: List[StreamEvent] = []

    # ---- caller side
    def cancel(self) -> None:
        self._cancel.set()

    @property
    def cancelled(self) -> bool:
        return self._cancel.is_set()

    def poll(self) -> List[StreamEvent]:
        with self._lock:
            self._scan(final=False)
            out, self._queue = self._queue, []
        return out

    # ---- engine side
    def _attach(self, buffers: StreamBuffers) -> None:
        with self._lock:
            self._buffers = buffers

    def _bind(self, slot: int, request: int, choice: int) -> None:
        with self._lock:
            if slot not in self._rows:
                self._rows[slot] = _Row(self.requests[request] if self.requests is not None else request, choice)

    def _reset(self, slot: int) -> None:
        """``slot`` starts over: its host words and the device mirror are zeroed here, under the reader's lock, so that a
        poll never sees half of it.  A row bound already keeps its decoder and what it handed out: the request is being
        served again."""
        with self._lock:
            self._buffers.reset(slot)
            row = self._rows.get(slot)
            if row is not None:
                if not row.served:
                    row.served = bytes(row.buf[:row.fed])
                row.buf = bytearray()
                row.taken, row.safe, row.status = 0, 0, OPEN

    def _end_group(self) -> None:
        with self._lock:
            self._scan(final=True)
            self._rows = {}

    # ---- the work
    def _take(self, slot: int, row: _Row) -> None:
        """New records of ``slot`` -> row.buf / row.safe / row.status."""
        b = self._buffers
        c = int(b.count[slot])            # the release store behind the records: everything below c is in place
        if c <= 0 or row.status != OPEN:
            return
        lo = row.taken if row.taken else int(b.start[slot])
        c = min(c, b.T)
        for p in range(lo, c):
            tok, safe, status, _ = (int(v) for v in b.records[slot, p])
            if status == OPEN or status == STOP:      # an EOS token adds no byte
                row.buf += self.tokenizer.token_bytes(tok)
            row.safe, row.status = safe, status
            if status != OPEN:
                break
        row.taken = c

    def _feed(self, row: _Row, upto: int, final: bool) -> None:
        upto = min(upto, len(row.buf))
        if row.served:
            n = min(len(row.served), len(row.buf))
            if bytes(row.buf[:n]) != row.served[:n]:
                raise RuntimeError("stream: a request served again produced other bytes than were handed out")
        text = ""
        if upto > row.fed:
            text = row.decoder.decode(bytes(row.buf[row.fed:upto]))
            row.fed = upto
        if final:
            text += row.decoder.decode(b"", final=True)
        if text:
            self._queue.append(StreamEvent(row.request, row.choice, text))

    def _scan(self, final: bool) -> None:
        if self._buffers is None:
            return
        for slot, row in self._rows.items():
            self._take(slot, row)
            if final:
                # EOS: safe is the end; stop: the cut; still open (a length limit, a cancelled run): everything there is
                self._feed(row, len(row.buf) if row.status == OPEN else row.safe, True)
            else:
                self._feed(row, row.safe, False)
