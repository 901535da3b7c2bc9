"""The next-token pick and the request switches that steer it (logprobs, JSON mode, a JSON Schema, nucleus sampling /
seeds, penalties, top_k / min_p / logit_bias, no_repeat_ngram_size / bad_words / min_tokens) or watch it (stop strings, streaming): which launches turn a row of logits into a
token, the state behind each switch, and the part of the decode-graph key that depends on them.  Both engines derive from ``PickStage``; nothing else knows this policy."""
from __future__ import annotations

import contextlib
from typing import Dict, Iterable, List, Optional, Sequence

import torch

from . import hip
from .ban import NEUTRAL as BAN_NEUTRAL, BanBuffers, BanRequest, bad_word_ids
from .json_mode import JsonBuffers, SchemaBuffers, check_schema, engine_tokenizer
from .logprobs import LogprobsBuffers, check_k
from .penalties import NEUTRAL, PenaltyBuffers
from .sampling import SLOT_SEED_STRIDE, SampleBuffers, check_top_p
from .shaping import NEUTRAL as SHAPE_NEUTRAL, ShapeBuffers, check_vocab
from .stop import StopBuffers, check_stop, empty_dfa, finish_of, host_finish
from .stream import StreamBuffers, StreamReader


class PickStage:
    """Base class of the engines: works on ``self``, holds no model knowledge.

    Contract - what it reads of the engine, all present before ``_init_pick_stage()`` runs: ``cfg.vocab``, ``cfg.eos_ids``,
    ``max_batch``, ``device``, the per-slot rows ``tokens_b`` [slots, T] / ``logits_b`` [slots, V] / ``step_b`` [slots], the
    pick workspace ``ws_val`` / ``ws_idx`` (>= 256 entries per slot), ``temperature`` and ``seed`` of the request running,
    and ``tokenizer`` (the vocabulary's token_bytes; the client sets it when it loads the model).  The streams of an
    engine's ``_prefill_streams``, where it has any, are ordered around a schema's table upload."""

    def _init_pick_stage(self) -> None:
        # token log-probabilities (generate(..., logprobs=k)): k while a request asks for them, else None; buffers on first use
        self.lp_k: Optional[int] = None
        self._lp: Optional[LogprobsBuffers] = None
        self.last_logprobs: Optional[list] = None
        # JSON mode (generate(..., json_mode=True)): on while a request asks for it; token table and state on first use.
        self.json_on = False
        self._json: Optional[JsonBuffers] = None
        # schema-constrained decoding (generate(..., json_schema=SchemaDFA)): the same pick with vis_schema_mask's rows
        self.schema_on = False
        self._schema: Optional[SchemaBuffers] = None
        # nucleus sampling / per-request seeds (generate(..., top_p=), generate_batch(..., top_p=, seeds=)): while on, every
        # pick is vis_sample_f32 with the row seeds of a device buffer; top_p None = 1; _slot_seed: slot -> request seed
        self.smp_on, self.top_p, self.seeded = False, None, False
        self._smp: Optional[SampleBuffers] = None
        self._slot_seed: Dict[int, int] = {}
        # logit penalties (generate(..., repetition_penalty=, frequency_penalty=, presence_penalty=)): while on, every pick
        # reads the row vis_penalize_f32 wrote instead of the raw logits; _slot_pen: slot -> the request's (r, f, q)
        self.pen_on = False
        self._pen: Optional[PenaltyBuffers] = None
        self._slot_pen: Dict[int, tuple] = {}
        # logit shaping (generate(..., top_k=, min_p=, logit_bias=)): while on, every pick reads the row vis_shape_f32 wrote
        # (after the penalties and the grammar mask); _slot_shape: slot -> the request's (top_k, min_p, bias list)
        self.shape_on = False
        self._shp: Optional[ShapeBuffers] = None
        self._slot_shape: Dict[int, tuple] = {}
        # token bans (generate(..., no_repeat_ngram_size=, bad_words=, min_tokens=)): while on, every pick reads the row
        # vis_ban_f32 wrote (after the penalties, ahead of the grammar mask and the shaping); _slot_ban: slot -> the request's
        # (no_repeat_ngram_size, min_tokens)
        self.ban_on = False
        self._ban: Optional[BanBuffers] = None
        self._slot_ban: Dict[int, tuple] = {}
        # stop strings (generate(..., stop=)): while on, vis_stop_scan follows every pick and the engines poll its records
        # instead of the token rows; stop_eos: whether an EOS id ends a row too (off in a run that ignores EOS)
        self.stop_on, self.stop_eos = False, True
        self._stop: Optional[StopBuffers] = None
        # streaming (generate(..., on_stream=StreamReader)): while on, the stop scan is on too (with the request's stop strings
        # or with the automaton of no string) and vis_stream_publish follows it after every pick; _reader: the request's reader
        self.stream_on = False
        self._stream: Optional[StreamBuffers] = None
        self._reader: Optional[StreamReader] = None
        self._graph_warmup = False      # DecodeStage._captured_step: the step now running will be run again at the same counters
        # how each request of the last run ended: (reason, cut) with reason "eos" / "stop" / "length", None for a failed one
        self.last_finish: Optional[list] = None
        # the device ids of the prompt last picked from in each slot
        self._slot_ids: Dict[int, torch.Tensor] = {}

    # ------------------------------------------------------------------ one request's switches
    @contextlib.contextmanager
    def _pick_request(self, logprobs, json_mode, json_schema, top_p, seeded: bool, penalties: Optional[Sequence[tuple]],
                      stop=None, *, shaping: Optional[Sequence[tuple]] = None, on_stream: Optional[StreamReader] = None,
                      ban: Optional[BanRequest] = None):
        """The switches of one request (or one batch of them) on for the body, and all off again afterwards - also when the
        body, or switching on itself (no tokenizer, a schema the device tables cannot hold), raises.  ``penalties``:
        check_penalties' result; a single request runs in slot 0 and its triple is placed there.  ``stop``: None, a string or
        1..4 of them (check_stop), one set for the whole group.  ``shaping``: check_shaping's result, placed like the penalties.
        ``on_stream``: the StreamReader the group's tokens are published to, or None.  ``ban``: check_ban's result, its rows
        placed like the penalties; not together with JSON mode or a schema."""
        check_k(logprobs)
        check_schema(json_mode, json_schema)
        if not isinstance(json_mode, bool):
            raise ValueError("json_mode must be True or False")
        check_top_p(top_p)
        stop = check_stop(stop)
        if on_stream is not None and not isinstance(on_stream, StreamReader):
            raise ValueError("on_stream must be a stream.StreamReader or None")
        if on_stream is not None and logprobs is not None:
            raise ValueError("on_stream together with logprobs is not supported")
        if ban is not None and (json_mode or json_schema is not None):
            raise ValueError("no_repeat_ngram_size / bad_words / min_tokens together with JSON mode or a JSON schema is not "
                             "supported: a ban could leave the grammar no token")
        try:
            self._begin_logprobs(logprobs)
            self._begin_schema(json_mode, json_schema)
            self._begin_json(json_mode)
            self._begin_sampling(top_p, seeded)
            self._begin_penalties(penalties)
            if penalties is not None and len(penalties) == 1:
                self._slot_pen[0] = penalties[0]
            self._begin_stop(stop if stop is not None or on_stream is None else empty_dfa())
            self._begin_stream(on_stream)
            self._begin_shaping(shaping)
            if shaping is not None and len(shaping) == 1:
                self._slot_shape[0] = shaping[0]
            self._begin_ban(ban)
            if ban is not None and len(ban.rows) == 1:
                self._slot_ban[0] = ban.rows[0]
            yield
        finally:
            self.lp_k = None
            self.json_on = False
            self.schema_on = False
            self._end_sampling()
            self._end_penalties()
            self.stop_on, self.stop_eos = False, True
            if self.stream_on:      # the run is over (its last D2H has drained the stream): the reader hands out the rest
                self._reader._end_group()
            self.stream_on, self._reader = False, None
            self._end_shaping()
            self._end_ban()

    def _pick_key(self) -> tuple:
        """The switches' part of a decode-graph key.  The logprobs k, the masks and top_p are kernel arguments or launches
        baked into a captured step; the row seeds of vis_sample_f32 and the penalty values of vis_penalize_f32 are read from
        device memory at replay, so only whether they are in use is part of it."""
        return (self.lp_k, self.json_on, self.schema_on, self.top_p, self.seeded, self.pen_on)

    def _stop_key(self) -> tuple:
        """The stop scan's part of a decode-graph key, appended by the engines next to _pick_key(): whether the launch is in
        the step and its one switch that is a kernel argument.  The stop strings themselves are read from device tables."""
        return (self.stop_on, self.stop_eos)

    def _shape_key(self) -> tuple:
        """The shaping launch's part of a decode-graph key, appended by the engines next to _stop_key(): whether the launch
        is in the step.  k, delta and the bias lists are read from device memory at replay."""
        return (self.shape_on,)

    def _ban_key(self) -> tuple:
        """The ban launch's part of a decode-graph key, appended by the engines next to _stream_key(): whether the launch is
        in the step, and the lengths of the group's words, which are launch arguments.  n, min_tokens, the prompts and the
        words' ids are read from device memory at replay."""
        return (self.ban_on, self._ban.word_len) if self.ban_on else (False,)

    def _stream_key(self) -> tuple:
        """The publishing launch's part of a decode-graph key, appended by the engines next to _shape_key(): whether the
        launch is in the step.  What it reads and where it writes are device and host addresses fixed for the engine's life."""
        return (self.stream_on,)

    # ------------------------------------------------------------------ token log-probabilities
    def _begin_logprobs(self, logprobs: Optional[int]) -> None:
        """Switch the per-pick logprobs launch on (k alternatives) or off (None) for the request about to run."""
        self.lp_k = check_k(logprobs)
        self.last_logprobs = None
        if self.lp_k is not None and self._lp is None:
            self._lp = LogprobsBuffers(self.max_batch, self.tokens_b.shape[1], self.cfg.vocab, self.device)

    def _logprobs_after_pick(self, B: int, slot: int = 0) -> None:
        """vis_logprobs_f32 on the logits of slots slot .. slot + B - 1, right after their pick (nothing when off)."""
        if self.lp_k is not None:
            self._lp.launch(self.logits_b[slot:slot + B], self.tokens_b[slot:slot + B], self.step_b[slot:slot + B], self.lp_k, slot)

    def _record_logprobs(self, rows: Iterable[Optional[tuple]]) -> None:
        """After the run (the stream has drained): ``last_logprobs`` = one record per request from its (slot, start, length)
        row, None for a request that failed (nothing when off)."""
        if self.lp_k is not None:
            self.last_logprobs = [self._lp.record(*r, self.lp_k) if r is not None else None for r in rows]

    # ------------------------------------------------------------------ JSON mode / JSON Schema
    def _begin_schema(self, json_mode: bool, json_schema) -> None:
        """Switch vis_schema_mask on (with ``json_schema``'s tables on the device) or off for the request group about to run.
        Runs before the group's first prompt pass and outside any captured graph; the engine's prompt-pass streams are ordered
        around the table upload."""
        check_schema(json_mode, json_schema)
        if json_schema is None:
            self.schema_on = False
            return
        if self._schema is None:
            self._schema = SchemaBuffers(engine_tokenizer(self), self.cfg.vocab, self.cfg.eos_ids, self.max_batch, self.device,
                                         share=self._json or self._stop)
        self._schema.load(json_schema, getattr(self, "_prefill_streams", ()))
        self.schema_on = True

    def _begin_json(self, json_mode: bool) -> None:
        """Switch the grammar mask of every pick on or off for the request about to run."""
        if not isinstance(json_mode, bool):
            raise ValueError("json_mode must be True or False")
        if json_mode and self._json is None:
            self._json = JsonBuffers(engine_tokenizer(self), self.cfg.vocab, self.cfg.eos_ids, self.max_batch, self.device,
                                     share=self._schema or self._stop)
        self.json_on = json_mode

    @property
    def _mask(self):
        """The buffers of the grammar mask that is on (JSON mode or a schema), or None."""
        return self._schema if self.schema_on else (self._json if self.json_on else None)

    def _mask_failed(self, slots: Iterable[int]) -> List[int]:
        """After the run: those of ``slots`` whose grammar could not be continued by any token (none when no mask is on);
        synchronises."""
        slots = list(slots)
        if self._mask is None:
            return []
        return [s for s, bad in zip(slots, self._mask.failed(slots)) if bad]

    def _spec_checked(self, sp, toks: List[int]) -> List[int]:
        """After a speculative run (``toks``: the reply as _finish cut it): under a ``grammar`` configuration the plain loop's
        failure outcome - JsonModeError for a reply the vocabulary could not continue - decided from the reply itself."""
        if sp.grammar and self._schema.reply_failed(toks, self.last_finish[0][0] == "eos"):
            self.last_finish = [None]
            raise self._mask_error()
        return toks

    # ------------------------------------------------------------------ nucleus sampling / per-request seeds
    def _begin_sampling(self, top_p, seeded: bool) -> None:
        """Route every pick of the request about to run through vis_sample_f32 when top_p < 1 or it brings its own seeds."""
        top_p = check_top_p(top_p)
        self.top_p = top_p if top_p is not None and top_p < 1.0 else None
        self.seeded = bool(seeded)
        self.smp_on = self.seeded or self.top_p is not None
        if self.smp_on and self._smp is None:
            self._smp = SampleBuffers(self.max_batch, self.cfg.vocab, self.device)

    def _end_sampling(self) -> None:
        self.smp_on, self.top_p, self.seeded = False, None, False
        self._slot_seed = {}

    def _seed_slot(self, slot: int) -> None:
        """Before a prompt pass's pick: the row seed of ``slot`` (the request's own, else the slot-derived one)."""
        if self.smp_on:
            self._smp.set_slot(slot, self._slot_seed.get(slot, self.seed + SLOT_SEED_STRIDE * slot))

    # ------------------------------------------------------------------ logit penalties
    def _begin_penalties(self, penalties: Optional[Sequence[tuple]]) -> None:
        """Route every pick of the request about to run through vis_penalize_f32 when some request of it carries a penalty
        (penalties: check_penalties' result - one (r, f, q) per request, or None = off)."""
        self.pen_on = penalties is not None
        self._slot_pen = {}
        if self.pen_on and self._pen is None:
            self._pen = PenaltyBuffers(self.max_batch, self.cfg.vocab, self.device)

    def _end_penalties(self) -> None:
        self.pen_on = False
        self._slot_pen = {}

    def _penalty_slot(self, slot: int, ids_dev: torch.Tensor) -> None:
        """Before a prompt pass's pick: fresh token statistics of ``slot``, the request's triple and its prompt ids (mllama's
        image token has the id of the vocabulary size: the kernel skips it)."""
        if self.pen_on:
            self._pen.begin(slot, ids_dev, *self._slot_pen.get(slot, NEUTRAL))

    # ------------------------------------------------------------------ logit shaping (top_k, min_p, logit_bias)
    def _begin_shaping(self, shaping: Optional[Sequence[tuple]]) -> None:
        """Route every pick of the request about to run through vis_shape_f32 when some request of it asks for top_k, min_p
        or a logit_bias (shaping: check_shaping's result - one (top_k, min_p, bias list) per request, or None = off)."""
        if shaping is not None:
            check_vocab(shaping, self.cfg.vocab)
        self.shape_on = shaping is not None
        self._slot_shape = {}
        if self.shape_on and self._shp is None:
            self._shp = ShapeBuffers(self.max_batch, self.cfg.vocab, self.device)

    def _end_shaping(self) -> None:
        self.shape_on = False
        self._slot_shape = {}

    def _shape_slot(self, slot: int) -> None:
        """Before a prompt pass's pick: the request's k, its min_p threshold at the temperature it runs at and its bias list
        in the parameter rows of ``slot``."""
        if self.shape_on:
            self._shp.begin(slot, *self._slot_shape.get(slot, SHAPE_NEUTRAL), self.temperature)

    # ------------------------------------------------------------------ token bans (no_repeat_ngram_size, bad_words, min_tokens)
    def _begin_ban(self, ban: Optional[BanRequest]) -> None:
        """Route every pick of the request group about to run through vis_ban_f32 when some request of it asks for
        no_repeat_ngram_size, bad_words or min_tokens (ban: check_ban's result, or None = off).  The words are tokenised here
        with the engine's tokenizer and uploaded before the group's first prompt pass, outside any captured graph."""
        self._slot_ban = {}
        if ban is None:
            self.ban_on = False
            return
        word_ids = bad_word_ids(ban.words, engine_tokenizer(self)) if ban.words else []
        for w in word_ids:
            for t in w:
                if not 0 <= t < self.cfg.vocab:
                    raise ValueError(f"bad_words: token id {t} is outside the vocabulary [0, {self.cfg.vocab})")
        if self._ban is None:
            self._ban = BanBuffers(self.max_batch, self.tokens_b.shape[1], self.cfg.vocab, self.cfg.eos_ids, self.device)
        self._ban.load(word_ids, getattr(self, "_prefill_streams", ()))
        self.ban_on = True

    def _end_ban(self) -> None:
        self.ban_on = False
        self._slot_ban = {}

    def _ban_slot(self, slot: int, ids_dev: torch.Tensor, step: torch.Tensor) -> None:
        """Before a prompt pass's pick: the request's n and min_tokens, its prompt ids and the position its reply starts at
        (``step`` as it stands in front of the pick) in the rows of ``slot``."""
        if self.ban_on:
            self._ban.begin(slot, ids_dev, step, *self._slot_ban.get(slot, BAN_NEUTRAL))

    # ------------------------------------------------------------------ stop strings / how a reply ended
    def _begin_stop(self, stop: Optional[tuple]) -> None:
        """Switch vis_stop_scan on (with the automaton of ``stop``, check_stop's result, on the device) or off for the request
        group about to run.  Runs before the group's first prompt pass and outside any captured graph; the engine's
        prompt-pass streams are ordered around the table upload."""
        self.last_finish = None
        if stop is None:
            self.stop_on = False
            return
        if self._stop is None:
            self._stop = StopBuffers(engine_tokenizer(self), self.cfg.vocab, self.cfg.eos_ids, self.max_batch, self.device,
                                     share=self._json or self._schema)
        self._stop.load(stop, getattr(self, "_prefill_streams", ()))
        self.stop_on = True

    def _stop_after_pick(self, B: int, slot: int = 0) -> None:
        """vis_stop_scan on the token rows of slots slot .. slot + B - 1, right after their pick (nothing when off)."""
        if self.stop_on:
            self._stop.scan(self.tokens_b[slot:slot + B], self.step_b[slot:slot + B], slot, self.stop_eos)

    # ------------------------------------------------------------------ streaming
    def _begin_stream(self, reader: Optional[StreamReader]) -> None:
        """Switch vis_stream_publish on (publishing to ``reader``) or off for the request group about to run.  Runs after
        _begin_stop, before the group's first prompt pass and outside any captured graph.  The device is drained first: the
        slots' host words are reset from the host, which needs every launch of an earlier request to have finished, and the
        depth table is overwritten."""
        self._reader = reader
        if reader is None:
            self.stream_on = False
            return
        if self._stream is None:
            self._stream = StreamBuffers(self.max_batch, self.tokens_b.shape[1], self.device)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._stream.load(self._stop.dfa)
        self._stream.count[:] = 0      # what an earlier request left in the slots: a reader bound before its slot's prompt pass
        #                                must not take it for its own
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        reader._attach(self._stream)
        self.stream_on = True

    def _stream_after_pick(self, B: int, slot: int = 0) -> None:
        """vis_stream_publish for slots slot .. slot + B - 1, behind the stop scan of their pick (nothing when off).  The
        warm-up step of a graph capture publishes nothing: its replay does, and a run that ends before the replay (one new
        token, a cancelled request) must not have handed out a token it does not return."""
        if self.stream_on and not self._graph_warmup:
            self._stream.launch(self._stop.state[slot:slot + B], self.tokens_b[slot:slot + B], self.step_b[slot:slot + B], slot)

    def _stream_bind(self, choice_slots: Sequence[Optional[Sequence[int]]]) -> None:
        """Tell the reader which slot serves which (request, choice): choice_slots[j] = the slots of request j's choices, None
        for a failed request (nothing when off).  Records published before this are kept: the arrays are append-only."""
        if self.stream_on:
            for j, cs in enumerate(choice_slots):
                for i, s in enumerate(cs or ()):
                    self._reader._bind(s, j, i)

    def _stream_cancelled(self) -> bool:
        """The loops' check at a ``check_every`` boundary: the reader's owner has given up on the request."""
        return self.stream_on and self._reader.cancelled

    def _stop_done(self, slots: Iterable[int]) -> bool:
        """The poll while stop strings are on: True when every one of ``slots`` has ended (EOS or a stop string);
        one small D2H, synchronises."""
        return all(r[3] != 0 for r in self._stop.records(slots))

    def _finish(self, rows: Sequence[Optional[tuple]], eos_ids, ignore_eos: bool, keep_eos: bool = False) -> list:
        """After the run: ``last_finish`` = one (reason, cut) per request and the token lists cut where each reply ended.
        ``rows``: per request (slot, tokens generated) or None for a failed one.  With stop strings on, the device records
        say where (an EOS token itself is kept only for ``keep_eos``); off, the host finds the first EOS id in the tokens as
        it always did.  Returns the cut lists (None for a failed request)."""
        eos = set(eos_ids)
        recs = {}
        if self.stop_on:
            slots = [r[0] for r in rows if r is not None]
            recs = dict(zip(slots, self._stop.records(slots))) if slots else {}
        outs, fin = [], []
        for r in rows:
            if r is None:
                outs.append(None)
                fin.append(None)
                continue
            slot, toks = r
            if self.stop_on:
                rec = recs[slot]
                f = finish_of(rec)
                if f[0] != "length":
                    toks = toks[:rec[4] + (1 if keep_eos and f[0] == "eos" else 0)]
            else:
                f = host_finish(toks, eos, ignore_eos)
                if not ignore_eos:
                    toks = toks[:next((i + (1 if keep_eos else 0) for i, t in enumerate(toks) if t in eos), len(toks))]
            outs.append(toks)
            fin.append(f)
        self.last_finish = fin
        return outs

    # ------------------------------------------------------------------ the pick
    def _pick(self, logits, ws_val, ws_idx, tokens, cur_token, step, temperature, seed, slot: int = 0) -> None:
        """The next-token pick of slots slot .. slot + B - 1: vis_argmax_f32, or in JSON mode vis_json_mask + the masked pick;
        vis_sample_f32 (seeds from the device buffer, the JSON rows as its mask) while nucleus sampling / seeds are on.  While
        penalties are on, all of them read the penalised copy of the rows (vis_penalize_f32); the raw rows stay intact.  While
        top_k / min_p / logit_bias are on, vis_shape_f32 runs after the penalties and the mask launch, takes the mask's rows,
        and the pick reads its copy.  While no_repeat_ngram_size / bad_words / min_tokens are on, vis_ban_f32 runs after
        the penalties and ahead of the mask launch: mask, shaping and pick read its copy."""
        if self.pen_on:
            logits = self._pen.apply(logits, tokens, step, slot)
        if self.ban_on:
            logits = self._ban.apply(logits, tokens, step, slot)
        allow = self._mask.mask(tokens, step, slot) if self._mask is not None else None
        if self.shape_on:
            logits = self._shp.apply(logits, slot, allow)
        if self.smp_on:
            self._smp.pick(logits, tokens, cur_token, step, temperature, self.top_p, slot, allow)
        elif allow is None:
            hip.argmax(logits, ws_val, ws_idx, tokens, cur_token, step, temperature, seed)
        else:
            hip.argmax_masked(logits, ws_val, ws_idx, tokens, cur_token, step, allow, temperature, seed)

    def _gemv_pick(self, x, w, logits, ws_val, ws_idx, tokens, cur_token, step, **kw) -> None:
        """The fused lm_head + pick of the single-sequence step (slot 0), masked in JSON mode; while nucleus sampling / seeds,
        penalties, logit shaping or token bans are on, the plain lm_head GEMV writes the f32 logits and _pick follows."""
        if self.smp_on or self.pen_on or self.shape_on or self.ban_on:
            hip.gemv(x, w, logits, norm_w=kw.get("norm_w"), eps=kw.get("eps", 1e-6))
            self._pick(logits, ws_val, ws_idx, tokens, cur_token, step, kw.get("temperature", 0.0), kw.get("seed", 0))
            return
        if self._mask is None:
            hip.gemv_argmax(x, w, logits, ws_val, ws_idx, tokens, cur_token, step, **kw)
            return
        allow = self._mask.mask(tokens, step, 0)
        hip.gemv_argmax_masked(x, w, logits, ws_val, ws_idx, tokens, cur_token, step, allow[0], **kw)

    def _prompt_pick(self, slot: int, ids_dev: torch.Tensor, logits, tokens, cur_token, step) -> None:
        """The first token of ``slot``, from the logits of its prompt's last row: a fresh grammar state, row seed, token
        statistics and shaping parameters, then the pick and its logprobs."""
        self._slot_ids[slot] = ids_dev      # a further choice of this request (DecodeStage._fork_choices) starts from them too
        if self._mask is not None:
            self._mask.reset(slot)
        self._seed_slot(slot)
        self._penalty_slot(slot, ids_dev)
        self._shape_slot(slot)
        self._ban_slot(slot, ids_dev, step)
        ws = slice(256 * slot, 256 * (slot + 1))    # per-slot workspace: prefills of different slots may run concurrently
        # on different streams
        self._pick(logits, self.ws_val[ws], self.ws_idx[ws], tokens, cur_token, step, self.temperature,
                   self.seed + SLOT_SEED_STRIDE * slot, slot)
        self._logprobs_after_pick(1, slot)
        if self.stop_on:
            self._stop.reset(slot)
            self._stop_after_pick(1, slot)
        if self.stream_on:
            self._reader._reset(slot)
            self._stream_after_pick(1, slot)
