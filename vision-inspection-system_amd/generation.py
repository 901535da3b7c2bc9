"""What drives a request through an engine: the checks of its arguments, the routes of one request and of one choice, the
scope of the pick's switches, the prompt pass(es), the poll-and-decode loop, the timing record and the shaping of the
results - once, for the single sequence and for a batch.  ``decode_stage.py`` knows the step and ``pick.py`` the pick; both
engines derive from ``Generation`` and keep only what their models do differently, behind the hooks named in its docstring."""
from __future__ import annotations

import logging
from dataclasses import replace
from typing import List, Sequence

import torch

from . import hip, spec, spec_batch
from .ban import check_ban
from .decode_stage import DecodeStage
from .fork import check_n_list
from .json_mode import JsonModeError, check_schema
from .logprobs import check_k
from .penalties import check_penalties
from .request import Switches
from .sampling import check_seeds, check_top_p
from .shaping import check_shaping
from .stop import check_stop

_LOG = logging.getLogger("vision_inspection_system_amd.engine")


class Generation(DecodeStage):
    """Base class of the engines: works on ``self``, holds no model knowledge.

    The engines' public ``generate`` / ``generate_batch`` keep their own spellings (Qwen2-VL: ``ignore_eos`` / ``check_every``
    / ``frames``; Mllama: ``stop_on_eos`` / ``chunk`` / ``frame``) and hand over to ``_generate`` / ``_generate_batch`` here,
    which know one spelling: ``ignore_eos``, ``check_every``, ``frames`` (whatever the engine's prompt pass takes as images),
    and take every further keyword of theirs as one request.Switches.
    What an engine supplies:
      ``_prompt_pass(input_ids, frames, max_new_tokens, temperature, seed)``: the single sequence's prompt pass into slot 0;
      ``prefill_many(requests, temperature=, seed=, max_new_tokens=, seeds=, penalties=, shaping=[, ban=]) -> (slots,
        errors)``: the prompt passes of a batch into consecutive slots; a lazy request that failed has no slot and its
        exception (``ban`` is passed only while token bans are on);
      ``_batch_graph(B)``: the captured batched step under the engine's own graph key;
      ``decode(n_steps, use_graph=)``: n further tokens of the single sequence, its own bounds checked;
    and may override: ``keep_eos``, ``lazy_single_owns_failure``, ``single_route_check_every``, ``_fork_prefix_len()``,
    ``_clamp_request()``, ``_check_batch()``, ``disable_chain()`` and ``_maybe_reenable_chain()`` - each difference between the
    models is written down at its definition below."""

    # Whether a reply that ended on EOS keeps the EOS token (Mllama) or is cut in front of it (Qwen2-VL).
    keep_eos = False
    # generate_batch with ONE lazy request: whether every failure of it (its prompt pass's too) becomes its entry in the
    # returned list (Mllama), or only the failure of its callable while the rest propagates (Qwen2-VL).
    lazy_single_owns_failure = False
    # generate_batch with ONE request takes the single-sequence loop: polled at the call's own interval (None, Qwen2-VL) or
    # at this one whatever the call said (Mllama: 32, the default ``chunk`` of its ``generate``).
    single_route_check_every = None
    # generate(.., speculative=): the Qwen2-VL / Qwen2.5-VL engine, and an MllamaEngine built with speculative=True (its
    # cross-attention rows take vis_decode_cross_attn_draft / _fp8_draft; the instance then sets this).  The class default -
    # and with it an engine built without the keyword - refuses.
    speculative_supported = False

    # ------------------------------------------------------------------ hooks with a default
    def _fork_prefix_len(self) -> int:
        """The text prefix every root of the batch just prefilled reads from slot 0 (fork.fork_layout).  Qwen2-VL:
        ``batch_shared_len``; Mllama shares no prefix."""
        return 0

    def _clamp_request(self, input_ids: Sequence[int], max_new_tokens: int) -> int:
        """``max_new_tokens`` as the single sequence's prompt pass gets it.  Qwen2-VL clamps it to the context here and says
        so once per engine; Mllama's prompt pass does not take it, the loop's own silent clamp behind the prompt pass is all."""
        return max_new_tokens

    def _check_batch(self, requests: Sequence) -> None:
        """What a batch of more than one sequence must satisfy besides the shared checks (Mllama: an image in every request)."""

    def disable_chain(self) -> None:
        """After a stalled chained launch: this engine decodes on the four launches per layer head, for good; the captured
        graphs hold chained launches and are dropped.  Qwen2-VL keeps the chain's workspace instead and comes back to it
        (``_maybe_reenable_chain``)."""
        self.chain_sync = None
        self._graphs.clear()

    def _maybe_reenable_chain(self) -> None:
        """After a single-sequence request served without a stall.  Only Qwen2-VL switches the chain back on."""

    # ------------------------------------------------------------------ the single sequence
    def _generate(self, input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                  sw: Switches) -> List[int]:
        """Generate up to max_new_tokens (greedy at temperature 0).  EOS is checked on the host every ``check_every`` tokens so
        the decode loop itself never synchronises; output is truncated at the first EOS (exclusive; inclusive for an engine
        with ``keep_eos``).  ``sw``: what the request switches on (request.Switches describes every switch)."""
        pred = spec.check_prediction_ids(sw.prediction, getattr(self, "max_ctx", None))
        sp = spec.with_prediction(sw.speculative, pred is not None)
        if sp is not None:
            what = "speculative" if pred is None else "prediction (speculative decoding)"
            if not self.speculative_supported:
                raise ValueError(("speculative decoding is" if pred is None else "prediction (speculative decoding) is") +
                                 " offered by the Qwen2-VL / Qwen2.5-VL engine only, unless an MllamaEngine is built for it: "
                                 "MllamaEngine(.., speculative=True), or VIS_AUDITOR_SPECULATIVE=k (1..3) where the client "
                                 "loads it")
            spec.check_exclusive(sp, temperature, seed, what=what, **sw.exclusive())
        penalties = check_penalties(sw.repetition_penalty, sw.frequency_penalty, sw.presence_penalty, 1)
        shaping = check_shaping(sw.top_k, sw.min_p, sw.logit_bias, 1)
        ban = check_ban(sw.no_repeat_ngram_size, sw.bad_words, sw.min_tokens, 1, max_new_tokens, json_mode=sw.json_mode,
                        json_schema=sw.json_schema)
        with self._pick_request(sw.logprobs, sw.json_mode, sw.json_schema, sw.top_p, False, penalties, stop=sw.stop,
                                shaping=shaping, on_stream=sw.on_stream, **({} if ban is None else {"ban": ban})):
            self.stop_eos = not ignore_eos
            self._stream_bind([[0]])
            max_new_tokens = self._clamp_request(input_ids, max_new_tokens)
            if sp is not None:      # no chained launch in a speculative step: nothing of the stall handling below applies
                return self._run_single_spec(sp, input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, pred, temperature, seed)
            try:
                out = self._run_single(input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed)
                self._maybe_reenable_chain()
                return out
            except hip.ChainStalled as e:
                # Something else held CU slots this launch's producers needed (another PROCESS sharing the GPU, or other work
                # of this process on another stream: chained launches of this process are ordered, DecodeStage._decode_ordered,
                # everything else is covered by the bounded wait only).  From the launch after the stall on every chained
                # launch of the request returned at once (status word read at kernel entry), so what was lost is one wait
                # bound.  The request is served again on the unchained launches - the same HIP kernels' arithmetic, identical
                # tokens - and the engine stays on them (disable_chain says for how long).
                _LOG.warning("%s - continuing on the unchained decode step", e)
                self.disable_chain()
                return self._run_single(input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed)

    def _run_single(self, input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed) -> List[int]:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]      # per-stage device time (tracing)
        ev[0].record()
        self._prompt_pass(input_ids, frames, max_new_tokens, temperature, seed)
        ev[1].record()
        max_new_tokens = min(max_new_tokens, self.max_ctx - len(input_ids) - 1)      # silent; nothing left to cut after _clamp_request
        done, eos = 1, set(self.cfg.eos_ids)
        while done < max_new_tokens and not self._stream_cancelled():
            if self.stop_on:
                if self._stop_done([0]):
                    break
            elif not ignore_eos and any(t in eos for t in self.generated(done)):
                break
            # a run that ignores EOS and has neither stop strings nor a reader is issued in one go: nothing to poll for
            n = min(check_every if not ignore_eos or self.stop_on else max_new_tokens, max_new_tokens - done)
            self.decode(n, use_graph=use_graph)
            done += n
        ev[2].record()
        toks = self.generated(done)                                         # D2H: synchronises, the events have completed
        self.last_timing = {"prompt_tokens": len(input_ids), "prefill_ms": ev[0].elapsed_time(ev[1]),
                            "decode_ms": ev[1].elapsed_time(ev[2]), "decode_steps": done - 1, "sequences": 1}
        toks = self._finish([(0, toks)], eos, ignore_eos, keep_eos=self.keep_eos)[0]
        self._record_logprobs([(0, self.prompt_len - 1, len(toks))])
        if self._mask_failed([0]):
            self.last_finish = [None]
            raise self._mask_error()
        return toks

    def _run_single_spec(self, sp: "spec.SpecConfig", input_ids, frames, max_new_tokens, ignore_eos, use_graph,
                         check_every, prediction=None, temperature=0.0, seed=0) -> List[int]:
        """_run_single with speculative steps: ``check_every`` steps are issued ahead as there, then the poll reads the device
        step counter together with the token row - a step has produced 1..R tokens.  Ends at EOS or when the reply has
        max_new_tokens tokens (the device ``limit`` cuts the last step's run there; steps issued past it change nothing)."""
        R = sp.rows
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        self._prompt_pass(input_ids, frames, max_new_tokens + R - 1, temperature or 0.0, seed or 0)      # + rope rows past the last token
        ev[1].record()
        max_new_tokens = max(1, min(max_new_tokens, self.max_ctx - len(input_ids) - 1))
        buf = self._spec_begin(sp, max_new_tokens, prediction)
        start, eos = self.prompt_len - 1, set(self.cfg.eos_ids)

        def poll():      # one D2H each: the step counter, then the tokens it covers
            n = min(int(self.step.item()) - start, max_new_tokens)
            return self.tokens[start:start + n].cpu().tolist()

        toks, steps = poll(), 0
        while len(toks) < max_new_tokens and (ignore_eos or not any(t in eos for t in toks)):
            n = min(check_every, max_new_tokens - len(toks))
            self._decode_steps_spec(n, R, use_graph)
            steps += n
            toks = poll()
        ev[2].record()
        torch.cuda.current_stream().synchronize()
        self._decoded = len(toks) - 1
        c = buf.read_counters()
        self.last_timing = {"prompt_tokens": len(input_ids), "prefill_ms": ev[0].elapsed_time(ev[1]),
                            "decode_ms": ev[1].elapsed_time(ev[2]), "decode_steps": steps, "sequences": 1,
                            "spec_steps": c[0], "spec_proposed": c[1], "spec_accepted": c[2]}
        if prediction:
            st = buf.read_pred_state()
            self.last_timing.update(pred_accepted=st.accepted, pred_rejected=st.rejected)
        toks = self._finish([(0, toks)], eos, ignore_eos, keep_eos=self.keep_eos)[0]
        self._record_logprobs([(0, self.prompt_len - 1, len(toks))])
        return self._spec_checked(sp, toks)

    @staticmethod
    def _mask_error() -> JsonModeError:
        return JsonModeError("json_mode: the vocabulary could not continue the JSON text")

    # ------------------------------------------------------------------ a batch
    def _generate_batch(self, requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                        sw: Switches) -> list:
        """requests: [(input_ids, frames)] for up to max_batch images - or zero-argument callables returning that pair
        (see prefill_many: resolved in order while the GPU already works on the earlier ones).  Prefill runs per image
        (M = S rows is already MFMA-efficient); the decode steps are shared: one weight pass per step for all sequences.
        Returns one token list per request; for a lazy request whose callable raised, the exception object instead.
        ``sw``: what the group switches on (request.Switches: every switch, and which take one value per request)."""
        n_req = len(requests)
        if not 1 <= n_req <= self.max_batch:
            raise ValueError(f"batch of {n_req} does not fit max_batch={self.max_batch}")
        check_k(sw.logprobs)
        if not isinstance(sw.json_mode, bool):
            raise ValueError("json_mode must be True or False")
        check_schema(sw.json_mode, sw.json_schema)
        check_top_p(sw.top_p)
        seeds = check_seeds(sw.seeds, n_req)
        penalties = check_penalties(sw.repetition_penalty, sw.frequency_penalty, sw.presence_penalty, n_req)
        shaping = check_shaping(sw.top_k, sw.min_p, sw.logit_bias, n_req)
        ban = check_ban(sw.no_repeat_ngram_size, sw.bad_words, sw.min_tokens, n_req, max_new_tokens, json_mode=sw.json_mode,
                        json_schema=sw.json_schema)
        check_stop(sw.stop)
        ns = check_n_list(sw.n, n_req, self.max_batch)
        if n_req == 1 and ns is not None and ns[0] == 1:      # one choice: the route without n, the results nested
            out = self._generate_batch(requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                                       replace(sw, n=None))
            if not isinstance(out[0], Exception):
                out = [[out[0]]]
                self.last_finish = [[self.last_finish[0]]]
                if self.last_logprobs is not None:
                    self.last_logprobs = [[self.last_logprobs[0]]]
            return out
        if n_req == 1 and ns is None:
            # one request (always the case with max_batch == 1, where the batched buffers need not exist): the single-sequence
            # loop; a lazy request's failure stays its own, as in the batched form
            r, own = requests[0], False

            def failed(e):
                self.last_logprobs = [None] if sw.logprobs is not None else None
                self.last_finish = [None]
                return [e]

            if callable(r):
                own = self.lazy_single_owns_failure
                try:
                    r = r()
                except Exception as e:      # noqa: BLE001
                    return failed(e)
            try:
                return [self._generate(r[0], r[1], max_new_tokens, ignore_eos, use_graph,
                                       self.single_route_check_every or check_every, temperature,
                                       seed if seeds is None else seeds[0], sw.request(0))]
            except Exception as e:      # noqa: BLE001
                if own:
                    return failed(e)
                if isinstance(e, JsonModeError):
                    return [e]
                raise
        self._check_batch(requests)
        with self._pick_request(sw.logprobs, sw.json_mode, sw.json_schema, sw.top_p, seeds is not None, penalties,
                                stop=sw.stop, shaping=shaping, on_stream=sw.on_stream, **({} if ban is None else {"ban": ban})):
            self.stop_eos = not ignore_eos
            try:
                return self._run_batch(requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                                       seeds, penalties, shaping, ns, ban)
            finally:
                self.fork_on = False

    def _run_batch(self, requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed, seeds, penalties,
                   shaping, ns, ban=None) -> list:
        n_req = len(requests)
        # every prompt's own limit (prompt + new tokens <= context) is applied by its prefill; the shared loop below
        # runs to the limit of the longest one
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        # an engine built with batch_speculative (spec_batch.py): its configuration where this batch may take the speculative
        # step, else None; the prompt passes then prepare rope rows for the R - 1 positions a step's rows reach past the reply
        sb = spec_batch.plan(self, n_req, ns, temperature)
        slots, errors = self.prefill_many(requests, temperature=temperature, seed=seed,
                                          max_new_tokens=max_new_tokens + (sb.rows - 1 if sb else 0),
                                          seeds=seeds, penalties=penalties, shaping=shaping,
                                          **({} if ban is None else {"ban": ban.rows}))
        ev[1].record()
        live = [b for b in range(n_req) if slots[b] is not None]
        if not live:
            self._record_logprobs([None] * n_req)
            self.last_finish = [None] * n_req
            return list(errors)
        # the further choices of every request: slots behind the roots', forked from them (no launch and no copy without them)
        choice_slots = self._fork_choices(slots, ns or [1] * n_req, self._fork_prefix_len(), seeds, penalties, shaping)
        self._stream_bind(choice_slots)
        B = sum(len(cs) for cs in choice_slots if cs is not None)
        longest = max(self.slot_prompt_len[slots[b]] for b in live)      # a further choice's prompt is its root's
        max_new_tokens = max(1, min(max_new_tokens, self.max_ctx - longest - 1))
        eos = set(self.cfg.eos_ids)
        starts = [self.slot_prompt_len[s] - 1 for s in range(B)]

        def collect(n):
            t = self.tokens_b[:B].cpu()
            return [t[b, starts[b]:starts[b] + n].tolist() for b in range(B)]

        done, spec_t = 1, {}
        spec_on = sb is not None and len(live) == n_req      # every request live: the plain replies in fewer steps
        if spec_on:
            outs, steps, spec_t = spec_batch.run(self, sb, B, starts, max_new_tokens, eos, ignore_eos, use_graph, check_every,
                                                 temperature)
            done = steps + 1
        g = self._batch_graph(B) if use_graph and not spec_on else None
        while not spec_on and done < max_new_tokens and not self._stream_cancelled():
            if self.stop_on:
                if self._stop_done(range(B)):
                    break
            elif not ignore_eos and all(any(t in eos for t in seq) for seq in collect(done)):
                break
            n = min(check_every if not ignore_eos or self.stop_on else max_new_tokens, max_new_tokens - done)
            for _ in range(n):
                if g is not None:
                    g.replay()
                else:
                    self._decode_step_batched(B)
            done += n
        ev[2].record()
        if spec_on:      # its last poll has the tokens; the event has to complete
            torch.cuda.current_stream().synchronize()
        else:
            outs = collect(done)
        # host waiting for the lazy requests' decodes is inside prefill_ms here: it is the time until all prompts are in
        self.last_timing = {"prompt_tokens": longest, "prefill_ms": ev[0].elapsed_time(ev[1]),
                            "decode_ms": ev[1].elapsed_time(ev[2]), "decode_steps": done - 1, "sequences": B, **spec_t}
        return self._gather_choices(choice_slots, errors, outs, starts, eos, ignore_eos, self.keep_eos, ns is not None,
                                    self._mask_error)
