"""What drives a request through an engine: the checks of its arguments, the routes of one request and of one choice, the
scope of the pick's switches, the prompt pass(es), the poll-and-decode loop, the timing record and the shaping of the
results - once, for the single sequence and for a batch.  ``decode_stage.py`` knows the step and ``pick.py`` the pick; both
engines derive from ``Generation`` and keep only what their models do differently, behind the hooks named in its docstring."""
from __future__ import annotations

import logging
from typing import List, Sequence

import torch

from . import hip, spec
from .ban import ban_kwargs, check_ban
from .decode_stage import DecodeStage
from .fork import check_n_list
from .json_mode import JsonModeError, check_schema
from .logprobs import check_k
from .penalties import check_penalties
from .sampling import check_seeds, check_top_p
from .shaping import check_shaping, shaping_kwargs
from .stop import check_stop

_LOG = logging.getLogger("vision_inspection_system_amd.engine")
_PENALTY_NAMES = ("repetition_penalty", "frequency_penalty", "presence_penalty")


class Generation(DecodeStage):
    """Base class of the engines: works on ``self``, holds no model knowledge.

    The engines' public ``generate`` / ``generate_batch`` keep their own spellings (Qwen2-VL: ``ignore_eos`` / ``check_every``
    / ``frames``; Mllama: ``stop_on_eos`` / ``chunk`` / ``frame``) and hand over to ``_generate`` / ``_generate_batch`` here,
    which know one spelling: ``ignore_eos``, ``check_every``, ``frames`` (whatever the engine's prompt pass takes as images).
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
    def _generate(self, input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed, *,
                  logprobs=None, json_mode=False, top_p=None, repetition_penalty=None, frequency_penalty=None,
                  presence_penalty=None, json_schema=None, stop=None, top_k=None, min_p=None, logit_bias=None,
                  on_stream=None, no_repeat_ngram_size=None, bad_words=None, min_tokens=None, speculative=None,
                  prediction=None) -> List[int]:
        """Generate up to max_new_tokens (greedy at temperature 0).  EOS is checked on the host every
        ``check_every`` tokens so the decode loop itself never synchronises; output is truncated at the
        first EOS (exclusive; inclusive for an engine with ``keep_eos``).  ``logprobs`` = k in 0..20: afterwards
        ``last_logprobs`` holds one TokenLogprobs record
        (log-softmax of the raw logits - independent of temperature and seed - for every returned token, plus its k most
        likely alternatives); None = off, no extra launch.  ``json_mode``: every pick is restricted to the tokens that
        continue a JSON object (json_grammar; needs ``self.tokenizer``): the reply is a prefix of one, complete when it
        ended on EOS; JsonModeError when the vocabulary could not continue it.  Logprobs keep their meaning (raw logits),
        so top_logprobs may list tokens the mask forbade.  ``top_p`` in [0, 1]: nucleus sampling (sampling.py) - each pick
        draws from the shortest most-likely prefix holding top_p of the temperature-scaled mass; None or 1 = off.
        ``repetition_penalty`` > 0 (transformers' meaning: over prompt and generated ids), ``frequency_penalty`` /
        ``presence_penalty`` in [-2, 2] (OpenAI's: over generated ids): penalties.py - applied to the raw logits ahead of
        everything above; None or 1 / 0 / 0 = off.  Logprobs keep their meaning (raw logits).
        ``json_schema`` (a json_schema.SchemaDFA): as ``json_mode``, with the schema's compiled DFA as the grammar
        (vis_schema_mask): a reply that ended on EOS is a document of the schema.  Not together with ``json_mode``.
        ``stop``: a string or 1..4 of them (stop.py): the reply ends with the token that completes the first occurrence of
        one in its bytes (vis_stop_scan after every pick; the poll then reads its records, not the token row), also in an
        ``ignore_eos`` run.  Afterwards, always, ``last_finish`` = [(reason, cut)]: "eos", "stop" (cut = the byte offset in
        the returned tokens' bytes where the stop string starts) or "length" (max_new_tokens, the context clamp, or an
        ``ignore_eos`` run that matched nothing).
        ``top_k`` >= 1, ``min_p`` in [0, 1] (transformers' TopKLogitsWarper / MinPLogitsWarper) and ``logit_bias`` {token id:
        bias in [-100, 100]}, at most 300 entries (OpenAI's): shaping.py - one launch ahead of the pick adds the biases to
        the (penalised) logits, then takes out every token below the k-th largest allowed one or less likely than min_p
        times the most likely one; top_p and the draw see the rest.  None / 0 / {} = off; a greedy request is affected by
        logit_bias only.  Logprobs keep their meaning (raw logits).
        ``on_stream`` (a stream.StreamReader the caller polls from another thread): every token is published to it while the
        loop runs - vis_stream_publish after every pick, behind the stop scan, which is then on with or without ``stop`` -
        and the loop keeps its launch-ahead.  ``on_stream.cancel()`` ends the loop at its next ``check_every`` boundary (the
        reply then ended as "length").  Not together with ``logprobs``.  A request served again after a stalled chained
        launch resets the reader's slot; the reader continues behind what it had handed out (stream.py).
        ``no_repeat_ngram_size`` in 1..64 (transformers' NoRepeatNGramLogitsProcessor: no n-gram of prompt + reply occurs
        twice), ``bad_words``, up to 16 strings of 1..8 token ids each (transformers' NoBadWordsLogitsProcessor / vLLM's: the
        token that would complete one is never picked; a word the tokenizer spells differently behind a space is banned in
        both spellings) and ``min_tokens`` <= max_new_tokens (vLLM's: no EOS id before that many tokens): ban.py - one launch
        after the penalties takes the banned ids out of the pick.  None / 0 / [] = off.  Not together with ``json_mode`` /
        ``json_schema`` (ValueError: a ban could leave the grammar no token).  ``min_tokens`` holds back EOS ids only: a
        ``stop`` string may still end the reply earlier.  Logprobs keep their meaning (raw logits).
        ``speculative``: None (off: exactly the launches of before), the integer k in 1..3 or {"method": "ngram",
        "num_speculative_tokens": k, "prompt_lookup_max": 4, "prompt_lookup_min": 2} (spec.py): a decode step carries the
        current token and up to k ids drafted by prompt lookup over prompt + reply through ONE pass over the weights and
        keeps the drafts the model's own greedy picks confirm - the reply is the plain reply token for token, in fewer
        weight passes where the reply repeats earlier text.  Greedy single requests of the Qwen2-VL engines, or of an
        MllamaEngine built with speculative=True, only: ValueError
        with a temperature, a seed or any switch above (they advance one token at a time).  Afterwards ``last_timing`` holds
        ``spec_steps`` / ``spec_proposed`` / ``spec_accepted``.
        ``prediction``: a sequence of token ids the reply will probably repeat (OpenAI's Predicted Outputs; at most max_ctx
        are kept, none = off): the drafts come from it while the reply follows it, and from prompt lookup where it does not
        (spec.propose_pred, vis_spec_draft_pred).  Alone it implies speculative = k 3, window 4..2; ``speculative`` next to it
        sets k and the window.  The same conditions and refusals as ``speculative``; the reply is the plain reply.  Afterwards
        ``last_timing`` also holds ``pred_accepted`` / ``pred_rejected``: the prediction's drafts the steps kept and did not
        keep, over every step issued."""
        pred = spec.check_prediction_ids(prediction, getattr(self, "max_ctx", None))
        sp = spec.with_prediction(speculative, pred is not None)
        if sp is not None:
            what = "speculative" if pred is None else "prediction (speculative decoding)"
            if not self.speculative_supported:
                raise ValueError(("speculative decoding is" if pred is None else "prediction (speculative decoding) is") +
                                 " offered by the Qwen2-VL / Qwen2.5-VL engine only, unless an MllamaEngine is built for it: "
                                 "MllamaEngine(.., speculative=True), or VIS_AUDITOR_SPECULATIVE=k (1..3) where the client "
                                 "loads it")
            spec.check_exclusive(sp, temperature, seed, what=what, logprobs=logprobs, json_mode=json_mode, top_p=top_p,
                                 repetition_penalty=repetition_penalty, frequency_penalty=frequency_penalty,
                                 presence_penalty=presence_penalty, json_schema=json_schema, stop=stop, top_k=top_k,
                                 min_p=min_p, logit_bias=logit_bias, on_stream=on_stream,
                                 no_repeat_ngram_size=no_repeat_ngram_size, bad_words=bad_words, min_tokens=min_tokens)
        penalties = check_penalties(repetition_penalty, frequency_penalty, presence_penalty, 1)
        shaping = check_shaping(top_k, min_p, logit_bias, 1)
        ban = check_ban(no_repeat_ngram_size, bad_words, min_tokens, 1, max_new_tokens, json_mode=json_mode,
                        json_schema=json_schema)
        with self._pick_request(logprobs, json_mode, json_schema, top_p, False, penalties, stop=stop, shaping=shaping,
                                on_stream=on_stream, **({} if ban is None else {"ban": ban})):
            self.stop_eos = not ignore_eos
            self._stream_bind([[0]])
            max_new_tokens = self._clamp_request(input_ids, max_new_tokens)
            if sp is not None:      # no chained launch in a speculative step: nothing of the stall handling below applies
                return self._run_single_spec(sp, input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, pred)
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
                         check_every, prediction=None) -> List[int]:
        """_run_single with speculative steps: ``check_every`` steps are issued ahead as there, then the poll reads the device
        step counter together with the token row - a step has produced 1..R tokens.  Ends at EOS or when the reply has
        max_new_tokens tokens (the device ``limit`` cuts the last step's run there; steps issued past it change nothing)."""
        R = sp.rows
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        self._prompt_pass(input_ids, frames, max_new_tokens + R - 1, 0.0, 0)      # rope rows for the rows past the last token
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
        return toks

    @staticmethod
    def _mask_error() -> JsonModeError:
        return JsonModeError("json_mode: the vocabulary could not continue the JSON text")

    # ------------------------------------------------------------------ a batch
    def _generate_batch(self, requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed, *,
                        logprobs=None, json_mode=False, top_p=None, seeds=None, repetition_penalty=None,
                        frequency_penalty=None, presence_penalty=None, json_schema=None, stop=None, top_k=None, min_p=None,
                        logit_bias=None, n=None, on_stream=None, no_repeat_ngram_size=None, bad_words=None,
                        min_tokens=None) -> list:
        """requests: [(input_ids, frames)] for up to max_batch images - or zero-argument callables returning that pair
        (see prefill_many: resolved in order while the GPU already works on the earlier ones).  Prefill runs per image
        (M = S rows is already MFMA-efficient); the decode steps are shared: one weight pass per step for all sequences.
        Returns one token list per request; for a lazy request whose callable raised, the exception object instead.
        ``logprobs``: as in generate; ``last_logprobs`` then holds one record per request (None for a failed one).
        ``json_mode``: as in generate; a request whose JSON text could not be continued gets a JsonModeError.
        ``top_p``: as in generate.  ``seeds``: one integer per request, its own sampling seed in place of the slot-derived
        one, so a request's sampled reply does not depend on its slot or on what shares the batch.
        ``repetition_penalty``, ``frequency_penalty``, ``presence_penalty``: as in generate, each a number or a sequence
        with one value per request.  ``json_schema``: as in generate, one schema for the whole group.  ``stop``: as in
        generate, one set for the whole group; the shared loop ends when every row has ended.  ``last_finish`` holds one
        (reason, cut) per request, None for a failed one.  ``top_k``, ``min_p``, ``logit_bias``: as in generate, each one
        value for the group or a sequence with one value (or None) per request.
        ``n``: None, an integer >= 1 or one integer per request - that many sampled choices of each request from ONE prompt
        pass (fork.py): the further choices take slots behind the requests', read the prompt's keys / values from the slot
        that ran the prompt pass (vis_decode_attn_forked) and sample with seeds[j] + i (without seeds: the slot-derived seed
        of the slot they land in).  All choices together must fit max_batch.  With ``n`` given, the entry of a request is a
        list of n[j] token lists (for a failed request the exception object, as without), and ``last_logprobs`` /
        ``last_finish`` nest the same way.  At temperature 0 all choices of a request are equal; they are decoded all the
        same.  A slot is still a full-size cache: ``n`` saves prompt passes and attention traffic, not cache memory.
        ``on_stream``: as in generate, one reader for the whole group; its events name the request and the choice.
        ``no_repeat_ngram_size``, ``min_tokens``: as in generate, each one value for the group or a sequence with one value
        per request; ``bad_words``: as in generate, one list for the whole group.  The choices of a request (``n``) inherit
        its values."""
        n_req = len(requests)
        if not 1 <= n_req <= self.max_batch:
            raise ValueError(f"batch of {n_req} does not fit max_batch={self.max_batch}")
        check_k(logprobs)
        if not isinstance(json_mode, bool):
            raise ValueError("json_mode must be True or False")
        check_schema(json_mode, json_schema)
        check_top_p(top_p)
        seeds = check_seeds(seeds, n_req)
        penalties = check_penalties(repetition_penalty, frequency_penalty, presence_penalty, n_req)
        shaping = check_shaping(top_k, min_p, logit_bias, n_req)
        ban = check_ban(no_repeat_ngram_size, bad_words, min_tokens, n_req, max_new_tokens, json_mode=json_mode,
                        json_schema=json_schema)
        check_stop(stop)
        ns = check_n_list(n, n_req, self.max_batch)
        switches = dict(logprobs=logprobs, json_mode=json_mode, json_schema=json_schema, top_p=top_p, stop=stop,
                        on_stream=on_stream, **ban_kwargs(ban))
        if n_req == 1 and ns is not None and ns[0] == 1:      # one choice: the route without n, the results nested
            out = self._generate_batch(requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                                       seeds=seeds, repetition_penalty=repetition_penalty, frequency_penalty=frequency_penalty,
                                       presence_penalty=presence_penalty, top_k=top_k, min_p=min_p, logit_bias=logit_bias,
                                       **switches)
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
                self.last_logprobs = [None] if logprobs is not None else None
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
                                       seed if seeds is None else seeds[0], **switches, **shaping_kwargs(shaping),
                                       **({} if penalties is None else dict(zip(_PENALTY_NAMES, penalties[0]))))]
            except Exception as e:      # noqa: BLE001
                if own:
                    return failed(e)
                if isinstance(e, JsonModeError):
                    return [e]
                raise
        self._check_batch(requests)
        with self._pick_request(logprobs, json_mode, json_schema, top_p, seeds is not None, penalties, stop=stop,
                                shaping=shaping, on_stream=on_stream, **({} if ban is None else {"ban": ban})):
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
        slots, errors = self.prefill_many(requests, temperature=temperature, seed=seed, max_new_tokens=max_new_tokens,
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

        done = 1
        g = self._batch_graph(B) if use_graph else None
        while done < max_new_tokens and not self._stream_cancelled():
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
        outs = collect(done)
        # host waiting for the lazy requests' decodes is inside prefill_ms here: it is the time until all prompts are in
        self.last_timing = {"prompt_tokens": longest, "prefill_ms": ev[0].elapsed_time(ev[1]),
                            "decode_ms": ev[1].elapsed_time(ev[2]), "decode_steps": done - 1, "sequences": B}
        return self._gather_choices(choice_slots, errors, outs, starts, eos, ignore_eos, self.keep_eos, ns is not None,
                                    self._mask_error)
