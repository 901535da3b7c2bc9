"""What a request may switch on at an engine, as one record: the engines' public ``generate`` / ``generate_batch`` turn their
``**switches`` into it and ``Generation._generate`` / ``_generate_batch`` take it as one argument."""
from __future__ import annotations

from dataclasses import dataclass, fields, replace
from typing import Any, Optional, Sequence

import numpy as np

from . import spec
from .ban import ban_kwargs, check_ban
from .penalties import check_penalties
from .shaping import check_shaping, shaping_kwargs

PENALTY_NAMES = ("repetition_penalty", "frequency_penalty", "presence_penalty")      # the order of check_penalties' triples
_PER_REQUEST = PENALTY_NAMES + ("top_k", "min_p", "logit_bias", "no_repeat_ngram_size", "bad_words", "min_tokens")


def _refuse(where: str, given: dict, *names: str) -> None:
    for name in names:
        if name in given:
            raise TypeError(f"{where}() got an unexpected keyword argument {name!r}")


@dataclass(frozen=True)
class Switches:
    """The switches of one engine call, in the engines' spelling; every default is "off": exactly the launches of a call
    without the keyword.  The fields stand in the order in which a speculative request names its conflicts (``exclusive``).
    In a batch the penalties, ``top_k``, ``min_p``, ``logit_bias``, ``no_repeat_ngram_size`` and ``min_tokens`` are each one
    value for the group or a sequence with one value (or None) per request, whose choices (``n``) inherit it; every other
    switch is one value for the group.  Logprobs keep their meaning under every switch: they are of the raw logits.
    ``logprobs`` = k in 0..20: afterwards ``last_logprobs`` holds one TokenLogprobs record per request (None for a failed
    one): the log-softmax of the raw logits - independent of temperature and seed - for every returned token, plus its k most
    likely alternatives; None = off, no extra launch.
    ``json_mode``: every pick is restricted to the tokens that continue a JSON object (json_grammar; needs
    ``self.tokenizer``): the reply is a prefix of one, complete when it ended on EOS; JsonModeError when the vocabulary could
    not continue it (in a batch: that request's entry).  top_logprobs may list tokens the mask forbade.
    ``top_p`` in [0, 1]: nucleus sampling (sampling.py) - each pick draws from the shortest most-likely prefix holding top_p
    of the temperature-scaled mass; None or 1 = off.
    ``repetition_penalty`` > 0 (transformers' meaning: over prompt and generated ids), ``frequency_penalty`` /
    ``presence_penalty`` in [-2, 2] (OpenAI's: over generated ids): penalties.py - applied to the raw logits ahead of
    everything above; None or 1 / 0 / 0 = off.
    ``json_schema`` (a json_schema.SchemaDFA): as ``json_mode``, with the schema's compiled DFA as the grammar
    (vis_schema_mask): a reply that ended on EOS is a document of the schema.  Not together with ``json_mode``.
    ``stop``: a string or 1..4 of them (stop.py): the reply ends with the token that completes the first occurrence of one in
    its bytes (vis_stop_scan after every pick; the poll then reads its records, not the token row), also in an ``ignore_eos``
    run; the shared loop of a batch ends when every row has ended.  Afterwards, always, ``last_finish`` = [(reason, cut)],
    one per request (None for a failed one): "eos", "stop" (cut = the byte offset in the returned tokens' bytes where the
    stop string starts) or "length" (max_new_tokens, the context clamp, or an ``ignore_eos`` run that matched nothing).
    ``top_k`` >= 1, ``min_p`` in [0, 1] (transformers' TopKLogitsWarper / MinPLogitsWarper) and ``logit_bias`` {token id:
    bias in [-100, 100]}, at most 300 entries (OpenAI's): shaping.py - one launch ahead of the pick adds the biases to the
    (penalised) logits, then takes out every token below the k-th largest allowed one or less likely than min_p times the
    most likely one; top_p and the draw see the rest.  None / 0 / {} = off; a greedy request is affected by logit_bias only.
    ``on_stream`` (a stream.StreamReader the caller polls from another thread; its events name the request and the choice):
    every token is published to it while the loop runs - vis_stream_publish after every pick, behind the stop scan, which is
    then on with or without ``stop`` - and the loop keeps its launch-ahead.  ``on_stream.cancel()`` ends the loop at its next
    ``check_every`` boundary (the reply then ended as "length").  Not together with ``logprobs``.  A request served again
    after a stalled chained launch resets the reader's slot; the reader continues behind what it had handed out (stream.py).
    ``no_repeat_ngram_size`` in 1..64 (transformers' NoRepeatNGramLogitsProcessor: no n-gram of prompt + reply occurs twice),
    ``bad_words``, up to 16 strings of 1..8 token ids each (transformers' NoBadWordsLogitsProcessor / vLLM's: the token that
    would complete one is never picked; a word the tokenizer spells differently behind a space is banned in both spellings)
    and ``min_tokens`` <= max_new_tokens (vLLM's: no EOS id before that many tokens): ban.py - one launch after the penalties
    takes the banned ids out of the pick.  None / 0 / [] = off.  Not together with ``json_mode`` / ``json_schema``
    (ValueError: a ban could leave the grammar no token).  ``min_tokens`` holds back EOS ids only: a ``stop`` string may
    still end the reply earlier.
    ``seeds`` (generate_batch only): one integer per request, its own sampling seed in place of the slot-derived one, so a
    request's sampled reply does not depend on its slot or on what shares the batch.
    ``n`` (generate_batch only): None, an integer >= 1 or one integer per request - that many sampled choices of each request
    from ONE prompt pass (fork.py): the further choices take slots behind the requests', read the prompt's keys / values from
    the slot that ran the prompt pass (vis_decode_attn_forked) and sample with seeds[j] + i (without seeds: the slot-derived
    seed of the slot they land in).  All choices together must fit max_batch.  With ``n`` given, the entry of a request is a
    list of n[j] token lists (for a failed request the exception object, as without), and ``last_logprobs`` /
    ``last_finish`` nest the same way.  At temperature 0 all choices of a request are equal; they are decoded all the same.
    A slot is still a full-size cache: ``n`` saves prompt passes and attention traffic, not cache memory.
    ``speculative`` (generate only): None (off), the integer k in 1..3 or {"method": "ngram", "num_speculative_tokens": k,
    "prompt_lookup_max": 4, "prompt_lookup_min": 2} (spec.py): a decode step carries the current token and up to k ids
    drafted by prompt lookup over prompt + reply through ONE pass over the weights and keeps the drafts the model's own greedy
    picks confirm - the reply is the plain reply token for token, in fewer weight passes where the reply repeats earlier
    text.  Greedy single requests of the Qwen2-VL engines, or of an MllamaEngine built with speculative=True, only:
    ValueError with any switch above (one token at a time; "grammar": True lets ``json_schema`` through, spec.py) or, unless the dict says "sampled": True (the plain sampled reply),
    with a temperature or a seed.  Afterwards ``last_timing`` holds ``spec_steps`` / ``spec_proposed`` / ``spec_accepted``.
    ``prediction`` (generate only; generate_batch refuses one other than None): a sequence of token ids the reply will
    probably repeat (OpenAI's Predicted Outputs; at most max_ctx are kept, none = off): the drafts come from it while the
    reply follows it, and from prompt lookup where it does not (spec.propose_pred, vis_spec_draft_pred).  Alone it implies
    speculative = k 3, window 4..2; ``speculative`` next to it sets k and the window.  The same conditions and refusals as
    ``speculative``; the reply is the plain reply.  Afterwards ``last_timing`` also holds ``pred_accepted`` /
    ``pred_rejected``: the prediction's drafts the steps kept and did not keep, over every step issued."""
    logprobs: Optional[int] = None
    json_mode: bool = False
    top_p: Optional[float] = None
    repetition_penalty: Any = None
    frequency_penalty: Any = None
    presence_penalty: Any = None
    json_schema: Any = None
    stop: Any = None
    top_k: Any = None
    min_p: Any = None
    logit_bias: Any = None
    on_stream: Any = None
    no_repeat_ngram_size: Any = None
    bad_words: Optional[Sequence[str]] = None
    min_tokens: Any = None
    seeds: Optional[Sequence[int]] = None
    n: Any = None
    speculative: Any = None
    prediction: Optional[Sequence[int]] = None

    @classmethod
    def single(cls, **switches) -> "Switches":
        """The keywords of ``generate``; TypeError for one that is no switch, ``seeds`` and ``n`` among them."""
        _refuse("generate", switches, "seeds", "n")
        return cls(**switches)

    @classmethod
    def group(cls, **switches) -> "Switches":
        """The keywords of ``generate_batch``; TypeError for one that is no switch, ``speculative`` among them, ValueError for
        a ``prediction``: the speculative step carries one sequence."""
        _refuse("generate_batch", switches, "speculative")
        spec.refuse_batch_prediction(switches.get("prediction"))
        return cls(**switches)

    def exclusive(self) -> dict:
        """What spec.check_exclusive has to look at: the fields a speculative request may not carry that are not at their
        default, under their names, in the fields' order (the first conflict is the one its message names)."""
        return {f.name: getattr(self, f.name) for f in fields(self)
                if f.name not in ("speculative", "prediction") and getattr(self, f.name) is not f.default}

    def request(self, b: int) -> "Switches":
        """Request ``b`` of a group alone, for the single-sequence route: of a field with one value per request its b-th, in
        the form the checks give it (a ``logit_bias`` dict rebuilt from the checked list, ``bad_words`` a list or None; a
        family of switches that is off is None throughout); no ``seeds``, no ``n``."""
        def own(v):
            return v[b] if isinstance(v, (Sequence, np.ndarray)) and not isinstance(v, (str, bytes)) else v
        penalties = check_penalties(*(own(getattr(self, name)) for name in PENALTY_NAMES), 1)
        shaping = check_shaping(own(self.top_k), own(self.min_p), own(self.logit_bias), 1)
        ban = check_ban(own(self.no_repeat_ngram_size), self.bad_words, own(self.min_tokens), 1)
        values = {**dict.fromkeys(_PER_REQUEST), **dict(zip(PENALTY_NAMES, penalties[0]) if penalties else ()),
                  **shaping_kwargs(shaping), **ban_kwargs(ban)}
        return replace(self, seeds=None, n=None, **values)
