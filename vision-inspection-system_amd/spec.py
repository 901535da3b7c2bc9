"""Lossless n-gram speculative decoding of one greedy request: the request's switch and what it excludes, the prompt-lookup
drafter as a numpy reference (``propose``; vis_spec_draft equals it exactly), a numpy restatement of the accept step
(``accept_ref``; vis_spec_accept), and the device buffers of the speculative step (DecodeStage._decode_step_spec).

A step feeds R = 1 + k rows - the current token and up to k drafted ones - through every projection in ONE pass over the
weights (vis_gemv_*_rows: each row's arithmetic is the single-row kernel's, bit for bit) and through
vis_decode_attn_draft (row r bit-identical to a plain attention launch at its position).  Row r's logits therefore are
the logits the plain step would have computed after the drafts in front of it - when those drafts are what the plain
step would have picked.  The accept step keeps exactly that prefix, so the reply is the plain reply token for token.

A request may bring a second source of drafts, the caller's prediction of the reply (OpenAI's Predicted Outputs:
``check_prediction``): ``propose_pred`` is that drafter's definition (vis_spec_draft_pred equals it exactly), and
``simulate_prediction`` the model-free walk that gives the counters a run must report.

A request that opts in (``"sampled": True``) may sample: the engines' pick at a temperature is Gumbel-max over a counter hash
of (seed, step, id), so the token is a pure function of (logits row, seed, step), and row r of a step carries the logits of
step + r.  vis_spec_accept_sampled takes every row's pick with that counter (``accept_ref_sampled`` walks given picks); the
reply is then the plain SAMPLED reply token for token - equality, not rejection sampling's equality in distribution.

A request that opts in (``"grammar": True``) may carry a JSON Schema: the DFA state in front of row r is the state in front of
row r - 1 walked through draft r - 1, so vis_schema_mask_rows writes every row's mask, vis_spec_accept_masked takes the masked
picks, and a draft the schema rejects is never the masked pick - the reply is the plain schema-constrained reply.  The schema
then drafts too (``schema_drafts``, schema_draft.py): the bytes it forces are known before the model is asked."""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

MAX_K = 3            # R = k + 1 <= 4 rows: the bound of the multi-row GEMVs (hip.SPEC_MAX_ROWS)
MAX_LOOKUP = 8       # hip.SPEC_MAX_LOOKUP
ROWS_LDS_MAX = 152 * 1024      # GV_ROWS_LDS_MAX of csrc/decode.hip: the input rows of a multi-row GEMV live in LDS


class SpecConfig(tuple):
    """(k, lookup_max, lookup_min[, True][, "grammar"[, "no_schema_drafts"]]): num_speculative_tokens, prompt_lookup_max,
    prompt_lookup_min and the request's own opt-ins.  ``sampled``: the accept step takes the sampled pick
    (vis_spec_accept_sampled).  ``grammar``: the request carries a JSON Schema, and the step masks every row's pick with the
    schema's DFA state in front of that row (vis_schema_mask_rows, vis_spec_accept_masked); ``schema_drafts`` (on with
    ``grammar`` unless switched off): the schema's forced bytes are drafts too (schema_draft.py, vis_spec_draft_schema).  A
    value stands in the tuple only when it is set, so the record of a request that did not opt in is, value for value, the
    three-field record of before (what the engines are handed and what a recorded call compares against); SpecConfig(2, 4, 2)
    == SpecConfig(2, 4, 2, False) == SpecConfig(2, 4, 2, False, False)."""
    __slots__ = ()

    def __new__(cls, k: int, lookup_max: int, lookup_min: int, sampled: bool = False, grammar: bool = False,
                schema_drafts: Optional[bool] = None):
        extra = ((True,) if sampled else ()) + (("grammar",) if grammar else ())
        if grammar and schema_drafts is False:
            extra += ("no_schema_drafts",)
        return tuple.__new__(cls, (k, lookup_max, lookup_min) + extra)

    k = property(lambda self: self[0])
    lookup_max = property(lambda self: self[1])
    lookup_min = property(lambda self: self[2])
    sampled = property(lambda self: len(self) > 3 and self[3] is True)
    grammar = property(lambda self: "grammar" in self[3:])
    schema_drafts = property(lambda self: "grammar" in self[3:] and "no_schema_drafts" not in self[3:])

    @property
    def rows(self) -> int:
        return self.k + 1

    def __repr__(self) -> str:
        more = f", grammar=True, schema_drafts={self.schema_drafts}" if self.grammar else ""
        return f"SpecConfig(k={self.k}, lookup_max={self.lookup_max}, lookup_min={self.lookup_min}, sampled={self.sampled}{more})"


def _int(v, name: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"speculative: {name} must be an integer in {lo}..{hi}")
    return v


def check_speculative(speculative) -> Optional[SpecConfig]:
    """None (off), the integer k, or {"method": "ngram", "num_speculative_tokens": k[, "prompt_lookup_max": 4,
    "prompt_lookup_min": 2][, "sampled": False][, "grammar": False[, "schema_drafts": True]]} (vLLM's names; ``sampled``,
    ``grammar`` and ``schema_drafts`` are this package's: the request may carry a temperature and a seed / a JSON Schema, see
    check_exclusive) -> SpecConfig or None; ValueError otherwise."""
    if speculative is None:
        return None
    if isinstance(speculative, SpecConfig):
        speculative = {"method": "ngram", "num_speculative_tokens": speculative.k, "prompt_lookup_max": speculative.lookup_max,
                       "prompt_lookup_min": speculative.lookup_min, "sampled": speculative.sampled,
                       **({"grammar": True, "schema_drafts": speculative.schema_drafts} if speculative.grammar else {})}
    if isinstance(speculative, int) and not isinstance(speculative, bool):
        speculative = {"method": "ngram", "num_speculative_tokens": speculative}
    if not isinstance(speculative, dict):
        raise ValueError("speculative must be None, an integer k or a dict with 'method' and 'num_speculative_tokens'")
    unknown = set(speculative) - {"method", "num_speculative_tokens", "prompt_lookup_max", "prompt_lookup_min", "sampled",
                                  "grammar", "schema_drafts"}
    if unknown:
        raise ValueError(f"speculative: unknown keys {sorted(unknown)}")
    if speculative.get("method", "ngram") != "ngram":
        raise ValueError("speculative: the only method is 'ngram' (prompt lookup; there is no draft model)")
    if "num_speculative_tokens" not in speculative:
        raise ValueError("speculative: num_speculative_tokens is required")
    k = _int(speculative["num_speculative_tokens"], "num_speculative_tokens", 1, MAX_K)
    hi = _int(speculative.get("prompt_lookup_max", 4), "prompt_lookup_max", 1, MAX_LOOKUP)
    lo = _int(speculative.get("prompt_lookup_min", min(2, hi)), "prompt_lookup_min", 1, hi)
    sampled = speculative.get("sampled", False)
    if not isinstance(sampled, bool):
        raise ValueError("speculative: sampled must be True or False")
    grammar, drafts = speculative.get("grammar", False), speculative.get("schema_drafts")
    if not isinstance(grammar, bool):
        raise ValueError("speculative: grammar must be True or False")
    if drafts is not None and not isinstance(drafts, bool):
        raise ValueError("speculative: schema_drafts must be True or False")
    if drafts and not grammar:
        raise ValueError("speculative: schema_drafts needs 'grammar': True (the schema's drafts are checked by the schema's mask)")
    return SpecConfig(k, hi, lo, sampled, grammar, drafts)


PRED_DEFAULT = SpecConfig(3, 4, 2)      # what ``prediction`` alone implies: four rows per step, vLLM's lookup window


def check_prediction(prediction) -> Optional[str]:
    """OpenAI's Predicted Outputs argument -> its text: {"type": "content", "content": str}, or content as a list of
    {"type": "text", "text": str} parts (concatenated).  None, or a prediction without text: None (no prediction).
    ValueError for any other type, a missing content or a part that is not text."""
    if prediction is None:
        return None
    if not isinstance(prediction, dict):
        raise ValueError("prediction must be a dict {'type': 'content', 'content': ...}")
    unknown = set(prediction) - {"type", "content"}
    if unknown:
        raise ValueError(f"prediction: unknown keys {sorted(unknown)}")
    if prediction.get("type") != "content":
        raise ValueError("prediction: the only type is 'content'")
    if "content" not in prediction:
        raise ValueError("prediction: content is required")
    content = prediction["content"]
    if isinstance(content, (list, tuple)):
        for part in content:
            if not isinstance(part, dict) or set(part) != {"type", "text"} or part["type"] != "text" \
                    or not isinstance(part["text"], str):
                raise ValueError("prediction: every content part must be {'type': 'text', 'text': str}")
        content = "".join(part["text"] for part in content)
    if not isinstance(content, str):
        raise ValueError("prediction: content must be a string or a list of text parts")
    return content or None


def check_prediction_ids(prediction, max_ids: Optional[int] = None) -> Optional[List[int]]:
    """The engine-level form: a sequence of token ids (>= 0), at most ``max_ids`` kept.  None or empty: None."""
    if prediction is None:
        return None
    if isinstance(prediction, (str, bytes, dict)) or not hasattr(prediction, "__len__"):
        raise ValueError("prediction must be a sequence of token ids")
    ids = []
    for t in (prediction if max_ids is None else prediction[:max_ids]):
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < 2 ** 31:
            raise ValueError("prediction must be a sequence of token ids (integers >= 0)")
        ids.append(int(t))
    return ids or None


def refuse_batch_prediction(prediction) -> None:
    """generate_batch / complete_many: a prediction belongs to ONE greedy request (the speculative step carries one sequence)."""
    if prediction is not None:
        raise ValueError("prediction (speculative decoding) serves one request per call: chat.completions.create / generate, "
                         "not a batch")


def with_prediction(speculative, has_prediction: bool) -> Optional[SpecConfig]:
    """The step configuration of a request: ``speculative`` as check_speculative reads it; a prediction alone implies
    PRED_DEFAULT (k = 3: with a prediction that holds, the four-row step is the cheapest per token in every weight format).
    ``schema_drafts`` next to a prediction is a ValueError: the prediction drafter counts what the accept step kept of the
    draft row as its own, so it has to be the row's only writer ("schema_drafts": False keeps the schema's mask)."""
    sp = check_speculative(speculative)
    if sp is not None and sp.schema_drafts and has_prediction:
        raise ValueError("prediction together with the schema's drafts is not supported: the prediction drafter's accepted / "
                         "rejected counts assume it owns the draft row; pass 'schema_drafts': False in speculative")
    return PRED_DEFAULT if sp is None and has_prediction else sp


def check_exclusive(cfg: Optional[SpecConfig], temperature: float = 0.0, seed=None, *, what: str = "speculative",
                    **switches) -> None:
    """What a speculative request may not carry: every switch that is a per-step device state machine advancing one token
    at a time, and everything that samples.  ``switches``: name -> value as the caller got it (None / neutral = off).
    ValueError naming the conflict.  ``what``: how the messages name the request's argument.
    A request that opted in (``cfg.sampled``) may carry ``temperature`` and ``seed``: its pick is Gumbel-max over a counter
    hash, a pure function of (logits row, seed, step), so "the draft equals the pick of the row in front of it" stays exact
    with the sampled pick at hash counter step + r (vis_spec_accept_sampled).  ``top_p`` and everything else stay refused.
    A request that opted in with ``cfg.grammar`` must carry a JSON Schema (``json_schema``, or a ``response_format`` of type
    json_schema) and may: the DFA state in front of row r is the state in front of row r - 1 walked through draft r - 1, so
    every row's mask is the plain step's (vis_schema_mask_rows), and a draft the schema rejects is never the masked pick."""
    if cfg is None:
        return
    if cfg.grammar:
        rf = switches.get("response_format")
        by_format = isinstance(rf, dict) and rf.get("type") == "json_schema"
        if switches.get("json_schema") is None and not by_format:
            raise ValueError(f"{what}: 'grammar' needs a JSON Schema on the request (json_schema / response_format of type "
                             "json_schema)")
        switches = {name: v for name, v in switches.items()
                    if name != "json_schema" and not (name == "response_format" and by_format)}
    if cfg.sampled:
        temperature = seed = None
    if temperature:
        raise ValueError(f"{what} together with temperature > 0 is not supported: acceptance is defined for the greedy pick")
    if seed:
        raise ValueError(f"{what} together with a seed is not supported: a greedy request has nothing to seed")
    neutral = {"top_p": (None, 1, 1.0), "repetition_penalty": (None, 1, 1.0), "frequency_penalty": (None, 0, 0.0),
               "presence_penalty": (None, 0, 0.0), "top_k": (None, 0), "min_p": (None, 0, 0.0), "logit_bias": (None, {}),
               "no_repeat_ngram_size": (None, 0), "bad_words": (None, [], ()), "min_tokens": (None, 0),
               "json_mode": (None, False), "json_schema": (None,), "response_format": (None, {"type": "text"}), "stop": (None, [], ()),
               "stream": (None, False), "on_stream": (None,), "logprobs": (None, False), "top_logprobs": (None,),
               "n": (None, 1), "seeds": (None,)}
    for name, value in switches.items():
        off = neutral.get(name, (None,))
        if not any(value is o or (type(value) is type(o) and value == o) for o in off):
            raise ValueError(f"{what} together with {name} is not supported: it is a per-step state of the pick, and a "
                             "speculative step yields several tokens")


def sampled_seed(cfg: SpecConfig, seed, default: int, response_format=None):
    """The client's checked keywords of ONE speculative request (client.engine_keywords' pair: the engine keywords that are
    on, the call's seed).  No other keyword is on; a request that opted in hands ``generate`` the seed the plain single
    request draws with - its own ``seed`` where it brought one, else the client's ``default``.  A request that did not is
    the call of before: nothing on.  A ``grammar`` configuration also hands on the compiled schema of the request's
    ``response_format`` (check_exclusive has seen that it is one)."""
    from .sampling import check_seed
    on = {}
    if cfg.grammar:
        from .client import schema_of
        on["json_schema"] = schema_of(response_format)
    if not cfg.sampled:
        return on, None
    seed = check_seed(seed)
    return {**on, "seed": default if seed is None else seed}, None


def sampled_from_env() -> bool:
    """VIS_SPECULATIVE_SAMPLED (unset, empty or 0 = off; 1 = on; anything else: ValueError): the configurations from_env and
    auditor_from_env return carry ``sampled``, so the agents' requests keep speculating at their temperature and seed."""
    v = os.environ.get("VIS_SPECULATIVE_SAMPLED", "").strip()
    if v not in ("", "0", "1"):
        raise ValueError("VIS_SPECULATIVE_SAMPLED must be 0 or 1")
    return v == "1"


def grammar_from_env() -> bool:
    """VIS_SPECULATIVE_GRAMMAR (unset, empty or 0 = off; 1 = on; anything else: ValueError): the configurations from_env and
    auditor_from_env return carry ``grammar``, so the agents' requests that send the report's schema (VIS_JSON_SCHEMA=1) keep
    speculating.  Alone it turns nothing on."""
    v = os.environ.get("VIS_SPECULATIVE_GRAMMAR", "").strip()
    if v not in ("", "0", "1"):
        raise ValueError("VIS_SPECULATIVE_GRAMMAR must be 0 or 1")
    return v == "1"


def from_env() -> Optional[SpecConfig]:
    """VIS_SPECULATIVE=k (1..3; unset, empty or 0 = off): the agents pass it on requests without an excluded switch.
    VIS_SPECULATIVE_SAMPLED=1 / VIS_SPECULATIVE_GRAMMAR=1 next to it set ``sampled`` / ``grammar`` on the configuration."""
    sampled, grammar = sampled_from_env(), grammar_from_env()
    v = os.environ.get("VIS_SPECULATIVE", "").strip()
    if v in ("", "0"):
        return None
    try:
        k = int(v)
    except ValueError:
        raise ValueError("VIS_SPECULATIVE must be an integer in 0..3") from None
    return check_speculative({"num_speculative_tokens": k, "sampled": sampled, "grammar": grammar})


def check_rows_fit(cfg_model, rows: int) -> None:
    """The multi-row GEMVs keep their input rows in LDS: the widest projection input of the model must fit."""
    width = max(cfg_model.intermediate, cfg_model.hidden)
    if width * 2 * (1 if rows == 1 else 2 if rows == 2 else 4) > ROWS_LDS_MAX:
        raise ValueError(f"speculative: {rows} rows of {width} inputs do not fit the multi-row GEMV's LDS")


def check_cross_rows_fit(cfg_model, rows: int) -> None:
    """The draft cross-attention kernels place every row's G = heads / kv_heads query heads of a kv group in the 16 columns of
    one score MFMA (vis_decode_cross_attn_draft): rows * G <= 16."""
    g = cfg_model.heads // cfg_model.kv_heads
    if rows * g > 16:
        raise ValueError(f"speculative: {rows} rows of {g} query heads per kv head do not fit the draft cross-attention "
                         f"(rows * heads per kv head <= 16: at most k = {16 // g - 1})")


def auditor_from_env() -> Optional[SpecConfig]:
    """VIS_AUDITOR_SPECULATIVE=k (1..3; unset, empty or 0 = off; anything else: ValueError): the Auditor's (Mllama) engine is
    built with speculative=True, the clients accept ``speculative`` / ``prediction`` for one request of an mllama model, and
    the agents pass k on a single request to one.  VIS_SPECULATIVE is the Qwen2-VL engines' and is not read here;
    VIS_SPECULATIVE_SAMPLED=1 / VIS_SPECULATIVE_GRAMMAR=1 set ``sampled`` / ``grammar`` on the configuration as in from_env."""
    sampled, grammar = sampled_from_env(), grammar_from_env()
    v = os.environ.get("VIS_AUDITOR_SPECULATIVE", "").strip()
    if v in ("", "0"):
        return None
    try:
        k = int(v)
    except ValueError:
        k = -1
    if not 1 <= k <= MAX_K:
        raise ValueError(f"VIS_AUDITOR_SPECULATIVE must be an integer in 0..{MAX_K}")
    return check_speculative({"num_speculative_tokens": k, "sampled": sampled, "grammar": grammar})


# ----------------------------------------------------------------------------------------------------- references
def propose(history: Sequence[int], k: int, lookup_max: int = 4, lookup_min: int = 2) -> List[int]:
    """Prompt lookup: for m from lookup_max down to lookup_min, the LATEST earlier occurrence of the last m ids of
    ``history`` that has at least one id behind it; the first m that has one gives the up to k ids that followed it.
    No match: []."""
    h = list(history)
    L = len(h)
    for m in range(lookup_max, lookup_min - 1, -1):
        if L <= m:
            continue
        tail = h[L - m:]
        for j in range(L - m - 1, -1, -1):
            if h[j:j + m] == tail:
                return h[j + m:j + m + k]
    return []


class PredState(NamedTuple):
    """What the prediction drafter keeps between two calls (the 7 device ints of vis_spec_draft_pred, in this order)."""
    cursor: int = 0      # index into pred of the id expected next; -1 = lost
    last: int = 0        # the last cursor value held before a loss
    seen: int = 0        # reply tokens consumed so far
    src: int = 0         # source of the drafts outstanding from the previous call: 0 none, 1 prompt lookup, 2 prediction
    n_out: int = 0       # their count
    accepted: int = 0    # prediction-sourced drafts the accept step kept
    rejected: int = 0    # ... and did not keep


def propose_pred(state: PredState, prompt: Sequence[int], reply: Sequence[int], pred: Sequence[int], k: int,
                 lookup_max: int = 4, lookup_min: int = 2, vocab: Optional[int] = None):
    """The drafter of a request with a prediction; vis_spec_draft_pred equals it exactly.  ``reply``: everything picked so
    far, the newest pick included.  Returns (draft, state).

    1. new = reply[seen:]; a = min(len(new) - 1, n_out) is what the accept step kept of the outstanding drafts (a step
       yields the kept drafts and one more token).  Drafts that came from the prediction count: accepted += a, rejected +=
       n_out - a - also those the request's token limit cut off.  No new token (a step issued behind the limit): no count.
    2. Every new token moves the cursor on when it is the id the prediction expected; the first one that is not loses the
       cursor (last = where it stood), and it stays lost for the rest of ``new``.
    3. A lost cursor is looked for again: for m = lookup_max down to lookup_min (the reply holds m ids), the candidates are
       e in [m, P) with pred[e-m:e] == reply[-m:].  The smallest candidate >= last wins - the reply went on in the
       prediction behind a substituted, skipped or inserted piece; without one the largest candidate < last - a report
       whose list entries repeat the template's keys.  The first m with a candidate decides.
    4. With the cursor inside the prediction the draft is pred[cursor:cursor + k] (src 2); else it is the prompt lookup
       ``propose(prompt + reply, ..)`` (src 1, or 0 when that has nothing).  Ids are clamped into [0, vocab)."""
    reply, pred = [int(t) for t in reply], [int(t) for t in pred]
    P = len(pred)
    cursor, last, seen, src, n_out, accepted, rejected = state
    new = reply[seen:]
    if new and src == 2:
        a = min(len(new) - 1, n_out)
        accepted, rejected = accepted + a, rejected + n_out - a
    for t in new:
        if 0 <= cursor < P and pred[cursor] == t:
            cursor += 1
        elif cursor >= 0:
            last, cursor = cursor, -1
    if cursor == -1 and P > 0:
        for m in range(lookup_max, lookup_min - 1, -1):
            if len(reply) < m:
                continue
            cand = [e for e in range(m, P) if pred[e - m:e] == reply[-m:]]
            if cand:
                fwd = [e for e in cand if e >= last]
                cursor = fwd[0] if fwd else cand[-1]
                break
    if 0 <= cursor < P:
        draft, src = pred[cursor:cursor + min(k, P - cursor)], 2
    else:
        draft = propose(list(prompt) + reply, k, lookup_max, lookup_min)
        src = 1 if draft else 0
    if vocab is not None:
        draft = [min(max(t, 0), vocab - 1) for t in draft]
    return draft, PredState(cursor, last, len(reply), src, len(draft), accepted, rejected)


def simulate_prediction(plain_reply: Sequence[int], prompt: Sequence[int], pred: Sequence[int], k: int, lookup_max: int = 4,
                        lookup_min: int = 2, max_new_tokens: Optional[int] = None, vocab: Optional[int] = None) -> dict:
    """What a run with ``prediction=pred`` must report, without a model: the scheme is lossless, so the pick behind any
    accepted prefix is the plain reply's next token.  ``plain_reply``: the reply of the plain request run to its length
    limit (ignore_eos), at least max_new_tokens ids.  Walks the steps as vis_spec_accept takes them (a draft counts while it
    equals the pick in front of it; the limit cuts the last step's run) and returns the reply and the five counters:
    {"reply", "spec_steps", "spec_proposed", "spec_accepted", "pred_accepted", "pred_rejected"}."""
    plain = [int(t) for t in plain_reply]
    N = len(plain) if max_new_tokens is None else min(len(plain), max_new_tokens)
    reply = plain[:1]
    draft, state = propose_pred(PredState(), prompt, reply, pred, k, lookup_max, lookup_min, vocab)
    steps = proposed = accepted = 0
    while len(reply) < N:
        n, d, a = len(reply), len(draft), 0
        while a < d and n + a < N - 1 and draft[a] == plain[n + a]:
            a += 1
        reply = plain[:n + a + 1]
        steps, proposed, accepted = steps + 1, proposed + d, accepted + a
        draft, state = propose_pred(state, prompt, reply, pred, k, lookup_max, lookup_min, vocab)
    return {"reply": reply, "spec_steps": steps, "spec_proposed": proposed, "spec_accepted": accepted,
            "pred_accepted": state.accepted, "pred_rejected": state.rejected}


def accept_ref(logits: np.ndarray, draft: Sequence[int], d: int, step: int, limit: int, tokens: np.ndarray,
               counters: Sequence[int]):
    """vis_spec_accept restated: returns (tokens, cur_token or None, step, counters) after the call."""
    tokens, counters = np.array(tokens), list(counters)
    R = logits.shape[0]
    if step < 0 or step > min(limit, len(tokens) - 1):
        return tokens, None, step, counters
    # np.argmax ignores nothing: restate the comparison (first maximum among the comparable values)
    picks = []
    for r in range(R):
        row = np.asarray(logits[r], dtype=np.float32)
        ok = ~np.isnan(row)
        picks.append(int(np.flatnonzero(ok & (row == row[ok].max()))[0]) if ok.any() else 0)
    d = min(max(d, 0), R - 1)
    a = 0
    while a < d and draft[a] == picks[a]:
        a += 1
    a = min(a, min(limit, len(tokens) - 1) - step)
    tokens[step:step + a + 1] = picks[:a + 1]
    return tokens, picks[a], step + a + 1, [counters[0] + 1, counters[1] + d, counters[2] + a]


def accept_ref_sampled(picks: Sequence[int], draft: Sequence[int], d: int, step: int, limit: int, tokens: np.ndarray,
                       counters: Sequence[int]):
    """The model-free half of accept_ref, which vis_spec_accept and vis_spec_accept_sampled share: the walk over GIVEN per-row
    picks (row r's pick, however it was made - the sampled one at hash counter step + r).  Returns (tokens, cur_token or
    None, step, counters) after the call."""
    tokens, counters, picks = np.array(tokens), list(counters), [int(p) for p in picks]
    R = len(picks)
    lim = min(limit, len(tokens) - 1)
    if step < 0 or step > lim:
        return tokens, None, step, counters
    d = min(max(d, 0), R - 1)
    a = 0
    while a < d and draft[a] == picks[a]:
        a += 1
    a = min(a, lim - step)
    tokens[step:step + a + 1] = picks[:a + 1]
    return tokens, picks[a], step + a + 1, [counters[0] + 1, counters[1] + d, counters[2] + a]


# --------------------------------------------------------------------------------------------------- device buffers
class SpecBuffers:
    """What the speculative step of one engine owns: its own activation rows (an engine built with max_batch=1 has no
    batched buffers), the attention workspace for 4 rows (``n_split``: the largest split count of the launches that share
    it - a model with cross-attention layers: max(nsplit, xsplit)), the f32 logits of 4 rows, the id row [cur, drafts], the request's
    prompt ids and the small device ints the launches read (draft count, limit, prompt length, start of the reply in the
    token row, counters), and for a request with a prediction its ids (max_ctx int32), their count and the drafter's state."""

    def __init__(self, cfg, n_split: int, max_ctx: int, device):
        bf, dev, R = torch.bfloat16, device, MAX_K + 1
        nq = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        self.x = torch.empty((R, cfg.hidden), dtype=bf, device=dev)
        self.x2 = torch.empty((R, cfg.hidden), dtype=bf, device=dev)
        self.qkv = torch.empty((R, nq), dtype=bf, device=dev)
        self.attn = torch.zeros((R, cfg.heads * cfg.head_dim), dtype=bf, device=dev)     # a row past the cache is never written
        self.act = torch.empty((R, cfg.intermediate), dtype=bf, device=dev)
        self.logits = torch.empty((R, cfg.vocab), dtype=torch.float32, device=dev)
        self.part_o = torch.empty(R * cfg.heads * n_split * cfg.head_dim, dtype=torch.float32, device=dev)
        self.part_ml = torch.empty(R * cfg.heads * n_split * 2, dtype=torch.float32, device=dev)
        self.ws_val = torch.empty(256 * R, dtype=torch.float32, device=dev)
        self.ws_idx = torch.empty(256 * R, dtype=torch.int32, device=dev)
        self.ids = torch.zeros(R, dtype=torch.int32, device=dev)           # [cur, draft 0 .. draft k-1]
        self.prompt = torch.zeros(max_ctx, dtype=torch.int32, device=dev)
        self.pred = torch.zeros(max_ctx, dtype=torch.int32, device=dev)    # the request's prediction (vis_spec_draft_pred)
        ints = torch.zeros(16, dtype=torch.int32, device=dev)
        self.n_draft, self.limit, self.prompt_len, self.gen_start = ints[0:1], ints[1:2], ints[2:3], ints[3:4]
        self.counters = ints[4:7]                                           # steps, proposed, accepted
        self.pred_len, self.pred_state = ints[8:9], ints[9:16]              # ... and the PredState ints behind its length
        self._ints = ints
        # what vis_spec_accept_sampled reads at run time: the bits of the f32 inv_temp, the uint32 seed (8 bytes)
        self.params = torch.zeros(2, dtype=torch.int32, device=dev)

    @property
    def cur(self) -> torch.Tensor:
        return self.ids[0:1]

    @property
    def draft(self) -> torch.Tensor:
        return self.ids[1:]

    def begin(self, cur_token: torch.Tensor, prompt_ids: torch.Tensor, step0: int, limit: int,
              prediction: Optional[Sequence[int]] = None) -> None:
        """A request starts behind its prompt pass: the first token, the prompt's ids, no drafts yet, counters at zero.
        ``step0``: the index of the token row the prompt pass's pick went to; ``limit``: the last one the reply may use.
        ``prediction``: the ids of the request's predicted reply (at most the buffer's size is kept), its drafter state zeroed."""
        n = prompt_ids.numel()
        self.prompt[:n].copy_(prompt_ids)
        self.ids.zero_()
        self.ids[0:1].copy_(cur_token)
        p = list(prediction or ())[:self.pred.numel()]
        if p:
            self.pred[:len(p)].copy_(torch.tensor(p, dtype=torch.int32))
        self._ints.copy_(torch.tensor([0, limit, n, step0, 0, 0, 0, 0, len(p)] + list(PredState()), dtype=torch.int32),
                         non_blocking=False)

    def set_params(self, temperature: float, seed: int) -> None:
        """The sampled accept's parameters of the request starting: inv_temp as hip.argmax forms it (the double quotient
        narrowed to f32; 0 at temperature 0 = the greedy pick) and the seed modulo 2^32."""
        inv_temp = np.float32((1.0 / temperature) if temperature > 0 else 0.0)
        raw = np.array([inv_temp.view(np.uint32), int(seed) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
        self.params.copy_(torch.from_numpy(raw))

    def read_counters(self) -> List[int]:
        return [int(v) for v in self.counters.cpu().tolist()]

    def read_pred_state(self) -> PredState:
        return PredState(*(int(v) for v in self.pred_state.cpu().tolist()))
