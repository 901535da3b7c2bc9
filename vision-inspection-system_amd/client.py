"""Boundary B1: a ``chat.completions.create``-shaped client backed by the local MI355X engine.

The reference talks to its models through exactly one call shape,
    client.chat.completions.create(model=, messages=, temperature=, max_tokens=).choices[0].message.content
(``huggingface_hub.InferenceClient`` at src/agents/vlm_inspector.py:32,:105-111 and
src/agents/vlm_auditor.py:152-158; ``groq.Groq`` at :117-129; text-only health check
vlm_inspector.py:533-544).  ``LocalVLMClient`` offers the same attribute chain and return shape, so
the reference's agents can be pointed at it without touching their code.

Errors: ordinary exceptions whose messages never contain "429", "rate", "413" or "payload" - the
substrings the reference's retry logic keys on (vlm_inspector.py:113-140).
"""
from __future__ import annotations

import logging
import os
import threading
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

from .config import LOCAL_PROVIDER, Qwen2VLConfig
from .fork import check_n      # noqa: F401  (re-exported: the client's check of ``n``)

logger = logging.getLogger("vision_inspection_system_amd.client")


# ----------------------------------------------------------------------------- response objects
@dataclass
class _Message:
    content: str
    role: str = "assistant"


@dataclass
class TopLogprob:
    token: str
    bytes: List[int]
    logprob: float


@dataclass
class TokenLogprob:
    """One completion token of ``choice.logprobs.content`` (OpenAI's ChatCompletionTokenLogprob)."""
    token: str
    bytes: List[int]
    logprob: float
    top_logprobs: List[TopLogprob] = field(default_factory=list)


@dataclass
class ChoiceLogprobs:
    content: List[TokenLogprob]


@dataclass
class _Choice:
    message: _Message
    index: int = 0
    finish_reason: str = "stop"
    logprobs: Optional[ChoiceLogprobs] = None      # set only when the request asked for logprobs=True


@dataclass
class ChatCompletion:
    choices: List[_Choice]
    model: str = ""
    usage: Dict[str, int] = field(default_factory=dict)
    # device time per stage of the batch this reply was part of (extension; the reference logs wall time only:
    # vlm_inspector.py:473-479): {"prefill_ms", "decode_ms", "decode_steps", "sequences", "prompt_tokens"}
    timings: Dict[str, float] = field(default_factory=dict)


@dataclass
class _Delta:
    role: Optional[str] = None
    content: Optional[str] = None


@dataclass
class _ChunkChoice:
    delta: _Delta
    index: int = 0
    finish_reason: Optional[str] = None
    logprobs: Optional[ChoiceLogprobs] = None      # always None: per-chunk logprobs are not offered


@dataclass
class ChatCompletionChunk:
    """One element of a ``stream=True`` reply (OpenAI's chat.completion.chunk).  Per choice: first a chunk whose delta has
    role "assistant" and empty content, then content chunks, then one with an empty delta and the finish_reason; with
    stream_options={"include_usage": True} a last chunk with no choices and the usage."""
    choices: List[_ChunkChoice]
    model: str = ""
    object: str = "chat.completion.chunk"
    usage: Optional[Dict[str, int]] = None
    request_index: int = 0      # extension: which request of a complete_many call the chunk belongs to


def _role_chunk(model: str, request: int, choice: int) -> ChatCompletionChunk:
    return ChatCompletionChunk([_ChunkChoice(_Delta(role="assistant", content=""), index=choice)], model, request_index=request)


def _content_chunk(model: str, request: int, choice: int, text: str) -> ChatCompletionChunk:
    return ChatCompletionChunk([_ChunkChoice(_Delta(content=text), index=choice)], model, request_index=request)


def _finish_chunk(model: str, request: int, choice: int, reason: str) -> ChatCompletionChunk:
    return ChatCompletionChunk([_ChunkChoice(_Delta(), index=choice, finish_reason=reason)], model, request_index=request)


def _usage_chunk(model: str, request: int, usage: Dict[str, int]) -> ChatCompletionChunk:
    return ChatCompletionChunk([], model, usage=dict(usage), request_index=request)


def _chunks_of(completion: "ChatCompletion", request: int, include_usage: bool):
    """A finished reply as its chunk sequence: role, one content chunk and the finish chunk per choice."""
    for c in completion.choices:
        yield _role_chunk(completion.model, request, c.index)
        if c.message.content:
            yield _content_chunk(completion.model, request, c.index, c.message.content)
        yield _finish_chunk(completion.model, request, c.index, c.finish_reason)
    if include_usage:
        u = completion.usage or {"prompt_tokens": 0, "completion_tokens": 0, "total_tokens": 0}
        yield _usage_chunk(completion.model, request, u)


class ChatCompletionStream:
    """What ``create(..., stream=True)`` returns: an iterator of ChatCompletionChunk.  The engine call runs on a worker
    thread (under the engine's lock, as every call); ``next()`` polls the request's StreamReader - host memory the GPU
    publishes every token to while the decode loop runs (stream.py) - and never touches the GPU.  An exception of the worker
    (a JsonModeError, a request that failed to decode) is raised from ``next()``.  ``close()``, leaving a ``with`` block or
    dropping the iterator cancels the request: the engine's loop ends at its next ``check_every`` boundary.
    ``worker_done`` is set when the engine call has returned."""

    def __init__(self, run, reader, model_id: str, include_usage: bool, hold_text: bool):
        # the worker and the generator hold ``state``, never this object: dropping the iterator runs __del__ at once
        self._reader = reader
        self.worker_done = threading.Event()
        state = {"result": None, "error": None, "done": self.worker_done}

        def work():
            try:
                state["result"] = run(reader)
            except BaseException as e:      # noqa: BLE001 - handed to the consumer
                state["error"] = e
            finally:
                state["done"].set()

        self._gen = self._chunks(state, reader, model_id, include_usage, hold_text)
        self._thread = threading.Thread(target=work, name="vis-stream", daemon=True)
        self._thread.start()

    @staticmethod
    def _chunks(state, reader, model, include_usage, hold_text):
        started = set()
        done = state["done"]
        while True:
            finished = done.is_set()      # read BEFORE the poll: a poll after it has everything
            events = reader.poll()
            if not hold_text:
                for ev in events:
                    if (ev.request, ev.choice) not in started:
                        started.add((ev.request, ev.choice))
                        yield _role_chunk(model, ev.request, ev.choice)
                    yield _content_chunk(model, ev.request, ev.choice, ev.text)
            if finished:
                break
            if not events:
                done.wait(0.001)
        if state["error"] is not None:
            raise state["error"]
        failed = None
        for j, comp in enumerate(state["result"]):
            if isinstance(comp, Exception):
                failed = failed or comp
                continue
            for c in comp.choices:
                if (j, c.index) not in started:
                    yield _role_chunk(model, j, c.index)
                    if hold_text and c.message.content:      # VIS_SYNTHETIC_REPLY: the substituted text, once
                        yield _content_chunk(model, j, c.index, c.message.content)
                yield _finish_chunk(model, j, c.index, c.finish_reason)
            if include_usage:
                yield _usage_chunk(model, j, comp.usage)
        if failed is not None:
            raise failed

    def __iter__(self):
        return self

    def __next__(self) -> ChatCompletionChunk:
        return next(self._gen)

    def close(self) -> None:
        self._reader.cancel()
        self._gen.close()
        if self._thread is not threading.current_thread():
            self._thread.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        self._reader.cancel()


class _Completions:
    def __init__(self, owner):
        self._owner = owner

    def create(self, model: Optional[str] = None, messages: Optional[list] = None,
               temperature: Optional[float] = None, max_tokens: Optional[int] = None, logprobs: bool = False,
               top_logprobs: Optional[int] = None, response_format: Optional[dict] = None, top_p: Optional[float] = None,
               seed: Optional[int] = None, frequency_penalty: Optional[float] = None,
               presence_penalty: Optional[float] = None, repetition_penalty: Optional[float] = None,
               stop=None, top_k: Optional[int] = None, min_p: Optional[float] = None,
               logit_bias: Optional[dict] = None, n: Optional[int] = None, stream: Optional[bool] = None,
               stream_options: Optional[dict] = None, no_repeat_ngram_size: Optional[int] = None,
               bad_words: Optional[list] = None, min_tokens: Optional[int] = None, speculative=None,
               prediction: Optional[dict] = None, **kwargs):
        """One request; LocalVLMClient._complete_many describes the keywords not described here.
        ``stream=True``: an iterator of ChatCompletionChunk instead of a ChatCompletion (``stream_options``: OpenAI's
        {"include_usage": True}); None or False: the call of before.
        ``speculative`` (extension; vLLM's names): {"method": "ngram", "num_speculative_tokens": k in 1..3[, "prompt_lookup_max": 4,
        "prompt_lookup_min": 2, "sampled": False, "grammar": False, "schema_drafts": True]} - lossless n-gram speculative decoding (request.Switches says how): the same
        text and usage in fewer weight passes where the reply repeats earlier text.  A single request of a Qwen2-VL model only:
        ValueError with ``n`` > 1 or any other sampling / constraint / stop / stream / logprobs keyword, and with a temperature
        or a seed unless ``"sampled": True`` opts in (the plain sampled reply), and with a json_schema ``response_format`` unless ``"grammar": True`` does (spec.py).  None: the call of before.
        ``prediction`` (OpenAI's Predicted Outputs): {"type": "content", "content": text} - or content as a list of {"type":
        "text", "text": ...} parts - text the reply will probably repeat: the previous reply of a retry, the report of an
        earlier inspection of the same part, a fixed template.  The speculative step drafts from it; the text and
        finish_reason are those of the call without it, and ``usage["completion_tokens_details"]`` = {"accepted_prediction_tokens",
        "rejected_prediction_tokens"} counts the prediction's drafts the steps kept and did not keep (over every step issued:
        those of a poll interval that ran past an EOS included).  Alone it implies k = 3 and the lookup window 4..2;
        ``speculative`` next to it sets them.  The conditions and refusals of ``speculative``; an empty text is no
        prediction.  None: the call of before."""
        from .stream import check_stream, check_stream_options
        if check_stream(stream):
            if logprobs:
                raise ValueError("stream=True together with logprobs=True is not supported: chunks carry no logprobs")
            kwargs["stream"] = True
            if check_stream_options(stream_options, True):
                kwargs["stream_options"] = stream_options
        else:
            check_stream_options(stream_options, False)
        given = {"frequency_penalty": frequency_penalty, "presence_penalty": presence_penalty,
                 "repetition_penalty": repetition_penalty, "stop": stop, "top_k": top_k, "min_p": min_p,
                 "logit_bias": logit_bias, "n": n, "no_repeat_ngram_size": no_repeat_ngram_size, "bad_words": bad_words,
                 "min_tokens": min_tokens, "speculative": speculative, "prediction": prediction}
        kwargs.update({name: v for name, v in given.items() if v is not None})
        return self._owner._complete(model, messages or [], temperature, max_tokens, logprobs=logprobs,
                                     top_logprobs=top_logprobs, response_format=response_format, top_p=top_p, seed=seed,
                                     **kwargs)


class _Chat:
    def __init__(self, owner):
        self.completions = _Completions(owner)


# device time of every generate_batch group served in this process (extension; bench.py --workload batch256 reads and
# clears it): [{"model", "prefill_ms", "decode_ms", "decode_steps", "sequences", "prompt_tokens"}]
TIMING_LOG: List[dict] = []

# ----------------------------------------------------------------------------- engine registry
_ENGINES: Dict[tuple, Any] = {}      # (model id, device) + an mllama engine's _auditor_key()
_ENGINES_LOCK = threading.Lock()


@dataclass
class LoadedModel:
    engine: Any
    tokenizer: Any
    cfg: Any
    model_id: str
    family: str = "qwen2_vl"      # or "mllama" (row f2: the Auditor's Llama-3.2-11B-Vision fallback)

    def __post_init__(self):
        if hasattr(self.engine, "tokenizer") and self.engine.tokenizer is None:
            self.engine.tokenizer = self.tokenizer      # JSON mode builds its token table from the vocabulary's bytes


def resolve_model_dir(model_id: str) -> Optional[str]:
    """A hub-style name is only ever mapped to a LOCAL directory: ``$VIS_MODEL_ROOT/<name>`` or
    ``$VIS_MODEL_ROOT/<org>--<name>``.  Nothing is downloaded."""
    if os.path.isdir(model_id):
        return model_id
    root = os.environ.get("VIS_MODEL_ROOT")
    if root:
        for cand in (os.path.join(root, model_id), os.path.join(root, model_id.replace("/", "--")),
                     os.path.join(root, model_id.split("/")[-1])):
            if os.path.isdir(cand):
                return cand
    return None


def get_model(model_id: str, device: Optional[str] = None) -> LoadedModel:
    """Process-wide singleton per (model, device): the reference constructs a NEW agent object on every
    node call (src/orchestration/nodes.py:128,:230), so the 16.6 GB model must not live in the agent."""
    import torch
    from .engine import Qwen2VLEngine
    from .tokenizer import ByteTokenizer, HFTokenizer
    from . import spec_batch, weights as W
    sbc = spec_batch.from_env()      # VIS_SPECULATIVE_BATCH: a Qwen2-VL engine built with it is another engine, under a key of its own
    if device is None:
        with _ENGINES_LOCK:      # a model that is already loaded / registered on exactly one device: no device query needed
            hits = [k for k in _ENGINES if k[0] == model_id and sbc is None]
            if any(len(k) > 2 for k in hits):      # mllama entries carry their settings: the entry of the current ones
                aud = _auditor_key()
                hits = [k for k in hits if len(k) == 2 or k[2:] == aud]
            if len(hits) == 1:
                return _ENGINES[hits[0]]
        device = f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0"
    key = (model_id, str(device))
    skey = () if sbc is None else ("batch_speculative",) + key + tuple(sbc)
    with _ENGINES_LOCK:
        if skey in _ENGINES:
            return _ENGINES[skey]
        # (with the setting on, the plain entry serves only when its engine was built with the same setting by the caller)
        if key in _ENGINES and (sbc is None or getattr(_ENGINES[key].engine, "batch_speculative", None) == sbc):
            return _ENGINES[key]
        # an mllama engine is cached under its quantisation settings too (VIS_AUDITOR_*, fixed per engine); the variables are
        # read only where an mllama model is loaded or already cached, so a malformed one cannot fail another model's load
        if any(k[:2] == key and len(k) > 2 for k in _ENGINES):
            akey = key + _auditor_key()
            if akey in _ENGINES:
                return _ENGINES[akey]
        # KV-cache rows per sequence.  Default: the reference's request fits as the reference sends it - ~2300 prompt tokens
        # (inspection prompt + one 1024 x 1024 image) + its own default max_tokens = 2048 (/root/reference utils/config.py:50-53)
        # = 4348 -> 4608 (72 context splits: the chained decode launch stays resident up to ~6700)
        max_ctx = int(os.environ.get("VIS_MAX_CTX", "4608"))
        max_batch = max(1, min(64, int(os.environ.get("VIS_MAX_BATCH", "64"))))
        mllama = _load_mllama(model_id, device, max_ctx, max_batch)
        if mllama is not None:
            _ENGINES[key + _auditor_key()] = mllama
            return mllama
        if model_id.startswith("synthetic:"):
            parts = model_id.split(":")
            kind = parts[1]
            seed = int(parts[2]) if len(parts) > 2 else 0
            if kind == "tiny":
                cfg = Qwen2VLConfig.tiny()
                w = W.pack_device_weights(cfg, W.synth_state_dict(cfg, seed), device)
                max_ctx = min(max_ctx, int(os.environ.get("VIS_TINY_MAX_CTX", "1024")))
            elif kind in ("7b", "qwen2-vl-7b"):
                cfg = Qwen2VLConfig.qwen2_vl_7b()
                w = W.random_device_weights(cfg, device, seed)
            elif kind in ("tiny25", "qwen2.5-vl-tiny"):
                cfg = Qwen2VLConfig.tiny_2_5()
                w = W.pack_device_weights(cfg, W.synth_state_dict(cfg, seed), device)
                max_ctx = min(max_ctx, int(os.environ.get("VIS_TINY_MAX_CTX", "1024")))
            elif kind in ("7b25", "qwen2.5-vl-7b"):
                cfg = Qwen2VLConfig.qwen2_5_vl_7b()
                w = W.random_device_weights(cfg, device, seed)
            else:
                raise ValueError(f"unknown synthetic model {kind!r} (use synthetic:tiny, synthetic:7b, synthetic:tiny25 "
                                 f"or synthetic:qwen2.5-vl-7b)")
            tok = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
        else:
            path = resolve_model_dir(model_id)
            if path is None:
                raise FileNotFoundError(
                    f"model {model_id!r} is not a local directory and VIS_MODEL_ROOT has no copy of it; the "
                    f"'{LOCAL_PROVIDER}' provider only loads local files (config.json, *.safetensors, tokenizer.json)")
            local_model_type(path)          # refuses anything but qwen2_vl / qwen2_5_vl (mllama was handled above)
            cfg = Qwen2VLConfig.from_hf_dir(path)
            w = W.load_safetensors_dir(cfg, path, device)
            tok = HFTokenizer(path, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
        lm = LoadedModel(Qwen2VLEngine(cfg, w, device, max_ctx=max_ctx, max_batch=max_batch,
                                       decode_weights=os.environ.get("VIS_DECODE_WEIGHTS", "bf16"),
                                       prefill_dtype=os.environ.get("VIS_PREFILL_DTYPE", "bf16"),
                                       mxfp4_gemm_from=_env_int_or_none("VIS_MXFP4_GEMM_FROM"),
                                       **({} if sbc is None else {"batch_speculative": sbc})), tok, cfg, model_id)
        _ENGINES[skey or key] = lm
        return lm


def _env_int_or_none(name: str) -> Optional[int]:
    """An integer switch from the environment; unset or empty means None, anything but an integer is a ValueError."""
    v = os.environ.get(name, "").strip()
    return int(v) if v else None


def _auditor_settings() -> tuple:
    """(decode_weights, mxfp4_gemm_from, cross_kv) of an mllama engine from VIS_AUDITOR_DECODE_WEIGHTS, VIS_AUDITOR_MXFP4_GEMM_FROM
    and VIS_AUDITOR_CROSS_KV; unset: ("bf16", None, "bf16").  VIS_DECODE_WEIGHTS is the Qwen2-VL engines' and is not read here."""
    return (os.environ.get("VIS_AUDITOR_DECODE_WEIGHTS", "").strip() or "bf16", _env_int_or_none("VIS_AUDITOR_MXFP4_GEMM_FROM"),
            os.environ.get("VIS_AUDITOR_CROSS_KV", "").strip() or "bf16")


def _auditor_speculative() -> bool:
    """VIS_AUDITOR_SPECULATIVE=k (1..3) is set: the mllama engine is built with speculative=True and the clients accept
    ``speculative`` / ``prediction`` for one request of an mllama model.  Read at every call; a malformed value is a ValueError."""
    from .spec import auditor_from_env
    return auditor_from_env() is not None


def _auditor_key() -> tuple:
    """What an mllama engine is cached under behind (model id, device): _auditor_settings(), and one further element while
    VIS_AUDITOR_SPECULATIVE is set (the engine built for speculative requests is another engine).  Unset: today's key."""
    return _auditor_settings() + (("speculative",) if _auditor_speculative() else ())


def _auditor_kwargs() -> dict:
    """The constructor keywords the VIS_AUDITOR_* variables set; nothing set -> no keyword (the bf16 engine's call as it was)."""
    dw, gf, xkv = _auditor_settings()
    kw = {}
    if _auditor_speculative():
        kw["speculative"] = True
    if dw != "bf16":
        kw["decode_weights"] = dw
    if gf is not None:
        kw["mxfp4_gemm_from"] = gf
    if xkv != "bf16":
        kw["cross_kv"] = xkv
    return kw


def _load_mllama(model_id: str, device, max_ctx: int, max_batch: int = 1) -> Optional[LoadedModel]:
    """mllama family (synthetic:mllama-tiny[:seed], synthetic:mllama-11b, or a local directory whose config.json
    says model_type "mllama"); None when ``model_id`` is not an mllama model.  VIS_AUDITOR_DECODE_WEIGHTS / _MXFP4_GEMM_FROM /
    _CROSS_KV choose the engine's decode weight format and the format of its cross-attention keys, VIS_AUDITOR_SPECULATIVE
    whether it serves speculative requests (MllamaEngine)."""
    import json
    from . import mllama_weights as MW
    from .mllama_engine import MllamaEngine
    from .tokenizer import LlamaByteTokenizer, LlamaHFTokenizer
    if model_id.startswith("synthetic:mllama"):
        parts = model_id.split(":")
        seed = int(parts[2]) if len(parts) > 2 else 0
        if parts[1] == "mllama-tiny":
            cfg = MW.MllamaConfig.tiny()
            w = MW.pack_device_weights(cfg, MW.synth_state_dict(cfg, seed), device)
            max_ctx = min(max_ctx, int(os.environ.get("VIS_TINY_MAX_CTX", "1024")))
        elif parts[1] in ("mllama-11b", "mllama"):
            cfg = MW.MllamaConfig.mllama_11b()
            w = MW.random_device_weights(cfg, device, seed)
        else:
            raise ValueError(f"unknown synthetic model {parts[1]!r}")
        tok = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
        return LoadedModel(MllamaEngine(cfg, w, device, max_ctx=max_ctx, max_batch=max_batch, **_auditor_kwargs()), tok, cfg, model_id, "mllama")
    path = resolve_model_dir(model_id)
    if path is None or not os.path.exists(os.path.join(path, "config.json")):
        return None
    with open(os.path.join(path, "config.json")) as f:
        if json.load(f).get("model_type") != "mllama":
            return None
    cfg = MW.config_from_hf_dir(path)
    w = MW.load_safetensors_dir(cfg, path, device)
    tok = LlamaHFTokenizer(path, cfg.image_token_id, cfg.eos_ids)
    return LoadedModel(MllamaEngine(cfg, w, device, max_ctx=max_ctx, max_batch=max_batch, **_auditor_kwargs()), tok, cfg, model_id, "mllama")


def _reply_text(model_id: str, decoded: str) -> str:
    """Throughput runs on ``synthetic:`` (seeded random) weights generate noise, which would send every image down the
    agents' failure + retry path (nodes.py retries with back-off) and time THAT instead of the pipeline.  For synthetic
    models only, VIS_SYNTHETIC_REPLY substitutes a fixed reply text AFTER the full generation has run (tools/ingest_bench.py);
    real checkpoints are never affected."""
    if model_id.startswith("synthetic:"):
        fixed = os.environ.get("VIS_SYNTHETIC_REPLY")
        if fixed:
            return fixed
    return decoded


def _finish_reason(fin) -> str:
    """An engine's ``last_finish`` entry as OpenAI's finish_reason: "stop" for EOS or a stop string, "length" for a reply
    that max_tokens or the context cut off (an engine stand-in without the record: "stop", as before)."""
    return "length" if fin is not None and fin[0] == "length" else "stop"


def _finished_text(tok, toks: List[int], fin) -> str:
    """The reply text of the returned tokens: on a stop match their bytes up to where the stop string starts (UTF-8, a
    sequence the cut split is replaced), else what the tokenizer decodes."""
    if fin is not None and fin[0] == "stop":
        return b"".join(tok.token_bytes(t) for t in toks)[:fin[1]].decode("utf-8", errors="replace")
    return tok.decode(toks)


def logprobs_k(logprobs, top_logprobs) -> Optional[int]:
    """OpenAI's (logprobs, top_logprobs) -> None (off) or the number of alternatives per token.  Checked before any model
    is loaded; the messages avoid the substrings the reference's retry logic keys on."""
    from .logprobs import MAX_TOP_LOGPROBS
    if top_logprobs is not None:
        if not logprobs:
            raise ValueError("top_logprobs needs logprobs=True")
        if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, int) or not 0 <= top_logprobs <= MAX_TOP_LOGPROBS:
            raise ValueError(f"top_logprobs must be an integer in 0..{MAX_TOP_LOGPROBS}")
    if not logprobs:
        return None
    return int(top_logprobs or 0)


def check_speculative_request(speculative, temperature=None, seed=None, *, prediction=None, **switches):
    """``speculative`` and ``prediction`` of one ``create`` call, checked without a model: spec.check_speculative's record
    (what a prediction alone implies: spec.PRED_DEFAULT; None when neither is on), or ValueError when a dict is malformed or
    the request carries something a speculative step cannot (spec.check_exclusive names it)."""
    from . import spec
    text = spec.check_prediction(prediction)
    sp = spec.with_prediction(speculative, text is not None)
    spec.check_exclusive(sp, float(temperature) if temperature else 0.0, seed,
                         what="speculative" if text is None else "prediction (speculative decoding)", **switches)
    return sp


def is_mllama_model(model_id: Optional[str]) -> bool:
    """Whether ``model_id`` names a model of the mllama family, found out without loading it."""
    import json
    if not model_id:
        return False
    if model_id.startswith("synthetic:"):
        return model_id.startswith("synthetic:mllama")
    path = resolve_model_dir(model_id)
    if path is None or not os.path.exists(os.path.join(path, "config.json")):
        return False
    with open(os.path.join(path, "config.json")) as f:
        return json.load(f).get("model_type") == "mllama"


def check_ban_keywords(no_repeat_ngram_size, bad_words, min_tokens, max_tokens, response_format) -> dict:
    """``no_repeat_ngram_size`` / ``bad_words`` / ``min_tokens`` of one request, checked without a model (ban.check_ban; how
    many ids a word has is the tokenizer's to say, when the request is switched on): the engine keywords that are on ({} when
    none is).  ``min_tokens`` is held against ``max_tokens`` (the client's default of 512 when that is not given); together
    with a response_format that turns a grammar on they are a ValueError."""
    from .ban import ban_kwargs, check_ban
    grammar = isinstance(response_format, dict) and response_format.get("type") in ("json_object", "json_schema")
    ban = check_ban(no_repeat_ngram_size, bad_words, min_tokens, 1, int(max_tokens) if max_tokens else 512, json_mode=grammar)
    return {name: v for name, v in ban_kwargs(ban).items() if v}


def json_mode_of(response_format) -> bool:
    """OpenAI's response_format -> JSON mode on / off: None or {"type": "text"} = off, {"type": "json_object"} = on
    (json_grammar: the reply is a JSON object).  Anything else raises ValueError; checked before any model is loaded, and
    the message avoids the substrings the reference's retry logic keys on."""
    if response_format is None:
        return False
    kind = response_format.get("type") if isinstance(response_format, dict) else None
    if kind == "text":
        return False
    if kind == "json_object":
        return True
    raise ValueError("response_format: only {'type': 'text'} and {'type': 'json_object'} turn JSON mode on or off "
                     "(json_schema goes through schema_of; other grammars are unsupported)")


_SCHEMA_CACHE: dict = {}
_SCHEMA_CACHE_MAX = 64


def schema_of(response_format):
    """OpenAI's response_format -> the compiled SchemaDFA of {"type": "json_schema", "json_schema": {"name": ..., "schema":
    {...}, "strict": ...}}, or None for every other form (json_mode_of judges those).  The schema is compiled here, before
    any model is loaded: what json_schema.compile_schema does not support is a ValueError naming the cause.  ``strict`` may be
    true, false or absent - the reply always conforms.  Compiled DFAs are cached by the schema's canonical JSON text."""
    if not isinstance(response_format, dict) or response_format.get("type") != "json_schema":
        return None
    from . import json_schema
    spec = response_format.get("json_schema")
    if not isinstance(spec, dict) or not isinstance(spec.get("schema"), dict):
        raise ValueError("response_format json_schema: needs {'json_schema': {'name': ..., 'schema': {...}}}")
    extra = set(response_format) - {"type", "json_schema"} | set(spec) - {"name", "schema", "strict", "description"}
    if extra:
        raise ValueError(f"response_format json_schema: unknown field(s) {sorted(extra)}")
    if "name" in spec and not isinstance(spec["name"], str) or not isinstance(spec.get("strict", True), bool):
        raise ValueError("response_format json_schema: 'name' must be a string and 'strict' true or false")
    try:
        key = json_schema.canonical(spec["schema"])
    except (TypeError, ValueError) as e:
        raise ValueError(f"response_format json_schema: the schema is not JSON ({e})") from None
    with _ENGINES_LOCK:
        dfa = _SCHEMA_CACHE.get(key)
    if dfa is None:
        dfa = json_schema.compile_schema(spec["schema"])
        with _ENGINES_LOCK:
            if len(_SCHEMA_CACHE) >= _SCHEMA_CACHE_MAX:
                _SCHEMA_CACHE.pop(next(iter(_SCHEMA_CACHE)))
            dfa = _SCHEMA_CACHE.setdefault(key, dfa)
    return dfa


# The one list of the request keywords of ``create`` / ``complete_many`` (_complete_many describes each; ``speculative`` and
# ``prediction`` are ``create``'s own), in the order in which a speculative request names its conflicts.
REQUEST_KEYWORDS = ("logprobs", "top_logprobs", "response_format", "top_p", "seed", "frequency_penalty", "presence_penalty",
                    "repetition_penalty", "stop", "top_k", "min_p", "logit_bias", "n", "stream", "stream_options",
                    "no_repeat_ngram_size", "bad_words", "min_tokens")


def _request_keywords(kwargs: dict, where: Optional[str] = None) -> dict:
    """The REQUEST_KEYWORDS among ``kwargs``, in the list's order; with ``where``, any other one is that function's TypeError."""
    for name in kwargs if where else ():
        if name not in REQUEST_KEYWORDS:
            raise TypeError(f"{where}() got an unexpected keyword argument {name!r}")
    return {name: kwargs[name] for name in REQUEST_KEYWORDS if name in kwargs}


def engine_keywords(max_tokens=None, **kw) -> Tuple[dict, Optional[int]]:
    """The request keywords of one call (REQUEST_KEYWORDS; another one is a TypeError), checked without a model - ValueError
    for the first one that is malformed - and translated: (the engine keywords that are on, the checked ``seed``).  Not
    looked at here: ``n`` (it needs the engine's max_batch) and ``stream`` / ``stream_options`` (the caller's)."""
    from .penalties import check_penalties
    from .request import PENALTY_NAMES
    from .sampling import check_seed, check_top_p
    from .shaping import check_shaping, shaping_kwargs
    from .stop import check_stop
    kw = _request_keywords(kw, "engine_keywords")
    response_format = kw.get("response_format")
    on = {"logprobs": logprobs_k(kw.get("logprobs", False), kw.get("top_logprobs")), "json_schema": schema_of(response_format)}
    on["json_mode"] = (json_mode_of(response_format) if on["json_schema"] is None else False) or None
    on["top_p"] = check_top_p(kw.get("top_p"))
    on["stop"] = check_stop(kw.get("stop"))
    seed = check_seed(kw.get("seed"))
    pen = check_penalties(*(kw.get(name) for name in PENALTY_NAMES), 1)
    on.update({} if pen is None else zip(PENALTY_NAMES, pen[0]))
    on.update(shaping_kwargs(check_shaping(kw.get("top_k"), kw.get("min_p"), kw.get("logit_bias"), 1)))
    on.update(check_ban_keywords(kw.get("no_repeat_ngram_size"), kw.get("bad_words"), kw.get("min_tokens"), max_tokens,
                                 response_format))
    return {name: v for name, v in on.items() if v is not None}, seed


def _prediction_ids(lm: "LoadedModel", prediction: Optional[str]) -> dict:
    """The text of a request's prediction as ``generate``'s keyword: tokenised without special tokens, at most the engine's
    max_ctx ids; {} without one."""
    return {"prediction": lm.tokenizer.encode(prediction)[:lm.engine.max_ctx]} if prediction else {}


def _log_timing(model_id: str, timing: dict) -> None:
    TIMING_LOG.append({"model": model_id, **timing})
    del TIMING_LOG[:-4096]


def _image_urls(messages):
    """The URL of every ``image_url`` part of ``messages``, in order."""
    for m in messages:
        content = m.get("content")
        if isinstance(content, list):
            for part in content:
                if part.get("type") == "image_url":
                    yield part["image_url"]["url"] if isinstance(part.get("image_url"), dict) else part["image_url"]


def _completion(model_id: str, tok, n_ids: int, toks, rec, fin, timing: dict, nested: bool) -> ChatCompletion:
    """One request's ChatCompletion from what the engine returned for it: a token list with its logprob record and (reason,
    cut) - or, ``nested`` (the request asked for n choices), a list of each.  The prompt is counted once."""
    if not nested:
        toks, rec, fin = [toks], [rec], [fin]
    elif rec is None:
        rec = [None] * len(toks)
    choices = [_Choice(_Message(_reply_text(model_id, _finished_text(tok, t, f))), index=i, finish_reason=_finish_reason(f),
                       logprobs=_choice_logprobs(tok, t, r) if r is not None else None)
               for i, (t, r, f) in enumerate(zip(toks, rec, fin))]
    done = sum(len(t) for t in toks)
    usage = {"prompt_tokens": n_ids, "completion_tokens": done, "total_tokens": n_ids + done}
    if "pred_accepted" in timing:      # the request came with a prediction (OpenAI's Predicted Outputs)
        usage["completion_tokens_details"] = {"accepted_prediction_tokens": timing["pred_accepted"],
                                              "rejected_prediction_tokens": timing["pred_rejected"]}
    return ChatCompletion(choices, model=model_id, usage=usage, timings=timing)


def _choice_logprobs(tok, toks: List[int], rec) -> ChoiceLogprobs:
    """An engine's TokenLogprobs record of one request -> choice.logprobs (one entry per completion token)."""
    def entry(cls, t, lp, **kw):
        b = tok.token_bytes(int(t))
        return cls(tok.token_text(int(t)), list(b), float(lp), **kw)
    return ChoiceLogprobs([entry(TokenLogprob, t, rec.token_logprobs[i],
                                 top_logprobs=[entry(TopLogprob, a, la) for a, la in zip(rec.top_ids[i], rec.top_logprobs[i])])
                           for i, t in enumerate(toks)])


def drop_models() -> None:
    with _ENGINES_LOCK:
        _ENGINES.clear()


def register_model(model_id: str, device: str, lm: LoadedModel) -> None:
    """Serve ``model_id`` on ``device`` from an engine the caller already built (bench.py times the client on the
    engine it has just measured instead of loading a second 16.6 GB replica)."""
    with _ENGINES_LOCK:
        _ENGINES[(model_id, str(device))] = lm


def unregister_model(model_id: str, device: str) -> None:
    with _ENGINES_LOCK:
        for k in [k for k in _ENGINES if (model_id, str(device)) in (k[:2], k[1:3])]:
            _ENGINES.pop(k)


SUPPORTED_MODEL_TYPES = ("qwen2_vl", "qwen2_5_vl", "mllama")


def local_model_type(path: str) -> str:
    """``model_type`` of a local HuggingFace directory, checked against what the engines implement.  The
    reference's code default for both agents is Qwen/Qwen2.5-VL-7B-Instruct (utils/config.py:42-45,:59-64), its
    README names Qwen2-VL-7B and Llama-3.2-11B-Vision; anything else is refused HERE with a clear message instead of
    failing with a KeyError deep inside a weight loader."""
    import json
    cfg_path = os.path.join(path, "config.json")
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"{cfg_path} not found: a local model directory needs config.json, *.safetensors and "
                                f"tokenizer.json")
    with open(cfg_path) as f:
        mt = json.load(f).get("model_type")
    if mt not in SUPPORTED_MODEL_TYPES:
        raise ValueError(f"model directory {path!r} has model_type {mt!r}; the '{LOCAL_PROVIDER}' provider serves "
                         f"{', '.join(SUPPORTED_MODEL_TYPES)} only")
    return mt


def _frame_to_device(f, device):
    """Host result of a request's decode -> uint8 [H, W, 3] device frame: either decoded pixels (PIL path, upload) or the
    entropy-decoded JPEG (upload of the coefficients + the IDCT / upsampling / colour kernels)."""
    import torch
    from . import jpeg
    if isinstance(f, jpeg.JpegCoeffs):
        return jpeg.to_rgb_device(f, device)
    from . import hip
    return hip.upload(f, device)


# ----------------------------------------------------------------------------- clients
class LocalVLMClient:
    """``InferenceClient``-shaped facade over the MI355X engine."""

    accepts_futures = True      # complete_many takes Futures of messages (agents.prepare_many) and streams them in

    def __init__(self, api_key: Optional[str] = None, device: Optional[str] = None, default_model: Optional[str] = None,
                 seed: int = 0, **_ignored):
        self.device = device
        self.default_model = default_model
        self.seed = seed
        self.chat = _Chat(self)

    def _prepare(self, lm, messages):
        """messages -> (token ids, [(decoded uint8 RGB frame, (target_h, target_w))]) for one request.
        The JPEG is decoded on the host; the bicubic resample to the smart_resize target runs on the GPU
        (hip.resize_rgb, bit-exact with PIL) unless VIS_GPU_RESIZE=0 asks for the host PIL path."""
        import numpy as np
        from . import jpeg
        from .image_processing import decode_data_uri, resize_for_model, target_size
        from .tokenizer import build_chat_ids
        cfg = lm.cfg
        gpu_resize = os.environ.get("VIS_GPU_RESIZE", "1") != "0"
        frames = []
        for url in _image_urls(messages):
            # baseline JPEG (what the reference's agents send): Huffman decode here, on this pool thread;
            # IDCT / upsampling / colour conversion on the GPU (jpeg.py).  Other flavours: PIL.
            jc = jpeg.parse_data_uri(url) if (gpu_resize and jpeg.enabled()) else None
            if jc is not None:
                frames.append((jc, target_size(jc.size, cfg.patch, cfg.merge, cfg.min_pixels, cfg.max_pixels)))
                continue
            img = decode_data_uri(url)
            th, tw = target_size(img.size, cfg.patch, cfg.merge, cfg.min_pixels, cfg.max_pixels)
            frames.append((np.array(img, dtype=np.uint8) if gpu_resize else
                           resize_for_model(img, cfg.patch, cfg.merge, cfg.min_pixels, cfg.max_pixels), (th, tw)))
        counts = [(th // cfg.patch) * (tw // cfg.patch) // cfg.merge ** 2 for _, (th, tw) in frames]
        return build_chat_ids(lm.tokenizer, messages, counts), frames

    def _complete(self, model, messages, temperature, max_tokens, speculative=None, prediction=None, **kwargs):
        from .spec import check_prediction, sampled_seed
        kw = _request_keywords(kwargs)      # an OpenAI keyword ``create`` swallowed and this client does not know ends here
        text = check_prediction(prediction)
        if speculative is not None or text is not None:
            sp = check_speculative_request(speculative, temperature, prediction=prediction,
                                           **{name: v for name, v in kw.items() if name != "stream_options"})
            if is_mllama_model(model or self.default_model) and not _auditor_speculative():
                raise ValueError(("speculative decoding is" if text is None else "prediction (speculative decoding) is") +
                                 " offered for Qwen2-VL / Qwen2.5-VL models only, unless VIS_AUDITOR_SPECULATIVE=k (1..3) "
                                 "has the Mllama engine built for it")
            return self._complete_many(model, [messages], temperature, max_tokens, speculative=sp, prediction=text,      # no other
                                       checked=sampled_seed(sp, kw.get("seed"), self.seed, kw.get("response_format")))[0]      # keyword is on
        out = self.complete_many(model, [messages], temperature, max_tokens, **kw)
        return out if isinstance(out, ChatCompletionStream) else out[0]

    def complete_many(self, model, batch_of_messages, temperature=None, max_tokens=None, *, prediction=None, **kw):
        """As ``_complete_many`` (``kw``: the REQUEST_KEYWORDS, described there; any other is a TypeError), plus ``stream``
        (OpenAI's): True returns ONE ChatCompletionStream over the chunks of all requests instead of the list - each chunk
        carries its request's index as ``request_index`` - while the engine call runs on a worker thread.  Every token is published from the GPU into
        host memory as it is picked (vis_stream_publish, stream.py), so text arrives while the decode loop runs and the
        loop keeps its launch-ahead; text that may still turn out to be the start of a stop string is held back.  The
        streamed text of a choice, its finish_reason and the usage are those of the same call not streamed.  Per choice:
        a chunk with ``delta.role`` "assistant" and empty content, content chunks, one chunk with an empty delta and the
        ``finish_reason``; ``stream_options={"include_usage": True}`` adds a chunk with ``choices=[]`` and the ``usage``
        per request.  Not together with ``logprobs``.  With VIS_SYNTHETIC_REPLY the substituted text comes as one content
        chunk after the generation.  Closing or dropping the iterator cancels the call at the loop's next poll; an exception
        of a request is raised from ``next()``; one of its arguments from this call.  None or False: the list, as before.
        ``prediction`` other than None is refused (ValueError): it belongs to the one request of ``create``."""
        from .spec import refuse_batch_prediction
        from .stream import StreamReader, check_stream, check_stream_options
        kw = _request_keywords(kw, "complete_many")
        refuse_batch_prediction(prediction)
        stream, stream_options = kw.pop("stream", None), kw.pop("stream_options", None)
        if not check_stream(stream):
            check_stream_options(stream_options, False)
            return self._complete_many(model, batch_of_messages, temperature, max_tokens, **kw)
        include_usage = check_stream_options(stream_options, True)
        if kw.get("logprobs"):
            raise ValueError("stream=True together with logprobs=True is not supported: chunks carry no logprobs")
        model_id = model or self.default_model
        if not model_id:
            raise ValueError("no model given")
        checked = engine_keywords(max_tokens, **kw)      # here, not on the worker: a bad argument raises from this call
        lm = get_model(model_id, self.device)
        hold = model_id.startswith("synthetic:") and bool(os.environ.get("VIS_SYNTHETIC_REPLY"))
        return ChatCompletionStream(
            lambda reader: self._complete_many(model, batch_of_messages, temperature, max_tokens, on_stream=reader,
                                               checked=checked, **kw),
            StreamReader(lm.tokenizer), model_id, include_usage, hold)

    def _complete_many(self, model, batch_of_messages, temperature=None, max_tokens=None, on_stream=None, speculative=None,
                       prediction: Optional[str] = None, checked=None, **kw) -> List[ChatCompletion]:
        """Several independent requests in one go: per-request prefill, then ONE shared decode loop in which every
        weight is streamed once per step for all of them (engine.generate_batch).  Groups larger than the
        engine's max_batch are processed in consecutive chunks.  Extension of the reference's call shape used by
        the batch path; ``chat.completions.create`` is the single-request form of it.
        ``logprobs`` / ``top_logprobs`` (OpenAI's): every choice gets ``logprobs.content``, one entry per completion token -
        the log-softmax of the model's raw logits (independent of temperature and seed) and the ``top_logprobs`` most
        likely alternatives.  With VIS_SYNTHETIC_REPLY (synthetic models) they describe the generated tokens, not the
        substituted text.
        ``response_format`` (OpenAI's): {"type": "json_object"} restricts every generated token to the ones that continue a
        JSON object (RFC 8259, strict UTF-8; the engines' json_mode): a reply that ended on EOS parses with json.loads, one cut
        by max_tokens is a prefix of a JSON object; a request the vocabulary could not continue fails with JsonModeError.
        {"type": "json_schema", "json_schema": {"name": ..., "schema": {...}, "strict": ...}}: the same with the schema as the
        grammar (json_schema.py: fixed keys in ``properties`` order, types, enum / const literals, nested objects and arrays,
        Optional as anyOf with null): a reply that ended on EOS is a document of the schema.  An unsupported schema is a
        ValueError before any model is loaded.
        None or {"type": "text"}: unchanged.  Logprobs keep their meaning: top_logprobs may list tokens the mask forbade.
        ``top_p`` (OpenAI's / huggingface_hub's): nucleus sampling - each token is drawn from the shortest most-likely set
        holding top_p of the temperature-scaled probability (sampling.py); None or 1 = the whole vocabulary.  ``seed``: every
        request of the call samples with this seed, so its reply depends on its own messages only (not on its place in the
        batch or what shares it); None = the client's seed, varied per batch slot as before.
        ``frequency_penalty`` / ``presence_penalty`` (OpenAI's / huggingface_hub's, in [-2, 2]): every logit is lowered by
        frequency_penalty times the number of times its token was generated so far, and by presence_penalty when it was
        generated at all.  ``repetition_penalty`` (extension, transformers' meaning, > 0): the logit of every token of the
        prompt or the reply so far is divided by it when positive, multiplied when negative.  Applied to the raw logits
        ahead of temperature, the JSON mask and top_p (penalties.py); None or 0 / 0 / 1 = off.  Logprobs keep their meaning.
        ``stop`` (OpenAI's): a string or up to 4 of them, each 1..64 bytes of UTF-8; the reply ends in front of the first
        occurrence of one in its bytes (stop.py, matched on the GPU) and never contains it; tokens, usage and logprobs run
        through the token that completed the match.  Every choice's ``finish_reason`` is "stop" when the reply ended on EOS
        or a stop string and "length" when max_tokens or the context cut it off.
        ``logit_bias`` (OpenAI's): {token id: bias in [-100, 100]}, at most 300 entries, ids as integers or decimal strings;
        the bias is added to the token's logit ahead of temperature: -100 bans a token, +100 all but forces it.  ``top_k``
        (vLLM's / huggingface_hub's, an integer >= 1): only the k most likely allowed tokens stay, ties at the k-th place
        included.  ``min_p`` (vLLM's, in [0, 1]): only tokens at least min_p times as likely as the most likely one stay.
        One launch ahead of the pick (shaping.py), after the penalties and the JSON mask, before top_p and the draw; a
        greedy request (temperature 0) is affected by logit_bias only.  None / 0 / {} = off.  Logprobs keep their meaning.
        ``n`` (OpenAI's): an integer in 1..max_batch - that many choices per request, ``choices[i].index`` = i, each with its
        own text, finish_reason and logprobs, from ONE prompt pass: the further choices read the prompt's keys / values from
        the first one's cache (fork.py, vis_decode_attn_forked).  Choice i samples with ``seed`` + i; at temperature 0 all
        choices are equal (and still decoded).  ``usage.prompt_tokens`` counts the prompt once, ``completion_tokens`` is the
        sum over the choices.  Chunks are filled by choices, max_batch // n requests each.  A request with a choice JSON mode
        could not continue fails as a whole.  None or 1 = one choice, the calls of before.
        ``no_repeat_ngram_size`` (transformers' / vLLM's, an integer in 1..64): no n-gram of prompt + reply occurs twice.
        ``bad_words`` (vLLM's): up to 16 strings of 1..8 tokens each that the reply never contains as token sequences; a word
        the tokenizer spells differently behind a space is banned in both spellings (both count against the 16).
        ``min_tokens`` (vLLM's, <= max_tokens): no EOS before that many completion tokens; it holds back EOS only, a ``stop``
        string may still end the reply earlier.  One launch ahead of the pick (ban.py), after the penalties.  None / 0 / []
        = off.  Not together with a ``response_format`` of json_object or json_schema: ValueError.  Checked before any GPU
        work.  Logprobs keep their meaning.
        ``speculative`` (a spec.SpecConfig, from ``create`` only - ``complete_many`` does not offer it): the ONE request of the
        call goes through the engine's ``generate(.., speculative=)``; every other keyword is off then (create checks; a sampled one keeps its seed).
        ``prediction`` (the text of create's ``prediction``, next to ``speculative``): tokenised without special tokens, at
        most the engine's max_ctx ids, handed to ``generate(.., prediction=)``; the completion's usage then carries
        ``completion_tokens_details``."""
        on, seed = checked or engine_keywords(max_tokens, **kw)
        k = on.get("logprobs")
        model_id = model or self.default_model
        if not model_id:
            raise ValueError("no model given")
        lm = get_model(model_id, self.device)
        eng, tok = lm.engine, lm.tokenizer
        max_new = int(max_tokens) if max_tokens else 512
        temp = float(temperature) if temperature else 0.0
        n = check_n(kw.get("n"), eng.max_batch)
        n = None if n == 1 else n
        if speculative is not None and (len(batch_of_messages) != 1 or
                                        (lm.family == "mllama" and not _auditor_speculative())):
            raise ValueError("speculative decoding serves one request of a Qwen2-VL / Qwen2.5-VL model per call (an mllama "
                             "model: with VIS_AUDITOR_SPECULATIVE=k set)")
        # What every engine call of this request group gets, built once: the switches that are on (an engine call without a
        # keyword is the call of before the keyword existed) and the ignore-EOS switch in the engine's spelling.
        ignore_eos = os.environ.get("VIS_IGNORE_EOS") == "1"
        gen = dict(max_new_tokens=max_new, temperature=temp, **on,
                   **({"stop_on_eos": not ignore_eos} if lm.family == "mllama" else {"ignore_eos": ignore_eos}))
        gen.update({name: v for name, v in (("n", n), ("on_stream", on_stream)) if v is not None})

        def serve(indices, request_of):
            """The requests ``indices`` of this call through generate_batch, in chunks filled by choices (max_batch // n
            requests each): yields (the chunk's indices, its results, logprob records, finishes and device timing)."""
            per_chunk = eng.max_batch // (n or 1)
            for i in range(0, len(indices), per_chunk):
                idx = indices[i:i + per_chunk]
                if on_stream is not None:
                    on_stream.requests = list(idx)      # which requests of the call this engine call serves
                if speculative is not None:      # one greedy request, no other switch: the single-sequence loop, speculating
                    ids, frames = request_of(idx[0])()
                    outs = [eng.generate(ids, frames, speculative=speculative, **_prediction_ids(lm, prediction), **gen)]
                else:
                    outs = eng.generate_batch([request_of(j) for j in idx], seed=self.seed, **gen,
                                              **({"seeds": [seed] * len(idx)} if seed is not None else {}))
                recs = eng.last_logprobs if k is not None else [None] * len(idx)
                fins = getattr(eng, "last_finish", None) or [None] * len(idx)
                timing = dict(getattr(eng, "last_timing", None) or {})
                if timing:
                    _log_timing(model_id, timing)
                yield idx, outs, recs, fins, timing

        if lm.family == "mllama":
            return self._complete_mllama_many(lm, batch_of_messages, gen, seed, serve, speculative, prediction)
        # Service-side decode (base64 + JPEG) of every request on the ingest pool.  A request may arrive as a Future of
        # its messages (the agents' prepare_many: the request-side encode is still running on the same pool); its decode
        # is queued the moment that encode finishes, ahead of the encodes still waiting (ingest.then).  The engine receives the
        # requests as callables and resolves them in order, so its first prompt pass starts as soon as image 0 is
        # decoded, and group i+1 decodes while group i is in its decode loop.
        # Eager requests (plain message lists): a request that fails to decode fails the call, like a malformed request
        # to the service.  Future requests: the failure (encode or decode) stays that request's own - its place in the
        # returned list holds the exception.
        from concurrent.futures import Future
        from . import hip, ingest
        lazy = any(isinstance(m, Future) for m in batch_of_messages)

        def prepare(msgs):
            with ingest.span("service-side decode (base64 + Huffman, pool thread)"):
                return self._prepare(lm, msgs)

        futs = [ingest.then(m, prepare) for m in batch_of_messages]
        n_ids = {}

        def resolver(j):
            def resolve():
                with ingest.span("engine thread: waiting for a request's encode + decode"):
                    ids, frames = futs[j].result()
                n_ids[j] = len(ids)
                if getattr(eng, "host_only", False):      # bench.py --dry-ingest: an engine stand-in that measures the host side
                    return ids, frames
                with ingest.span("engine thread: H2D of coefficients + IDCT / resize launches"):
                    return ids, [hip.resize_rgb(_frame_to_device(f, eng.device), th, tw) for f, (th, tw) in frames]
            return resolve

        out: List[ChatCompletion] = []
        with eng.lock:
            for idx, toks, recs, fins, timing in serve(range(len(futs)), resolver):
                if timing:
                    logger.debug("%s: %d request(s): prompt pass %.1f ms, %d decode steps in %.1f ms (device time)", model_id,
                                 len(idx), timing["prefill_ms"], timing["decode_steps"], timing["decode_ms"])
                for j, t, rec, fin in zip(idx, toks, recs, fins):
                    if isinstance(t, Exception):
                        if not lazy:
                            raise t
                        out.append(t)
                        continue
                    out.append(_completion(model_id, tok, n_ids[j], t, rec, fin, timing, n is not None))
        return out

    def _prepare_mllama(self, lm, messages):
        """messages -> (token ids, decoded uint8 RGB frame or None).  The JPEG is decoded on the host, the tile canvas is
        chosen on the host; bilinear resample / normalise / patchify and everything after run on the GPU."""
        import numpy as np
        from . import jpeg
        from .image_processing import decode_data_uri
        from .tokenizer import build_llama_chat_ids
        frames = []
        for url in _image_urls(messages):
            jc = jpeg.parse_data_uri(url) if jpeg.enabled() else None
            frames.append(jc if jc is not None else np.array(decode_data_uri(url), dtype=np.uint8))
        if len(frames) > 1:
            raise ValueError("the mllama backend takes one image per request (what the reference sends)")
        return build_llama_chat_ids(lm.tokenizer, messages, len(frames)), (frames[0] if frames else None)

    def _complete_mllama_many(self, lm, batch_of_messages, gen: dict, seed: Optional[int], serve, speculative=None,
                              prediction: Optional[str] = None) -> List[ChatCompletion]:
        """Requests with an image share ONE decode loop in groups of the engine's max_batch (MllamaEngine.generate_batch:
        per-request prompt pass, weights streamed once per generated token for the whole group); text-only requests
        (the agents' health check) take the single-sequence path.  ``gen`` / ``seed`` / ``serve``: the engine keywords, the
        call's seed and the chunked generate_batch of _complete_many.  ``speculative`` / ``prediction`` (VIS_AUDITOR_SPECULATIVE
        set, one request, no other switch - _complete_many has checked): the request goes through ``generate(.., speculative=)``
        with or without an image."""
        from concurrent.futures import Future
        eng, tok = lm.engine, lm.tokenizer
        from . import ingest
        k, n, on_stream = gen.get("logprobs"), gen.get("n"), gen.get("on_stream")
        one = {name: v for name, v in gen.items() if name != "n"}      # generate's keywords: one choice per call

        def completion(n_ids, t, rec=None, fin=None):
            return _completion(lm.model_id, tok, n_ids, t, rec, fin, dict(getattr(eng, "last_timing", {})), n is not None)

        futs = [ingest.then(m, lambda msgs: self._prepare_mllama(lm, msgs)) for m in batch_of_messages]
        if speculative is not None:
            ids, f = futs[0].result()
            with eng.lock:
                t = eng.generate(ids, _frame_to_device(f, eng.device) if f is not None else None, speculative=speculative,
                                 **_prediction_ids(lm, prediction), **one)
                _log_timing(lm.model_id, eng.last_timing)
                return [completion(len(ids), t, None, eng.last_finish[0])]
        if any(isinstance(m, Future) for m in batch_of_messages):
            # the batch seam (verify_many): every request carries an image; requests are resolved in order by the engine
            # while it already runs the earlier prompt passes; a failed request keeps its exception as its result
            out: list = []
            n_ids = {}

            def resolver(j):
                def resolve():
                    ids, f = futs[j].result()
                    n_ids[j] = len(ids)
                    return ids, (_frame_to_device(f, eng.device) if f is not None else None)
                return resolve

            with eng.lock:
                for idx, outs, recs, fins, _ in serve(range(len(futs)), resolver):
                    out.extend(t if isinstance(t, Exception) else completion(n_ids[j], t, r, f)
                               for j, t, r, f in zip(idx, outs, recs, fins))
            return out
        prepared = [f.result() for f in futs]
        toks_out: List[Optional[List[int]]] = [None] * len(prepared)
        recs: list = [None] * len(prepared)
        fins: list = [None] * len(prepared)
        with eng.lock:
            with_img = [i for i, (_, f) in enumerate(prepared) if f is not None]
            for grp, outs, lps, ends, _ in serve(with_img, lambda i: (prepared[i][0], _frame_to_device(prepared[i][1], eng.device))):
                for i, t, r, f in zip(grp, outs, lps, ends):
                    toks_out[i], recs[i], fins[i] = t, r, f
            for i, (ids, f) in enumerate(prepared):
                if f is not None:
                    continue
                if on_stream is not None:
                    on_stream.requests = [i]
                # text only (the health check): no batched step without an image - one pass per choice
                choices = [(eng.generate(ids, None, seed=(self.seed if seed is None else seed) + c, **one),
                            eng.last_logprobs[0] if k is not None else None, eng.last_finish[0]) for c in range(n or 1)]
                if n is None:
                    toks_out[i], recs[i], fins[i] = choices[0]
                else:
                    toks_out[i], fins[i] = [c[0] for c in choices], [c[2] for c in choices]
                    recs[i] = [c[1] for c in choices] if k is not None else None
        return [completion(len(ids), t, r, f) for (ids, _), t, r, f in zip(prepared, toks_out, recs, fins)]


_MOCK_REPLY: List[Optional[Any]] = [None]


def set_mock_reply(reply) -> None:
    """Reply (string, or callable messages -> string) of every ``CannedResponseClient`` built without one - i.e.
    of the clients the agents build under provider ``mock`` (None restores the default "OK")."""
    _MOCK_REPLY[0] = reply


class CannedResponseClient:
    """Mock backend (the reference declares ``use_mock_responses``, utils/config.py:191, but ships none):
    returns a fixed reply.  Used for the no-GPU plumbing configuration (BASELINE config 1) and by tests;
    it performs no model arithmetic and is never selected implicitly."""

    def __init__(self, reply: Optional[str] = None, **_ignored):
        self.reply = reply if reply is not None else (_MOCK_REPLY[0] if _MOCK_REPLY[0] is not None else "OK")
        self.calls: List[dict] = []
        self.chat = _Chat(self)

    def _complete(self, model, messages, temperature, max_tokens, speculative=None, prediction=None, **kwargs):
        kw = _request_keywords(kwargs)
        check_ban_keywords(kw.get("no_repeat_ngram_size"), kw.get("bad_words"), kw.get("min_tokens"), max_tokens,
                           kw.get("response_format"))
        if speculative is not None or prediction is not None:
            if prediction is not None and is_mllama_model(model) and not _auditor_speculative():
                raise ValueError("prediction (speculative decoding) is offered for Qwen2-VL / Qwen2.5-VL models only (an mllama "
                                 "model: with VIS_AUDITOR_SPECULATIVE=k set)")
            # whatever else ``create`` swallowed goes along, as before: check_exclusive names an unknown keyword as a conflict
            check_speculative_request(speculative, temperature, prediction=prediction,
                                      **{name: v for name, v in {**kw, **kwargs}.items() if name != "stream_options"})
        self.calls.append({"model": model, "messages": messages, "temperature": temperature, "max_tokens": max_tokens,
                           "response_format": kw.get("response_format"), "top_p": kw.get("top_p"), "seed": kw.get("seed")})
        given = {**kw, "speculative": speculative, "prediction": prediction}      # only the keywords that were given
        self.calls[-1].update({name: v for name, v in given.items()
                               if v is not None and name not in ("logprobs", "top_logprobs", "stream", "stream_options")})
        reply = self.reply(messages) if callable(self.reply) else self.reply
        done = ChatCompletion([_Choice(_Message(reply), index=i) for i in range(check_n(kw.get("n"), 64) or 1)], model=model or "")
        if kw.get("stream"):      # the reply as its chunk sequence: role, one content chunk, the finish chunk (and the usage, if asked for)
            from .stream import check_stream_options
            return _chunks_of(done, 0, check_stream_options(kw.get("stream_options"), True))
        return done


def make_client(provider: str, api_key: Optional[str] = None, **kwargs):
    """provider -> client object.  ``mi355x`` -> local engine; ``mock`` -> canned replies;
    ``huggingface`` -> the reference's own remote client (only if huggingface_hub is importable)."""
    if provider == LOCAL_PROVIDER:
        return LocalVLMClient(api_key=api_key, **kwargs)
    if provider == "mock":
        return CannedResponseClient(**kwargs)
    if provider == "huggingface":
        from huggingface_hub import InferenceClient
        return InferenceClient(api_key=api_key)
    raise ValueError(f"unknown provider {provider!r}")
