"""Generator of tests/golden/request_keywords.json: what reaches the engines, call by call.

Needs no GPU.  Two recording stand-in engines are registered with the client, one under a Qwen2-VL model id and one under an
mllama one; every call of CASES is made through ``chat.completions.create`` or ``complete_many`` of a LocalVLMClient with
text-only messages, and what is written down is every ``generate`` / ``generate_batch`` call the stand-in received: the
method, how many positional arguments, how many requests, and the FULL keyword dict - or, for a call the client refused, the
exception's type and message.  The same ``create`` calls go to a CannedResponseClient, whose ``calls[-1]`` is recorded.

How a value is written down (``plain``): ``on_stream`` is reduced to its presence; a compiled schema to its type and the shape
of its transition table; a tuple, a NamedTuple and a dict with keys that are not strings keep their type in a tagged form, so
that 5 and "5", a list and a tuple, 1 and 1.0 stay apart.  tests/test_request.py replays every case and compares the texts.

Usage:  python tests/golden/gen_request_keywords.py [--out FILE] [--commit HASH]
The JSON names the commit it was recorded at.  It pins the client's and the engines' way in: re-run it, on purpose, only when
a change is meant to alter what an engine is handed.
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "request_keywords.json")
QWEN, MLLAMA = "synthetic:tiny-recording", "synthetic:mllama-recording"
MSGS = [{"role": "user", "content": "is the weld seam closed?"}]
OTHER = [{"role": "system", "content": "answer briefly"}, {"role": "user", "content": [{"type": "text", "text": "and this one?"}]}]
SCHEMA = {"type": "json_schema", "json_schema": {"name": "verdict", "strict": True, "schema": {
    "type": "object", "properties": {"ok": {"type": "boolean"}, "defects": {"type": "array", "items": {"type": "string"}}},
    "required": ["ok", "defects"], "additionalProperties": False}}}
SPEC = {"method": "ngram", "num_speculative_tokens": 2, "prompt_lookup_max": 3}
PRED = {"type": "content", "content": "the seam is closed"}
AUD = {"VIS_AUDITOR_SPECULATIVE": "2"}
ALL_ON = dict(temperature=0.7, max_tokens=16, logprobs=True, top_logprobs=3, top_p=0.9, seed=7, frequency_penalty=0.5,
              presence_penalty=-1, repetition_penalty=1.05, stop=["END", "\n\n"], top_k=40, min_p=0.05,
              logit_bias={"5": -100, 7: 2.5}, n=2, no_repeat_ngram_size=3, bad_words=["As an AI", "x"], min_tokens=5)
ALL_ON_STREAMED = dict(temperature=0.7, max_tokens=16, response_format=SCHEMA, top_p=0.9, seed=7, frequency_penalty=0.5,
                       presence_penalty=-1, repetition_penalty=1.05, stop="END", top_k=40, min_p=0.05, logit_bias={5: -100},
                       n=2, stream=True, stream_options={"include_usage": True})

# name -> the call: ``kw`` its keywords; ``many``: through complete_many with that many requests (else create, one request);
# ``env``: the VIS_* variables set while it runs (every other VIS_* variable is unset).
CASES = {
    "plain": dict(kw={}),
    "plain_many": dict(kw={}, many=3),
    "plain_many_chunked": dict(kw={}, many=6),
    "temperature": dict(kw=dict(temperature=0.7)),
    "temperature_zero": dict(kw=dict(temperature=0)),
    "max_tokens": dict(kw=dict(max_tokens=16)),
    "logprobs": dict(kw=dict(logprobs=True)),
    "top_logprobs": dict(kw=dict(logprobs=True, top_logprobs=3)),
    "logprobs_off": dict(kw=dict(logprobs=False)),
    "top_p": dict(kw=dict(top_p=0.9)),
    "seed": dict(kw=dict(seed=7)),
    "seed_zero": dict(kw=dict(seed=0)),
    "frequency_penalty": dict(kw=dict(frequency_penalty=0.5)),
    "presence_penalty": dict(kw=dict(presence_penalty=-1)),
    "repetition_penalty": dict(kw=dict(repetition_penalty=1.05)),
    "stop_string": dict(kw=dict(stop="END")),
    "stop_list": dict(kw=dict(stop=["END", "\n\n"])),
    "top_k": dict(kw=dict(top_k=40)),
    "min_p": dict(kw=dict(min_p=0.05)),
    "logit_bias": dict(kw=dict(logit_bias={"5": -100, 7: 2.5})),
    "n": dict(kw=dict(n=2)),
    "no_repeat_ngram_size": dict(kw=dict(no_repeat_ngram_size=3)),
    "bad_words": dict(kw=dict(bad_words=["As an AI", "x"])),
    "min_tokens": dict(kw=dict(min_tokens=5)),
    "neutral_top_p": dict(kw=dict(top_p=1)),
    "neutral_penalties": dict(kw=dict(frequency_penalty=0, presence_penalty=0, repetition_penalty=1)),
    "neutral_top_k": dict(kw=dict(top_k=0)),      # top_k has no off value but None: refused
    "neutral_min_p": dict(kw=dict(min_p=0)),
    "neutral_logit_bias": dict(kw=dict(logit_bias={})),
    "neutral_n": dict(kw=dict(n=1)),
    "neutral_stop": dict(kw=dict(stop=[])),
    "neutral_bad_words": dict(kw=dict(bad_words=[])),
    "neutral_min_tokens": dict(kw=dict(min_tokens=0)),
    "neutral_no_repeat_ngram_size": dict(kw=dict(no_repeat_ngram_size=0)),
    "format_text": dict(kw=dict(response_format={"type": "text"})),
    "format_json_object": dict(kw=dict(response_format={"type": "json_object"})),
    "format_json_schema": dict(kw=dict(response_format=SCHEMA)),
    "seed_two_requests": dict(kw=dict(seed=7, temperature=0.5), many=2),
    "n_many": dict(kw=dict(n=2, temperature=0.5), many=3),
    "stream": dict(kw=dict(stream=True)),
    "stream_usage": dict(kw=dict(stream=True, stream_options={"include_usage": True})),
    "stream_off": dict(kw=dict(stream=False)),
    "stream_many": dict(kw=dict(stream=True, stop="END"), many=2),
    "speculative": dict(kw=dict(speculative=SPEC)),
    "prediction": dict(kw=dict(prediction=PRED)),
    "speculative_prediction": dict(kw=dict(speculative=SPEC, prediction=PRED, max_tokens=24)),
    "prediction_empty": dict(kw=dict(prediction={"type": "content", "content": ""}, top_p=0.9)),
    "speculative_auditor": dict(kw=dict(speculative=SPEC), env=AUD),
    "prediction_auditor": dict(kw=dict(prediction=PRED), env=AUD),
    "speculative_prediction_auditor": dict(kw=dict(speculative=SPEC, prediction=PRED), env=AUD),
    "speculative_with_top_p": dict(kw=dict(speculative=SPEC, top_p=0.9)),
    "speculative_with_neutrals": dict(kw=dict(speculative=SPEC, temperature=0.0, n=1, top_p=1, stop=[])),
    "prediction_many": dict(kw=dict(prediction=PRED), many=2),
    "speculative_many": dict(kw=dict(speculative=SPEC), many=2),
    "unknown_many": dict(kw=dict(best_of=2), many=2),
    "unknown_create": dict(kw=dict(user="line 3", max_completion_tokens=9, top_p=0.9)),
    "ignore_eos": dict(kw={}, env={"VIS_IGNORE_EOS": "1"}),
    "ignore_eos_many": dict(kw=dict(temperature=0.3), many=2, env={"VIS_IGNORE_EOS": "1"}),
    "bad_top_p": dict(kw=dict(top_p=1.5, logprobs=True, top_logprobs=99)),      # the first check that fails names the error
    "bad_ban_with_grammar": dict(kw=dict(min_tokens=2, response_format={"type": "json_object"})),
    "all_on": dict(kw=ALL_ON),
    "all_on_many": dict(kw=ALL_ON, many=3),
    "all_on_streamed": dict(kw=ALL_ON_STREAMED),
}
REPLY = [72, 105]


def plain(v, name=None):
    """``v`` as JSON that keeps its type apart (module docstring)."""
    if name == "on_stream":
        return v is not None
    if type(v).__name__ == "SchemaDFA":
        return {"__SchemaDFA__": [list(v.trans.shape), int(v.start)]}
    if isinstance(v, tuple):
        return {"__%s__" % type(v).__name__: [plain(x) for x in v]}
    if isinstance(v, list):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        if all(isinstance(k, str) for k in v):
            return {k: plain(x, k) for k, x in v.items()}
        return {"__items__": [[plain(k), plain(x)] for k, x in v.items()]}
    if isinstance(v, bytes):
        return {"__bytes__": v.hex()}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"{name}: no written form for a {type(v).__name__}")


class RecordingEngine:
    """Stands where an engine stands: takes what the client hands over, writes it down and returns a fixed reply in the shape
    the call asked for (nested with ``n``, a logprob record per reply with ``logprobs``)."""
    host_only = True      # the client's resolver hands the request's frames over as they are: nothing is uploaded

    def __init__(self, max_batch, max_ctx):
        self.max_batch, self.max_ctx, self.device, self.lock = max_batch, max_ctx, "cpu", threading.Lock()
        self.calls, self.last_timing, self.last_logprobs, self.last_finish = [], {}, None, None

    def _logprobs(self, k):
        import numpy as np
        from vision_inspection_system_amd.logprobs import TokenLogprobs
        n = len(REPLY)
        return TokenLogprobs(np.zeros(n, np.float32), np.zeros((n, k), np.int32), np.zeros((n, k), np.float32))

    def generate(self, *args, **kw):
        self.calls.append({"method": "generate", "positional": len(args), "kw": plain(kw)})
        self.last_finish = [("eos", None)]
        self.last_logprobs = [self._logprobs(kw["logprobs"])] if kw.get("logprobs") is not None else None
        self.last_timing = {"prompt_tokens": len(args[0]), "prefill_ms": 0.0, "decode_ms": 0.0, "decode_steps": 1, "sequences": 1}
        if kw.get("prediction"):
            self.last_timing.update(pred_accepted=1, pred_rejected=0)
        return list(REPLY)

    def generate_batch(self, *args, **kw):
        requests = [r() if callable(r) else r for r in args[0]]
        self.calls.append({"method": "generate_batch", "positional": len(args), "requests": len(requests), "kw": plain(kw)})
        n, k = kw.get("n"), kw.get("logprobs")
        nest = (lambda x: [x] * n) if n else (lambda x: x)
        self.last_finish = [nest(("eos", None)) for _ in requests]
        self.last_logprobs = [nest(self._logprobs(k)) for _ in requests] if k is not None else None
        self.last_timing = {}
        return [nest(list(REPLY)) for _ in requests]


@contextlib.contextmanager
def vis_env(env):
    """Only the VIS_* variables of ``env`` are set."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("VIS_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("VIS_")]:
            del os.environ[k]
        os.environ.update(saved)


@contextlib.contextmanager
def stand_ins():
    """The two recording engines, registered with the client: {model id: engine}."""
    from vision_inspection_system_amd import client as CL
    from vision_inspection_system_amd import mllama_weights as MW
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.tokenizer import ByteTokenizer, LlamaByteTokenizer
    qc, mc = Qwen2VLConfig.tiny(), MW.MllamaConfig.tiny()
    engines = {QWEN: RecordingEngine(4, 12), MLLAMA: RecordingEngine(4, 12)}
    CL.register_model(QWEN, "cpu", CL.LoadedModel(
        engines[QWEN], ByteTokenizer(qc.vocab, qc.image_token_id, qc.vision_start_id, qc.vision_end_id, qc.eos_ids), qc, QWEN))
    CL.register_model(MLLAMA, "cpu", CL.LoadedModel(
        engines[MLLAMA], LlamaByteTokenizer(mc.vocab, mc.image_token_id, mc.eos_ids), mc, MLLAMA, "mllama"))
    try:
        yield engines
    finally:
        CL.unregister_model(QWEN, "cpu")
        CL.unregister_model(MLLAMA, "cpu")


def _call(fn):
    """What a refused call raised, written down; None for one that went through."""
    try:
        out = fn()
        if not isinstance(out, list) and hasattr(out, "__next__"):
            for _ in out:      # a streamed call runs on a worker: the engine has been called once the chunks are through
                pass
        return None
    except Exception as e:      # noqa: BLE001 - the record names it
        # a TypeError's text is the interpreter's (it names the function's qualified name): its type is the record
        return {"type": type(e).__name__, "message": None if isinstance(e, TypeError) else str(e)}


def record(name, engines):
    """Case ``name`` through both stand-ins and the mock client: {"qwen": .., "mllama": .., "canned": ..}, each {"calls": [...],
    "error": None or {"type", "message"}}; "canned" only for a ``create`` case."""
    from vision_inspection_system_amd import client as CL
    case = CASES[name]
    kw, many = case["kw"], case.get("many")
    out = {}
    with vis_env(case.get("env", {})):
        for key, model in (("qwen", QWEN), ("mllama", MLLAMA)):
            eng, c = engines[model], CL.LocalVLMClient(device="cpu", seed=11)
            del eng.calls[:]
            if many:
                err = _call(lambda: c.complete_many(model, [MSGS, OTHER][:many] + [MSGS] * (many - 2), **kw))
            else:
                err = _call(lambda: c.chat.completions.create(model=model, messages=MSGS, **kw))
            out[key] = {"calls": list(eng.calls), "error": err}
        if not many:
            for key, model in (("canned", QWEN), ("canned_mllama", MLLAMA)):
                c = CL.CannedResponseClient("fine")
                err = _call(lambda: c.chat.completions.create(model=model, messages=MSGS, **kw))
                out[key] = {"calls": [plain(d) for d in c.calls], "error": err}
    return out


def text(recorded) -> str:
    """The form two records are compared in: JSON text with sorted keys (1 and 1.0 differ in it)."""
    return json.dumps(recorded, sort_keys=True, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="the commit the record is made at (default: git rev-parse HEAD)")
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    with stand_ins() as engines:
        cases = {name: record(name, engines) for name in CASES}
    with open(args.out, "w") as f:
        json.dump({"header": {"recorded_at_commit": commit,
                              "what": "engine keywords per client call, recorded on the CPU by tests/golden/gen_request_keywords.py"},
                   "cases": cases}, f, sort_keys=True, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
