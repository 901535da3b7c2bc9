"""Generator of tests/golden/generate_replies.json: what ``generate`` / ``generate_batch`` of both engines return, case by case.

Needs an MI355X.  It builds one tiny engine per model (Qwen2VLConfig.tiny() / MllamaConfig.tiny(), the seeded synthetic
weights, max_ctx=256, max_batch=4, the byte tokenizers, the prompts and frames of tests/golden/*.npz) and runs the cases of
CASES through the engines' PUBLIC methods only, so the same script runs at any commit.  Every case generates 12 tokens with
the host poll every 4 (``check_every`` / ``chunk``): three chunk boundaries, the smallest run in which the poll matters.

Recorded per case: the returned tokens (an exception as {"error": its type's name}), ``last_finish``, the logprob tokens
and values where logprobs are on, ``last_timing["decode_steps"]`` and ``last_timing["sequences"]``.  The stop string of the
"stop" case is cut out of the model's own greedy reply (the bytes of two tokens from the sixth on, so the match ends in the
second chunk) and written into the file; a rerun takes it from there.

Usage:  python tests/golden/gen_generate_replies.py [--out FILE] [--commit HASH]
The JSON names the commit it was recorded at.  It was recorded in front of a change that moved the generation loops and
must not be re-recorded to make such a change pass: the replies of these calls are the behaviour that change keeps.
tests/test_generate_replies_gpu.py rebuilds every case and compares - everything exactly, the logprob values within the
tolerance tests/test_logprobs_gpu.py uses for them.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "generate_replies.json")
N_NEW, EVERY = 12, 4
TEXT_ONLY = [1, 5, 6, 7, 8, 9]


# ----------------------------------------------------------------------------- engines and requests
def qwen(device):
    """(engine, [request A, request B]) of the tiny Qwen2-VL."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=4)
    eng.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    g = np.load(os.path.join(HERE, "qwen2vl_tiny.npz"))
    fa, fb1, fb2 = (torch.from_numpy(g[k]).to(device) for k in ("frame_a", "frame_b1", "frame_b2"))
    return eng, [(g["ids_a"].tolist(), [fa]), (g["ids_b"].tolist(), [fb1, fb2])]


def mllama(device):
    """(engine, [request a, b, c]) of the tiny Mllama."""
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=4)
    eng.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
    g = np.load(os.path.join(HERE, "mllama_tiny.npz"))
    return eng, [(g[f"{c}_ids"].tolist(), torch.from_numpy(g[f"{c}_image"]).to(device)) for c in "abc"]


MODELS = {"qwen": qwen, "mllama": mllama}


def spelling(model: str, ignore_eos: bool = False) -> dict:
    """The poll interval and the EOS switch as each engine's public methods spell them."""
    if model == "qwen":
        return dict(check_every=EVERY, ignore_eos=ignore_eos)
    return dict(chunk=EVERY, stop_on_eos=not ignore_eos)


def _boom():
    raise ValueError("this request's image could not be decoded")


# name -> (models it runs on, method, how its arguments are built from (model, requests, stop))
def _three(reqs):
    return [reqs[i % len(reqs)] for i in range(3)]


CASES = {
    "greedy": ("qwen mllama", "generate", lambda m, r, stop: (r[0], dict(spelling(m)))),
    "sampled_top_p": ("qwen mllama", "generate",
                      lambda m, r, stop: (r[0], dict(spelling(m), temperature=0.7, seed=5, top_p=0.9))),
    "stop": ("qwen mllama", "generate", lambda m, r, stop: (r[0], dict(spelling(m), stop=[stop]))),
    "logprobs": ("qwen mllama", "generate", lambda m, r, stop: (r[0], dict(spelling(m), logprobs=2))),
    "ignore_eos": ("qwen mllama", "generate", lambda m, r, stop: (r[0], dict(spelling(m, True)))),
    "batch3": ("qwen mllama", "generate_batch", lambda m, r, stop: ((_three(r),), dict(spelling(m)))),
    "batch3_lazy_middle_raises": ("qwen mllama", "generate_batch", lambda m, r, stop: (
        ([lambda: r[0], _boom, lambda: r[1]],), dict(spelling(m)))),
    "batch2_n2_seeds": ("qwen mllama", "generate_batch", lambda m, r, stop: (
        (r[:2],), dict(spelling(m), temperature=0.7, n=2, seeds=[11, 22]))),
    "batch1_n1": ("qwen mllama", "generate_batch", lambda m, r, stop: ((r[:1],), dict(spelling(m), n=1))),
    "text_only": ("mllama", "generate", lambda m, r, stop: ((TEXT_ONLY, None), dict(spelling(m)))),
    # 240 prompt tokens in a context of 256: room for 15 new ones, 40 asked for
    "beyond_context": ("qwen", "generate", lambda m, r, stop: (
        (np.random.default_rng(9).integers(3, 200, 240).tolist(), ()), dict(spelling(m), max_new_tokens=40))),
}


def cases_of(model: str) -> list:
    return [name for name, (models, _, _) in CASES.items() if model in models.split()]


# ----------------------------------------------------------------------------- one case
def _plain(x):
    """Tokens, finish tuples and exceptions as JSON holds them."""
    if isinstance(x, Exception):
        return {"error": type(x).__name__}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def _logprobs(rec):
    if rec is None or isinstance(rec, list):
        return None if rec is None else [_logprobs(r) for r in rec]
    return {"token_logprobs": rec.token_logprobs.astype(np.float64).tolist(), "top_ids": rec.top_ids.tolist(),
            "top_logprobs": rec.top_logprobs.astype(np.float64).tolist()}


def stop_string(eng, toks: list) -> list:
    """The bytes (as integers) of the first two tokens with any bytes from the sixth token of ``toks`` on."""
    eos = set(eng.cfg.eos_ids)
    tb = [b"" if t in eos else eng.tokenizer.token_bytes(t) for t in toks]
    have = [b for b in tb[5:] if b]
    if len(have) < 2:
        raise RuntimeError(f"no stop string in the second chunk of this reply: {tb}")
    return list(have[0] + have[1])


def run_case(model: str, name: str, eng, reqs, stop: bytes) -> dict:
    """Run case ``name`` on ``eng`` and return what is recorded of it."""
    _, method, build = CASES[name]
    args, kw = build(model, reqs, stop)
    kw.setdefault("max_new_tokens", N_NEW)
    try:
        out = getattr(eng, method)(*args, **kw)
    except Exception as e:      # noqa: BLE001 - a case that raises records the type
        return {"raised": type(e).__name__}
    return {"tokens": _plain(out), "finish": _plain(eng.last_finish),
            "logprobs": _logprobs(eng.last_logprobs) if kw.get("logprobs") is not None else None,
            "decode_steps": eng.last_timing["decode_steps"], "sequences": eng.last_timing["sequences"]}


def record(model: str, device, stop=None) -> dict:
    """{"stop": [...], "cases": {name: ...}} of one model; ``stop`` None: cut it out of the greedy ignore-EOS reply."""
    eng, reqs = MODELS[model](device)
    if stop is None:
        stop = stop_string(eng, run_case(model, "ignore_eos", eng, reqs, b"")["tokens"])
    return {"stop": list(stop), "cases": {name: run_case(model, name, eng, reqs, bytes(stop)) for name in cases_of(model)}}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="the commit this tree is (default: git rev-parse HEAD)")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    device = torch.device("cuda:0")
    models = {}
    for model in MODELS:
        models[model] = record(model, device)
        for name, c in models[model]["cases"].items():
            print(f"{model} {name}: {json.dumps({k: v for k, v in c.items() if k != 'logprobs'})}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_at": commit, "models": models}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
