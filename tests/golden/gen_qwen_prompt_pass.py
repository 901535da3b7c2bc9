"""Generator of tests/golden/qwen_prompt_pass.json: what the Inspector's prompt pass calls and what it leaves behind.

Needs an MI355X.  For every configuration of CONFIGS it builds the tiny engine (Qwen2VLConfig.tiny(), synth_state_dict(cfg, seed=0),
max_ctx=512, min_shared_prefix=64; the ``*_wide`` rows: the same with intermediate=8192, the smallest width at which the down
projection runs as two K-slices - every entry point accepted it, no wider shape was needed), runs the prompt pass through the
public surface alone (prefill, prefill_many, cached_prefix, generate, generate_batch, decode, generated) and writes down

  calls     the library calls, one list per issuing thread in the order the threads first appear (Recorder of
            gen_mllama_prompt_pass.py: arguments of kind i / f / l / u verbatim, pointers as ``ptr`` or ``None``).  Recorded are
            ``prefill(..., taps=)`` of the single configurations, ``prefill_many`` of the many configurations, and for the prefix
            configurations two whole ``generate(..., max_new_tokens=8)`` calls (the first computes the text prefix, the second
            finds it in the prefix cache; their 7 decode steps each are part of the list);
  digests   sha256 of the result bytes after torch.cuda.synchronize(): per used slot step, current token, logits, the cache rows
            of the prompt and the rope rows below the decode limit; single configurations: the taps image_embeds, layer0,
            first_logits; configurations with a text prefix: the bundle's k, v, vt and the prefix cache's hit count;
  tokens    single configurations on slot 0: the 8 greedy tokens after decode(7, use_graph=False) (prefix configurations: what
            the second generate returned); many configurations: 6 tokens per request of generate_batch(..., max_new_tokens=6,
            ignore_eos=True, use_graph=False), ``"error"`` for a lazy request that raised.

The requests are the frames and ids of tests/golden/qwen2vl_tiny.npz, the 150-text-token prompts of
tests/test_engine_gpu.py::test_shared_text_prefix_is_bit_identical (shared prefix 128) and its ``four`` list.  The JSON also holds one
digest of ``w.embed`` and ``w.patch_w`` of the tiny weights: a mismatch caused by another synthetic weight stream can be told from
a change of behaviour.

Usage:  python tests/golden/gen_qwen_prompt_pass.py [--out FILE] [--commit HASH] [--only NAME ...]
The JSON names the commit it was recorded at.  tests/test_qwen_prompt_pass_gpu.py compares every configuration against it.
"""
import argparse
import dataclasses
import functools
import hashlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from gen_decode_transcript import _qwen, _qwen_requests, first_difference  # noqa: E402,F401  (first_difference: for the test)
from gen_mllama_prompt_pass import recording, sha, vis_env  # noqa: E402

OUT = os.path.join(HERE, "qwen_prompt_pass.json")
TEXT_IDS = [256, 72, 105, 33, 90, 41]
FP8 = dict(prefill_dtype="fp8", decode_weights="fp8")
B4 = dict(max_batch=4)

# name -> run: "single" = prefill(ids, frames, slot=slot, taps=...), "prefix" = generate(ids, frames, max_new_tokens=8) twice,
# "many" = prefill_many(requests); requests: "a" / "b" = ids_a + frame_a / ids_b + frame_b1, frame_b2 of the npz, "text" = no image,
# "shared3" = the three prompts behind 150 common text tokens, "four" / "five" = same-structure prompts behind that text,
# "lazy" = shared3 as callables, the second raising; wide: intermediate=8192; env: the VIS_* switches (every other one is unset).
CONFIGS = {
    "single_image": dict(run="single", requests="a"),
    "single_two_images": dict(run="single", requests="b"),
    "single_text": dict(run="single", requests="text"),
    "single_slot1": dict(run="single", requests="a", slot=1, engine=B4),
    "single_fp8": dict(run="single", requests="a", engine=FP8),
    "single_pairs_off": dict(run="single", requests="a", env={"VIS_ATTN_PAIRS": "0"}),
    "single_prefix_pairs_off": dict(run="prefix", requests="shared3", env={"VIS_ATTN_PAIRS": "0"}),
    "single_prefix": dict(run="prefix", requests="shared3"),
    "single_prefix_fp8": dict(run="prefix", requests="shared3", engine=FP8),
    "many_1": dict(run="many", requests="a"),
    "many_3_shared": dict(run="many", requests="shared3", engine=B4),
    "many_3_shared_fp8": dict(run="many", requests="shared3", engine=dict(B4, **FP8)),
    "many_4_stacked": dict(run="many", requests="four", engine=B4),
    "many_4_stacked_fp8": dict(run="many", requests="four", engine=dict(B4, **FP8)),
    "many_4_group_attn_off": dict(run="many", requests="four", engine=B4, env={"VIS_GROUP_ATTN": "0"}),
    "many_4_merge_off": dict(run="many", requests="four", engine=B4, env={"VIS_MERGE_PREFILL": "0"}),
    "many_5_vit_batch_8": dict(run="many", requests="five", engine=dict(max_batch=8), env={"VIS_VIT_BATCH": "8"}),
    "many_2_no_prefix": dict(run="many", requests="ab", engine=B4),
    "many_3_one_stream": dict(run="many", requests="shared3", engine=B4, env={"VIS_PREFILL_STREAMS": "1"}),
    "many_lazy_error": dict(run="many", requests="lazy", engine=B4),
    "single_wide": dict(run="single", requests="a", wide=True),
    "single_wide_fp8": dict(run="single", requests="a", wide=True, engine=FP8),
    "many_4_wide": dict(run="many", requests="four", wide=True, engine=B4),
    "many_4_wide_fp8": dict(run="many", requests="four", wide=True, engine=dict(B4, **FP8)),
}


def _engine(device, c: dict):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    cfg = dataclasses.replace(Qwen2VLConfig.tiny(), intermediate=8192) if c.get("wide") else None
    cfg, eng = _qwen(device, cfg=cfg, max_ctx=512, **c.get("engine", {}))
    eng.min_shared_prefix = 64
    return cfg, eng


@functools.lru_cache(maxsize=None)
def weight_digest(device) -> str:
    _, eng = _engine(device, {})
    return hashlib.sha256((sha(eng.w.embed) + sha(eng.w.patch_w)).encode()).hexdigest()


def _lazy_error():
    raise ValueError("this image does not decode")


def _requests(cfg, device, which: str) -> list:
    if which == "text":
        return [(list(TEXT_IDS), [])]
    if which in ("a", "b", "ab"):
        a, b = _qwen_requests(cfg, device, 2, False)
        return {"a": [a], "b": [b], "ab": [a, b]}[which]
    shared3 = _qwen_requests(cfg, device, 3, True)
    if which == "shared3":
        return shared3
    if which == "lazy":
        return [lambda: shared3[0], _lazy_error, lambda: shared3[2]]
    ids, frames = shared3[0]                              # text + image a + [7, 8, 9]
    tails = [[7, 8, 9], [9, 9, 9], [1, 2, 3], [7, 8, 9], [4, 5, 6]][:{"four": 4, "five": 5}[which]]
    return [(ids[:-3] + t, frames) for t in tails]


def _slot_digests(eng, slot: int, S: int, limit: int) -> dict:
    return {"step": sha(eng.step_b[slot]), "cur": sha(eng.cur_b[slot]), "logits": sha(eng.logits_b[slot]),
            "kcache": sha(eng.kcache_b[slot][:, :, :S]), "vcache": sha(eng.vcache_b[slot][:, :, :S]),
            "cos": sha(eng.cos_b[slot][:limit]), "sin": sha(eng.sin_b[slot][:limit])}


def _prefix_digests(eng, ids, P: int) -> dict:
    """The bundle of ``ids[:P]`` as the prefix cache holds it (asking for it is one more hit, never a pass)."""
    hits = eng.prefix_cache_hits
    bundle = eng.cached_prefix(ids, P)
    if eng.prefix_cache_hits != hits + 1:
        raise RuntimeError("the text prefix was not in the prefix cache")
    return {"len": int(bundle["len"]), "hits": hits, "k": sha(bundle["k"]), "v": sha(bundle["v"]), "vt": sha(bundle["vt"])}


def record(name: str, device) -> dict:
    """Run configuration ``name`` and return {"calls": [[...] per thread], "digests": {...}, "tokens": ...}."""
    c = CONFIGS[name]
    with vis_env(c.get("env", {})), recording() as rec:
        cfg, eng = _engine(device, c)
        reqs = _requests(cfg, device, c["requests"])
        digests, tokens = {}, None
        if c["run"] == "single":
            (ids, frames), slot, taps = reqs[0], c.get("slot", 0), {}
            rec.armed = True
            eng.prefill(ids, frames, slot=slot, taps=taps)
            rec.armed = False
            torch.cuda.synchronize(device)
            digests[f"slot{slot}"] = _slot_digests(eng, slot, len(ids), eng.max_ctx)
            digests["taps"] = {k: sha(taps[k]) for k in ("image_embeds", "layer0", "first_logits") if k in taps}
            if slot == 0:
                digests["decode_limit"] = eng.decode_limit
                eng.decode(7, use_graph=False)
                tokens = eng.generated(8)
        elif c["run"] == "prefix":
            ids, frames = reqs[0]
            rec.armed = True
            first = eng.generate(ids, frames, max_new_tokens=8, ignore_eos=True, use_graph=False)
            tokens = eng.generate(ids, frames, max_new_tokens=8, ignore_eos=True, use_graph=False)
            rec.armed = False
            torch.cuda.synchronize(device)
            if first != tokens:
                raise RuntimeError(f"{name}: the pass behind the cached prefix gave {tokens}, the first one {first}")
            digests["decode_limit"] = eng.decode_limit
            digests["slot0"] = _slot_digests(eng, 0, len(ids), eng.decode_limit)
            digests["prefix"] = _prefix_digests(eng, ids, eng.text_prefix_len(ids))
        else:
            rec.armed = True
            slots, errors = eng.prefill_many(reqs)
            rec.armed = False
            torch.cuda.synchronize(device)
            live = [r() if callable(r) else r for r, e in zip(reqs, errors) if e is None]
            want_errors = [r is _lazy_error for r in reqs]
            if [s for s in slots if s is not None] != list(range(len(live))) or [e is not None for e in errors] != want_errors:
                raise RuntimeError(f"{name}: prefill_many gave slots {slots}, errors {errors}")
            digests["slots"] = slots
            for slot, (ids, _) in enumerate(live):
                digests[f"slot{slot}"] = _slot_digests(eng, slot, len(ids), eng.max_ctx)
            digests["batch_shared_len"] = eng.batch_shared_len
            P = eng.shared_prefix_len([ids for ids, _ in live])
            if P:
                digests["prefix"] = _prefix_digests(eng, live[0][0], P)
            out = eng.generate_batch(reqs, max_new_tokens=6, ignore_eos=True, use_graph=False)
            if [isinstance(t, Exception) for t in out] != want_errors:
                raise RuntimeError(f"{name}: generate_batch returned {out}")
            tokens = ["error" if isinstance(t, Exception) else t for t in out]
        torch.cuda.synchronize(device)
        eng.check_chain()
        return {"calls": list(rec.calls.values()), "digests": digests, "tokens": tokens}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="the commit this tree is (default: git rev-parse HEAD)")
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    device = torch.device("cuda:0")
    configs = {}
    for name in (args.only or CONFIGS):
        configs[name] = record(name, device)
        print(f"{name}: {[len(t) for t in configs[name]['calls']]} calls, tokens {configs[name]['tokens']}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_at": commit, "weights": weight_digest(device), "configs": configs}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
