"""Generator of tests/golden/engine_state.json: what an engine holds right after construction, configuration by configuration.

Needs an MI355X.  For every configuration of CONFIGS it builds a tiny engine (Qwen2VLConfig.tiny() / MllamaConfig.tiny(), the
seeded synthetic weights, max_ctx=256) and flattens ``vars(engine)``:
  * a tensor: one line ``<dtype> <shape> strides <strides> at <owner>+<byte offset> of <storage bytes>`` - where it lives is
    the attribute path that owns the storage (of the paths that share it the one with the most bytes, the alphabetically
    first among equals) and the byte offset in it;
  * a bool, int, float, str, None, torch.device or torch.dtype: its ``repr``;
  * a list, tuple or dict: its items under path names (``q8[0].down_w[1]``, ``slot_prompt_len[2]``), an empty one as
    ``list[0]`` / ``dict[0]``;
  * anything else (locks, streams, graphs, the pick stage's objects, layer weights): ``<TypeName>`` - that it exists, not what
    it holds.  ``cfg`` and ``w`` are skipped.
``alloc_bytes`` is what ``torch.cuda.memory_allocated()`` grew by over the construction (the weights exist before), for the
record only: the caching allocator hands out a cached block up to 1 MiB larger than asked for, so the figure depends on what
the process did before.  ``storage_bytes(state)`` - the bytes of the distinct storages a state names - does not.

Usage:  python tests/golden/gen_engine_state.py [--out FILE] [--commit HASH] [--only NAME ...]
The JSON names the commit it was recorded at.  Re-run it, on purpose, when a change is meant to alter what an engine
allocates; tests/test_engine_state_gpu.py compares every configuration against the file.
"""
import argparse
import gc
import json
import os
import re
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_decode_transcript as T  # noqa: E402

OUT = os.path.join(HERE, "engine_state.json")
SKIP = ("cfg", "w")


def _configs() -> dict:
    """The distinct (model, env, constructor keywords) of the decode transcript's configurations - a single-sequence one at
    max_batch 1, one of 3 sequences at 4, one of 6 at 6 - and the constructor keywords the transcript does not reach."""
    out, seen = {}, set()
    for name, c in T.CONFIGS.items():
        B = c.get("B", 1)
        kw = dict(c.get("engine", {}), max_batch=1 if B == 1 else 4 if B <= 4 else 6)
        key = (c["model"], tuple(sorted(c.get("env", {}).items())), tuple(sorted(kw.items())))
        if key not in seen:
            seen.add(key)
            out[name] = dict(model=c["model"], env=c.get("env", {}), engine=kw)
    out["qwen_prefill_fp8"] = dict(model="qwen", env={}, engine=dict(prefill_dtype="fp8", max_batch=1))
    out["qwen_b4_prefill_fp8"] = dict(model="qwen", env={}, engine=dict(prefill_dtype="fp8", max_batch=4))
    for B in (1, 4):
        tag = "single" if B == 1 else f"b{B}"
        out[f"mllama_{tag}_fp8"] = dict(model="mllama", env={}, engine=dict(decode_weights="fp8", max_batch=B))
        out[f"mllama_{tag}_mxfp4"] = dict(model="mllama", env={}, engine=dict(decode_weights="mxfp4", max_batch=B))
    out["mllama_b6_mxfp4_gemm5"] = dict(model="mllama", env={},
                                        engine=dict(decode_weights="mxfp4", mxfp4_gemm_from=5, max_batch=6))
    out["mllama_b4_fp8_fused_env"] = dict(model="mllama", env=T.FUSED, engine=dict(decode_weights="fp8", max_batch=4))
    out["mllama_b4_cross_kv_fp8"] = dict(model="mllama", env={}, engine=dict(cross_kv="fp8", max_batch=4))
    out["mllama_single_speculative"] = dict(model="mllama", env={}, engine=dict(speculative=True, max_batch=1))
    return out


CONFIGS = _configs()


def build(name: str, device):
    """The engine of configuration ``name`` and what its construction allocated."""
    c = CONFIGS[name]
    with T.vis_env(c["env"]):
        make = T._qwen if c["model"] == "qwen" else T._mllama
        if c["model"] == "qwen":      # T._qwen also hangs a tokenizer on: an object, recorded as its type
            make(device, max_batch=1)
        else:
            make(device)
        gc.collect()
        torch.cuda.synchronize(device)
        before = torch.cuda.memory_allocated(device)
        _, eng = make(device, **c["engine"])
        torch.cuda.synchronize(device)
        gc.collect()
        return eng, torch.cuda.memory_allocated(device) - before


def tensors_of(eng) -> dict:
    """path -> tensor for every tensor ``flatten`` names."""
    found = {}
    _walk(vars(eng), "", found, {})
    return found


def _walk(o, path: str, tensors: dict, plain: dict) -> None:
    if isinstance(o, torch.Tensor):
        tensors[path] = o
    elif o is None or isinstance(o, (bool, int, float, str, torch.device, torch.dtype)):
        plain[path] = repr(o)
    elif isinstance(o, dict):
        if not o:
            plain[path] = "dict[0]"
        for k, v in o.items():
            if not (path == "" and k in SKIP):
                _walk(v, f"{path}.{k}" if path else str(k), tensors, plain)
    elif isinstance(o, (list, tuple)):
        if not o:
            plain[path] = f"{type(o).__name__}[0]"
        for i, v in enumerate(o):
            _walk(v, f"{path}[{i}]", tensors, plain)
    else:
        plain[path] = f"<{type(o).__name__}>"


def flatten(eng) -> dict:
    tensors, plain = {}, {}
    _walk(vars(eng), "", tensors, plain)
    owner = {}
    for path in sorted(tensors):
        t = tensors[path]
        ptr, size = t.untyped_storage().data_ptr(), t.numel() * t.element_size()
        if ptr not in owner or size > owner[ptr][0]:
            owner[ptr] = (size, path)
    out = dict(plain)
    for path, t in tensors.items():
        s = t.untyped_storage()
        out[path] = (f"{str(t.dtype)[6:]} {list(t.shape)} strides {list(t.stride())} at {owner[s.data_ptr()][1]}"
                     f"+{t.storage_offset() * t.element_size()} of {s.nbytes()}")
    return dict(sorted(out.items()))


def storage_bytes(state: dict) -> int:
    """The bytes of the distinct storages the tensors of a flattened state live in."""
    owners = {}
    for v in state.values():
        m = re.search(r" at (.+)\+\d+ of (\d+)$", v)
        if m:
            owners[m.group(1)] = int(m.group(2))
    return sum(owners.values())


def record(name: str, device) -> dict:
    eng, alloc = build(name, device)
    return {"alloc_bytes": alloc, "state": flatten(eng)}


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
        print(f"{name}: {len(configs[name]['state'])} entries, {configs[name]['alloc_bytes']} bytes", flush=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_at": commit, "configs": configs}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
