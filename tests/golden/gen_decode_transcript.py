"""Generator of tests/golden/decode_transcript.json: the library calls of the decode step, configuration by configuration.

Needs an MI355X.  For every configuration of CONFIGS it builds a tiny engine (Qwen2VLConfig.tiny() / MllamaConfig.tiny(),
the seeded synthetic weights, max_ctx=256, the prompts and frames of tests/golden/*.npz), runs the prompt pass, and records
what two consecutive EAGER decode steps call in libvis_hip.so: the entry's name and its arguments, in order.  Nothing else
is recorded - not the prompt pass, not the polling between steps.

How a call is written down, so that the transcript is the same on every machine and in every process:
  * ``hip._lib`` is replaced by a proxy while a configuration runs (``hip.load()`` returns the module-level object once it
    is set); the proxy forwards every entry and, while armed, appends ``name(arg, arg, ...)`` to a list;
  * right before a step is recorded, every CUDA tensor reachable from the engine (its attributes, the weights, lists,
    dicts, objects with a ``__dict__`` such as the pick stage's buffers) is found and its storage's address range noted;
  * an integer argument inside one of those ranges is written ``a<k>+<byte offset>``, ``k`` numbering the storages in the
    order in which the transcript first names them; any other integer or float is its ``repr``, ``None`` is ``None``;
  * the steps run on the default stream, so the stream argument is 0;
  * an integer above 2^40 inside no range (a pointer to memory the engine does not own) is an error, never a constant.

The single-sequence Qwen2-VL and Mllama tiny shapes pass the chained layer head's support check, so the default
single-sequence configurations record the chained step (``"chained": true`` in the JSON says so per configuration).

Usage:  python tests/golden/gen_decode_transcript.py [--out FILE] [--commit HASH] [--only NAME ...]
The JSON names the commit it was recorded at.  Re-run it, on purpose, when a change is meant to alter the decode step's
launches; tests/test_decode_transcript_gpu.py compares every configuration against the file.
"""
import argparse
import bisect
import contextlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "decode_transcript.json")
FUSED = {"VIS_DECODE_FUSED": "1"}
STREAMK = {"VIS_DECODE_PROJ_FORM": "streamk"}

# name -> what to build and run.  model: qwen / mllama; env: the VIS_* switches of this configuration (every other VIS_*
# variable is unset while it runs); engine: constructor arguments besides max_ctx=256; run:
#   decode     prefill, then eng.decode(2, use_graph=False)                                   (single sequence)
#   steps      prefill_many of B requests, then eng._decode_step_batched(B) twice             (Qwen2-VL batched)
#   generate   generate_batch(B requests, use_graph=False), its first two batched steps       (Mllama batched; pick switches)
CONFIGS = {
    "qwen_single_bf16": dict(model="qwen", run="decode"),
    "qwen_single_bf16_unchained": dict(model="qwen", run="decode", env={"VIS_DECODE_CHAIN": "0"}),
    "qwen_single_fp8": dict(model="qwen", run="decode", engine=dict(decode_weights="fp8")),
    "qwen_single_mxfp4": dict(model="qwen", run="decode", engine=dict(decode_weights="mxfp4")),
    "qwen_b3_streamk_fold1": dict(model="qwen", run="steps", B=3, env={"VIS_QKV_FOLD": "1"}),
    "qwen_b3_streamk_fold0": dict(model="qwen", run="steps", B=3, env={"VIS_QKV_FOLD": "0"}),
    "qwen_b2_rows_gemv": dict(model="qwen", run="steps", B=2, env={"VIS_ROWS_GEMV": "4"}),
    "qwen_b3_fp8_fold1": dict(model="qwen", run="steps", B=3, env={"VIS_QKV_FOLD": "1"}, engine=dict(decode_weights="fp8")),
    "qwen_b3_fp8_fold0": dict(model="qwen", run="steps", B=3, env={"VIS_QKV_FOLD": "0"}, engine=dict(decode_weights="fp8")),
    "qwen_b3_fused": dict(model="qwen", run="steps", B=3, env=FUSED, projections_only=True),
    "qwen_b3_fused_down_pair": dict(model="qwen", run="steps", B=3, env={**FUSED, **STREAMK}, projections_only=True),
    "qwen_b3_fused_streamk_no_pair": dict(model="qwen", run="steps", B=3, env={**FUSED, **STREAMK, "VIS_DOWN_PAIR": "0"},
                                          projections_only=True),
    "qwen_b3_fused_fp8": dict(model="qwen", run="steps", B=3, env=FUSED, engine=dict(decode_weights="fp8"),
                              projections_only=True),
    "qwen_b6_mxfp4": dict(model="qwen", run="steps", B=6, engine=dict(decode_weights="mxfp4")),
    "qwen_b6_mxfp4_gemm5_fold1": dict(model="qwen", run="steps", B=6, env={"VIS_QKV_FOLD": "1"},
                                      engine=dict(decode_weights="mxfp4", mxfp4_gemm_from=5)),
    "qwen_b6_mxfp4_gemm5_fold0": dict(model="qwen", run="steps", B=6, env={"VIS_QKV_FOLD": "0"},
                                      engine=dict(decode_weights="mxfp4", mxfp4_gemm_from=5)),
    "qwen_b3_shared_prefix": dict(model="qwen", run="steps", B=3, shared_prefix=True),
    "qwen_b3_logprobs_stop": dict(model="qwen", run="generate", B=3, request=dict(logprobs=2, stop="\x02\x03\x04")),
    "mllama_single": dict(model="mllama", run="decode"),
    "mllama_single_unchained": dict(model="mllama", run="decode", env={"VIS_DECODE_CHAIN": "0"}),
    "mllama_single_text_only": dict(model="mllama", run="decode", text_only=True),
    "mllama_b3_streamk_fold1": dict(model="mllama", run="generate", B=3, env={"VIS_QKV_FOLD": "1"}),
    "mllama_b3_streamk_fold0": dict(model="mllama", run="generate", B=3, env={"VIS_QKV_FOLD": "0"}),
    "mllama_b3_fused": dict(model="mllama", run="generate", B=3, env=FUSED),
    "mllama_b3_fused_streamk": dict(model="mllama", run="generate", B=3, env={**FUSED, **STREAMK}),
}


# ----------------------------------------------------------------------------- the recorder
def cuda_storages(root) -> list:
    """Sorted, disjoint [start, end) address ranges of the storages of every CUDA tensor reachable from ``root``."""
    seen, ranges, stack = set(), {}, [root]
    while stack:
        o = stack.pop()
        if id(o) in seen or o is None or isinstance(o, (str, bytes, int, float, bool, np.ndarray, type, types.ModuleType,
                                                         types.FunctionType, types.MethodType)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                s = o.untyped_storage()
                if s.nbytes():
                    ranges[s.data_ptr()] = max(ranges.get(s.data_ptr(), 0), s.data_ptr() + s.nbytes())
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set, frozenset)):
            stack.extend(o)
        elif hasattr(o, "__dict__"):
            stack.extend(vars(o).values())
    return sorted(ranges.items())


class Recorder:
    """Stands in for ``hip._lib``: forwards every entry point; while armed, writes the call down first."""

    def __init__(self, real):
        self._real = real
        self.calls: list = []
        self._armed = False
        self._starts: list = []
        self._ranges: list = []
        self._names: dict = {}

    def __getattr__(self, name):
        entry = getattr(self._real, name)

        def call(*args):
            if self._armed:
                self.calls.append(f"{name}({', '.join(self.render(a, name) for a in args)})")
            return entry(*args)
        return call

    def render(self, a, where: str = "") -> str:
        if a is None:
            return "None"
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, bool) or not isinstance(a, int):
            raise TypeError(f"{where}: argument {a!r} of type {type(a).__name__} has no machine-independent form")
        i = bisect.bisect_right(self._starts, a) - 1
        if i >= 0 and a < self._ranges[i][1]:
            start = self._ranges[i][0]
            k = self._names.setdefault(start, len(self._names))
            return f"a{k}+{a - start}"
        if a > 1 << 40:
            raise ValueError(f"{where}: {a:#x} looks like a pointer but lies in no storage reachable from the engine")
        return repr(a)

    @contextlib.contextmanager
    def armed(self, eng):
        """Record the library calls made inside; the storages are looked up now (the pick switches allocate lazily)."""
        for start, end in cuda_storages(eng):
            i = bisect.bisect_left(self._starts, start)
            if i < len(self._starts) and self._starts[i] == start:
                self._ranges[i] = (start, max(end, self._ranges[i][1]))
            else:
                self._starts.insert(i, start)
                self._ranges.insert(i, (start, end))
        self._armed = True
        try:
            yield
        finally:
            self._armed = False

    def arm_method(self, eng, name: str, times: int = 2) -> None:
        """Instance-level wrapper: the first ``times`` calls of ``eng.<name>`` are recorded."""
        real, left = getattr(eng, name), [times]

        def wrapper(*a, **kw):
            if left[0] <= 0:
                return real(*a, **kw)
            left[0] -= 1
            with self.armed(eng):
                return real(*a, **kw)
        setattr(eng, name, wrapper)


@contextlib.contextmanager
def recording():
    """``hip._lib`` replaced by a Recorder for the duration."""
    from vision_inspection_system_amd import hip
    real = hip.load()
    rec = Recorder(real)
    hip._lib = rec
    try:
        yield rec
    finally:
        hip._lib = real


@contextlib.contextmanager
def vis_env(env: dict):
    """Exactly the VIS_* variables of ``env`` set, every other one unset, for the duration."""
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


# ----------------------------------------------------------------------------- engines and requests
_WEIGHTS: dict = {}


def _qwen(device, cfg=None, max_ctx: int = 256, **kw):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = cfg or Qwen2VLConfig.tiny()
    if ("qwen", cfg, str(device)) not in _WEIGHTS:
        _WEIGHTS[("qwen", cfg, str(device))] = pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)
    eng = Qwen2VLEngine(cfg, _WEIGHTS[("qwen", cfg, str(device))], device, max_ctx=max_ctx, **kw)
    eng.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    return cfg, eng


def _mllama(device, **kw):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    cfg = MllamaConfig.tiny()
    if ("mllama", str(device)) not in _WEIGHTS:
        _WEIGHTS[("mllama", str(device))] = pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)
    return cfg, MllamaEngine(cfg, _WEIGHTS[("mllama", str(device))], device, max_ctx=256, **kw)


def _qwen_requests(cfg, device, n: int, shared_prefix: bool) -> list:
    g = np.load(os.path.join(HERE, "qwen2vl_tiny.npz"))
    fa, fb1, fb2 = (torch.from_numpy(g[k]).to(device) for k in ("frame_a", "frame_b1", "frame_b2"))
    if shared_prefix:      # the requests of tests/test_engine_gpu.py::test_shared_text_prefix_is_bit_identical
        text = np.random.default_rng(5).integers(3, 200, 150).tolist()

        def ids_for(f, tail):
            n_img = (f.shape[0] // cfg.patch) * (f.shape[1] // cfg.patch) // cfg.merge ** 2
            return text + [cfg.vision_start_id] + [cfg.image_token_id] * n_img + [cfg.vision_end_id] + tail
        reqs = [(ids_for(fa, [7, 8, 9]), [fa]), (ids_for(fb1, [11]), [fb1]), (ids_for(fa, [7, 8, 9]), [fa])]
    else:
        reqs = [(g["ids_a"].tolist(), [fa]), (g["ids_b"].tolist(), [fb1, fb2])]
    return [reqs[i % len(reqs)] for i in range(n)]


def _mllama_requests(device, n: int) -> list:
    g = np.load(os.path.join(HERE, "mllama_tiny.npz"))
    reqs = [(g[f"{c}_ids"].tolist(), torch.from_numpy(g[f"{c}_image"]).to(device)) for c in "abc"]
    return [reqs[i % len(reqs)] for i in range(n)]


# ----------------------------------------------------------------------------- one configuration
def record(name: str, device) -> dict:
    """Run configuration ``name`` and return {"chained": ..., "calls": [...]}."""
    c = CONFIGS[name]
    B = c.get("B", 1)
    with vis_env(c.get("env", {})), recording() as rec:
        kw = dict(c.get("engine", {}))
        if B > 1:
            kw["max_batch"] = 8 if c["model"] == "qwen" else 4
        if c["model"] == "qwen":
            cfg, eng = _qwen(device, **kw)
            reqs = _qwen_requests(cfg, device, B, c.get("shared_prefix", False))
            if c.get("shared_prefix"):
                eng.min_shared_prefix = 64
        else:
            cfg, eng = _mllama(device, **kw)
            reqs = _mllama_requests(device, B)
        if c["run"] == "decode":
            if c.get("text_only"):
                eng.prefill([1, 5, 6, 7, 8, 9], None)
            else:
                eng.prefill(*reqs[0])
            with rec.armed(eng):
                eng.decode(2, use_graph=False)
        elif c["run"] == "steps":
            slots, errors = eng.prefill_many(reqs)
            if slots != list(range(B)) or any(errors):
                raise RuntimeError(f"{name}: prefill_many gave slots {slots}, errors {errors}")
            if c.get("shared_prefix") and eng.batch_shared_len != 128:
                raise RuntimeError(f"{name}: batch_shared_len is {eng.batch_shared_len}, not 128")
            for _ in range(2):
                with rec.armed(eng):
                    eng._decode_step_batched(B)
            if c.get("projections_only"):      # what bench.py replays: the weight-streaming launches alone
                with rec.armed(eng):
                    n = eng._decode_step_fused(B, projections_only=True)
                rec.calls.append(f"-> {n!r}")
        else:
            gen = dict(max_new_tokens=4, use_graph=False, **c.get("request", {}))
            gen.update(dict(ignore_eos=True) if c["model"] == "qwen" else dict(stop_on_eos=False))
            if c.get("request"):
                eng.generate_batch(reqs, **gen)      # a throw-away request: the pick switches allocate on first use
            rec.arm_method(eng, "_decode_step_batched")
            out = eng.generate_batch(reqs, **gen)
            if any(isinstance(o, Exception) for o in out):
                raise RuntimeError(f"{name}: generate_batch returned {out}")
        torch.cuda.synchronize(device)
        eng.check_chain()
        return {"chained": eng.chain_sync is not None and c["run"] == "decode", "calls": rec.calls}


def first_difference(got: list, want: list) -> str:
    """'' when the two call lists are equal, else a sentence naming the first call that differs."""
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"call {i} differs:\n  recorded now: {a}\n  golden:       {b}"
    if len(got) != len(want):
        extra = (got if len(got) > len(want) else want)[min(len(got), len(want))]
        return f"{len(got)} calls recorded now, {len(want)} in the golden; the first one without a partner: {extra}"
    return ""


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
        print(f"{name}: {len(configs[name]['calls'])} calls, chained={configs[name]['chained']}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_at": commit, "configs": configs}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
