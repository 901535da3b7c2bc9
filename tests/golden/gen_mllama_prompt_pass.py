"""Generator of tests/golden/mllama_prompt_pass.json: what the Auditor's prompt pass calls and what it leaves behind.

Needs an MI355X.  For every configuration of CONFIGS it builds the tiny engine (MllamaConfig.tiny(), synth_state_dict(cfg, seed=0),
max_ctx=256, the images and ids of tests/golden/mllama_tiny.npz), runs the prompt pass through the public surface alone
(prefill, prefill_many, vision_forward, vision_forward_many, decode, generated, generate_batch) and writes down

  calls     the library calls of the prompt pass, one list per issuing thread in the order the threads first appear.  ``hip._lib`` is
            replaced by a proxy while a configuration runs (the idea of gen_decode_transcript.py); a call is its entry name and its
            arguments: those of kind i / f / l / u in ``hip._SIGS`` verbatim, those of kind p as ``ptr`` or ``None`` (a null pointer,
            the default stream included).  A prompt pass allocates its own temporaries, so buffers cannot be named as the decode
            transcript names them;
  digests   sha256 of the result bytes after torch.cuda.synchronize(): the tower's output, per used slot the key count, step,
            current token, logits, the self-attention cache rows of the prompt, the cross-attention rows below the key count (and
            their e4m3 codes and scales under cross_kv="fp8"), and for the single configurations every tap of the text pass;
  tokens    single configurations on slot 0: the 8 greedy tokens after decode(7, use_graph=False); prefill_many configurations:
            6 tokens per request of generate_batch(..., max_new_tokens=6, stop_on_eos=False, use_graph=False).

The JSON also holds one digest of ``w.embed`` and ``w.patch_w``: a mismatch caused by another synthetic weight stream can be
told from a change of behaviour.

Usage:  python tests/golden/gen_mllama_prompt_pass.py [--out FILE] [--commit HASH] [--only NAME ...]
The JSON names the commit it was recorded at.  tests/test_mllama_prompt_pass_gpu.py compares every configuration against it.
"""
import argparse
import contextlib
import functools
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from gen_decode_transcript import _mllama, first_difference, vis_env  # noqa: E402,F401  (first_difference: for the test)

OUT = os.path.join(HERE, "mllama_prompt_pass.json")
TEXT_IDS = [1, 5, 6, 40, 41, 42, 7, 8]

# name -> run: "single" = prefill(ids, image, slot=slot, taps=...), "many" = prefill_many(requests); requests: letters of the
# npz images, "a+" = image a behind b's prompt with two more text tokens (another length: another layout), "a=" = image
# behind a's prompt (one layout for the whole batch), "text" = no image; env: the VIS_* switches (every other one is unset).
CONFIGS = {
    "single_image": dict(run="single", requests=["a"]),
    "single_text": dict(run="single", requests=["text"]),
    "single_slot1": dict(run="single", requests=["b"], slot=1, engine=dict(max_batch=4)),
    "single_cross_fp8": dict(run="single", requests=["a"], engine=dict(cross_kv="fp8")),
    "many_1": dict(run="many", requests=["a"]),
    "many_3_same_layout": dict(run="many", requests=["a=", "b=", "c="], engine=dict(max_batch=4)),
    "many_3_same_layout_fp8": dict(run="many", requests=["a=", "b=", "c="], engine=dict(max_batch=4, cross_kv="fp8")),
    "many_2_mixed_layout": dict(run="many", requests=["a", "b+"], engine=dict(max_batch=4)),
    "many_3_group_attn_off": dict(run="many", requests=["a=", "b=", "c="], engine=dict(max_batch=4), env={"VIS_GROUP_ATTN": "0"}),
    "many_2_one_stream": dict(run="many", requests=["a", "b"], engine=dict(max_batch=4), env={"VIS_PREFILL_STREAMS": "1"}),
}


class Recorder:
    """Stands in for ``hip._lib``: forwards every entry point; while armed, writes the call down first, per thread."""

    def __init__(self, real, sigs):
        self._real, self._sigs = real, sigs
        self.calls: dict = {}          # thread id -> its calls, in issue order (dicts keep the order of first appearance)
        self.armed = False

    def __getattr__(self, name):
        entry, sig = getattr(self._real, name), self._sigs[name]

        def call(*args):
            if self.armed:
                if len(args) != len(sig):
                    raise TypeError(f"{name}: {len(args)} arguments for the signature {sig!r}")
                shown = [("None" if not a else "ptr") if kind == "p" else repr(a) for kind, a in zip(sig, args)]
                self.calls.setdefault(threading.get_ident(), []).append(f"{name}({', '.join(shown)})")
            return entry(*args)
        return call


@contextlib.contextmanager
def recording():
    """``hip._lib`` replaced by a Recorder for the duration."""
    from vision_inspection_system_amd import hip
    real = hip.load()
    rec = Recorder(real, hip._SIGS)
    hip._lib = rec
    try:
        yield rec
    finally:
        hip._lib = real


def sha(t) -> str:
    """sha256 of a tensor's bytes (its logical, contiguous form)."""
    a = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(a.view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def weight_digest(device) -> str:
    _, eng = _mllama(device)
    return hashlib.sha256((sha(eng.w.embed) + sha(eng.w.patch_w)).encode()).hexdigest()


def _requests(device, names) -> list:
    g = np.load(os.path.join(HERE, "mllama_tiny.npz"))
    out = []
    for n in names:
        if n == "text":
            out.append((list(TEXT_IDS), None))
            continue
        ids = g[f"{n[0]}_ids"].tolist()
        if n.endswith("="):
            ids = g["a_ids"].tolist()
        elif n.endswith("+"):
            ids = g["b_ids"].tolist() + [9, 10]
        out.append((ids, torch.from_numpy(g[f"{n[0]}_image"]).to(device)))
    return out


def _slot_digests(eng, slot: int, S: int) -> dict:
    nk = int(eng.nkeys_b[slot].item()) + 1
    d = {"nkeys": sha(eng.nkeys_b[slot]), "step": sha(eng.step_b[slot]), "cur": sha(eng.cur_b[slot]),
         "logits": sha(eng.logits_b[slot]), "kcache": sha(eng.kcache_b[slot][:, :, :S]), "vcache": sha(eng.vcache_b[slot][:, :, :S]),
         "xk": sha(eng.xk_b[slot][:, :, :nk]), "xv": sha(eng.xv_b[slot][:, :, :nk])}
    if eng.cross_kv == "fp8":
        d.update(xkq=sha(eng.xkq_b[slot][:, :, :nk]), xks=sha(eng.xks_b[slot][:, :, :nk]),
                 xvq=sha(eng.xvq_b[slot][:, :, :nk]), xvs=sha(eng.xvs_b[slot][:, :, :nk]))
    return d


def record(name: str, device) -> dict:
    """Run configuration ``name`` and return {"calls": [[...] per thread], "digests": {...}, "tokens": ...}."""
    c = CONFIGS[name]
    with vis_env(c.get("env", {})), recording() as rec:
        cfg, eng = _mllama(device, **c.get("engine", {}))
        reqs = _requests(device, c["requests"])
        digests, tokens = {}, None
        if c["run"] == "single":
            (ids, frame), slot, taps = reqs[0], c.get("slot", 0), {}
            rec.armed = True
            eng.prefill(ids, frame, slot=slot, taps=taps)
            rec.armed = False
            torch.cuda.synchronize(device)
            digests["tower"] = sha(taps["cross_states"]) if "cross_states" in taps else None
            digests[f"slot{slot}"] = _slot_digests(eng, slot, len(ids))
            digests["taps"] = {k: sha(taps[k]) for k in [f"layer{i}" for i in range(cfg.layers)] + ["first_logits"] if k in taps}
            if slot == 0:
                eng.decode(7, use_graph=False)
                tokens = eng.generated(8)
        else:
            rec.armed = True
            slots, errors = eng.prefill_many(reqs)
            rec.armed = False
            torch.cuda.synchronize(device)
            if slots != list(range(len(reqs))) or any(errors):
                raise RuntimeError(f"{name}: prefill_many gave slots {slots}, errors {errors}")
            for slot, (ids, _) in zip(slots, reqs):
                digests[f"slot{slot}"] = _slot_digests(eng, slot, len(ids))
            tower = eng.vision_forward_many([fr for _, fr in reqs])
            torch.cuda.synchronize(device)
            digests["tower"] = [[sha(cs), int(n_tiles)] for cs, n_tiles in tower]
            tokens = eng.generate_batch(reqs, max_new_tokens=6, stop_on_eos=False, use_graph=False)
            if any(isinstance(t, Exception) for t in tokens):
                raise RuntimeError(f"{name}: generate_batch returned {tokens}")
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
