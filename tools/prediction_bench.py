"""What a prediction (generate(.., prediction=), OpenAI's Predicted Outputs) costs and saves on the MI355X.

    python tools/prediction_bench.py kernel [out.json]   # vis_spec_draft_pred next to vis_spec_draft at a history of 2300
                                                         # ids, pred_len 128 / 1024 / 4608, with the cursor held (the
                                                         # draft is a copy) and lost (the search over the prediction runs
                                                         # and finds nothing, then the prompt lookup)
    python tools/prediction_bench.py step [out.json]     # synthetic:7b, 128 new tokens, per decode_weights format: the plain
                                                         # request, the request with prediction = its own plain reply, and
                                                         # with that reply with every 16th id replaced - each at k = 3 and
                                                         # k = 1: ms per reply token, steps, accepted / rejected drafts
    python tools/prediction_bench.py all [out.json]      # both; default out: profiles/prediction.json

Every measurement runs in a child process of its own under a time limit (step: one child per format); this process never
opens the GPU.  A child that fails or runs out of time ends the run: nothing more is started on the GPU.  Kernel times are
device events around graph replays, median of the repeats; request times are the decode stage's device time of
``last_timing`` (polls included), median of 3, next to the plain request measured in the same process.  The weights are
seeded noise: a prediction equal to the plain reply is the best case by construction, and the acceptance of a real
checkpoint against a real earlier report is unmeasured here."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"kernel": 240, "step": 420}          # seconds per child
T, HIST, V, LD = 2560, 2300, 152064, 4608
FORMATS = ("bf16", "fp8", "mxfp4")
N_NEW = 128


def kernel_times() -> list:
    import torch
    from spec_bench import _time
    from vision_inspection_system_amd import hip
    dev = torch.device("cuda:0")
    ints = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)     # noqa: E731
    prompt = torch.randint(0, 4, (T,), dtype=torch.int32, device=dev)
    tokens = torch.randint(0, 4, (T,), dtype=torch.int32, device=dev)
    half, step = ints(1024), ints(HIST)                                 # prompt 1024 ids, reply 1276: history 2300
    draft, nd = ints(1, 2, 3), ints(0)
    rows = [{"kernel": "vis_spec_draft", "history": HIST,
             "us": round(_time(lambda: hip.spec_draft(prompt, half, tokens, half, step, 3, 4, 2, V, draft, nd)), 2)}]
    print(json.dumps(rows[-1]), flush=True)
    for P in (128, 1024, LD):
        pred = torch.zeros(LD, dtype=torch.int32, device=dev)
        plen = ints(P)
        # held: seen = the reply's length, the cursor inside the prediction - every replay copies three ids.
        # lost: ids 7.. stand nowhere in the reply (0..3): the search reads the whole prediction, finds nothing, and the
        # prompt lookup follows.  Neither state moves, so every replay does the same work.
        for name, fill, state in (("held", 1, (P // 2, 0, HIST - 1024, 2, 0, 0, 0)), ("lost", 7, (-1, 0, HIST - 1024, 0, 0, 0, 0))):
            pred.fill_(fill)
            st = ints(*state)
            us = _time(lambda: hip.spec_draft_pred(prompt, half, tokens, half, step, 3, 4, 2, V, pred, plen, st, draft, nd))
            rows.append({"kernel": "vis_spec_draft_pred", "history": HIST, "pred_len": P, "cursor": name, "us": round(us, 2)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def step_times(fmt: str) -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd import weights as W
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    dev = torch.device("cuda:0")
    cfg = Qwen2VLConfig.qwen2_vl_7b()
    eng = Qwen2VLEngine(cfg, W.random_device_weights(cfg, dev, 0), dev, max_ctx=1024, decode_weights=fmt)
    ids = [9] + np.random.default_rng(0).integers(1000, 100000, 384).tolist()

    def run(**kw):
        ms, out = [], None
        for _ in range(4):                                       # the first run captures the graph
            out = eng.generate(ids, [], max_new_tokens=N_NEW, ignore_eos=True, **kw)
            ms.append(eng.last_timing["decode_ms"] / (len(out) - 1))
        return out, float(np.median(ms[1:])), dict(eng.last_timing)

    plain, t1, _ = run()
    rows = [{"format": fmt, "request": "plain", "ms_per_token": round(t1, 4), "steps": len(plain) - 1}]
    print(json.dumps(rows[-1]), flush=True)
    damaged = [t if (i + 1) % 16 else (t + 1) % cfg.vocab for i, t in enumerate(plain)]
    for name, pred in (("prediction = plain reply", plain), ("prediction = plain reply, every 16th id replaced", damaged)):
        for k in (3, 1):
            out, tk, t = run(prediction=pred, speculative=k)
            if out != plain:
                raise SystemExit(f"{fmt} {name} k={k}: the reply differs from the plain reply")
            rows.append({"format": fmt, "request": name, "k": k, "ms_per_token": round(tk, 4), "plain_ms_per_token": round(t1, 4),
                         "speedup": round(t1 / tk, 3), "steps": t["spec_steps"], "accepted": t["pred_accepted"],
                         "rejected": t["pred_rejected"]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def _child(what: str, arg: str) -> None:
    from vision_inspection_system_amd import hip
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times(arg)
    print("RESULT " + json.dumps(rows), flush=True)


def _run_child(what: str, arg: str = "-") -> list:
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, arg], stdout=subprocess.PIPE, text=True,
                           timeout=LIMITS[what])
    except subprocess.TimeoutExpired:
        raise SystemExit(f"prediction_bench {what} {arg}: no result within {LIMITS[what]} s - stopping")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        raise SystemExit(f"prediction_bench {what} {arg}: the child ended with status {p.returncode} - stopping")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        _child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what not in ("kernel", "step", "all"):
        raise SystemExit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "prediction.json")
    result = {}
    if what in ("kernel", "all"):
        result["kernel"] = _run_child("kernel")
    if what in ("step", "all"):
        result["step"] = [row for fmt in FORMATS for row in _run_child("step", fmt)]
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
