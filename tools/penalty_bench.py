"""Cost of the logit penalties (vis_penalize_f32) on the MI355X.

    python tools/penalty_bench.py kernel [out.json]   # per call at V = 152064 / 128256, B = 1 / 16 / 64, next to
                                                      # vis_argmax_f32 on the same rows
    python tools/penalty_bench.py step [out.json]     # synthetic:7b decode step, penalties off / on, B = 1 and 64

kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events; the rows are N(0, 4) logits as
the lm_head writes them (L2 / MALL resident), 1000 prompt ids marked per row, the triple (1.3, 0.5, 0.2).  The step does not
advance between the timed launches, so they fold no token (in steady state: one compare per id and launch, in registers).
Bytes per call = B x V x 10 (4 logit in, 2 state in, 4 logit out).  step: the engine's own decode step (B = 1: graph-replayed
single-sequence step; B = 64: the batched step's graph), off and on alternated in one process, 5 rounds, median ms per step."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_inspection_system_amd import hip  # noqa: E402

DEV = torch.device("cuda:0")
TRIPLE = (1.3, 0.5, 0.2)


def _time(run, n=20, reps=10) -> float:
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            run()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / n)
    return float(np.median(ts))


def kernel_times() -> list:
    rows = []
    for V in (152064, 128256):
        for B in (1, 16, 64):
            x = torch.randn((B, V), device=DEV) * 4.0
            out = torch.empty_like(x)
            tokens = torch.zeros((B, 64), dtype=torch.int32, device=DEV)
            cur = torch.zeros(B, dtype=torch.int32, device=DEV)
            step = torch.full((B,), 8, dtype=torch.int32, device=DEV)
            state = hip.penalty_state(V, B, DEV)
            params = torch.tensor([TRIPLE] * B, dtype=torch.float32, device=DEV)
            prompt = torch.randint(0, V, (1000,), dtype=torch.int32, device=DEV)
            for b in range(B):
                hip.penalty_prompt(state[b], V, prompt)
            wv = torch.empty(256 * B, dtype=torch.float32, device=DEV)
            wi = torch.empty(256 * B, dtype=torch.int32, device=DEV)
            xs, os_, tk = (x, out, tokens) if B > 1 else (x[0], out[0], tokens[0])

            def pick():
                step.fill_(8)
                hip.argmax(xs, wv, wi, tk, cur, step, 0.0, 0)

            def fill():
                step.fill_(8)

            def run():
                step.fill_(8)
                hip.penalize(xs, state, params, tk, step, os_)
            fill_us = _time(fill)
            us = _time(run) - fill_us
            rows.append({"V": V, "B": B, "us_per_call": round(us, 2), "argmax_us_per_call": round(_time(pick) - fill_us, 2),
                         "bytes": B * V * 10, "GBps": round(B * V * 10 / us / 1e3, 1)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def step_times() -> list:
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    rng = np.random.default_rng(0)
    out = []
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng._begin_penalties([TRIPLE] if m == "on" else None)
            eng._slot_pen[0] = TRIPLE
            eng.prefill(ids, [], max_new_tokens=64)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    eng._end_penalties()
    for m in res:
        out.append({"B": 1, "penalties": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    eng._begin_penalties([TRIPLE] * B)          # the prompt passes mark every slot's prompt and write its triple
    eng.prefill_many(reqs, max_new_tokens=400, penalties=[TRIPLE] * B)
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng.pen_on = m == "on"
            g = eng._ensure_graph(B)
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    eng._end_penalties()
    for m in res:
        out.append({"B": B, "penalties": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)
