"""Cost of nucleus sampling / per-request seeds (vis_sample_f32) on the MI355X.

    python tools/sampling_bench.py kernel [out.json]   # per call at V = 152064 / 128256, B = 1 / 16 / 64, p = 0.9 / 0.999 / 0,
                                                       # T = 0.1 / 1.0, next to vis_argmax_f32 on the same rows
    python tools/sampling_bench.py step [out.json]     # synthetic:7b decode step at T = 1: sampling off / top_p = 0.9 / seed
                                                       # only, B = 1 and 64

kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events; the rows are N(0, 4) logits as
the lm_head writes them (L2 / MALL resident).  step: the engine's own decode step (B = 1: graph-replayed single-sequence
step; B = 64: the batched step's graph) with the three settings alternated in one process, 5 rounds, median ms per step."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_inspection_system_amd import hip  # noqa: E402

DEV = torch.device("cuda:0")


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
            T_tok = 64
            tokens = torch.zeros((B, T_tok), dtype=torch.int32, device=DEV)
            cur = torch.zeros(B, dtype=torch.int32, device=DEV)
            step = torch.zeros(B, dtype=torch.int32, device=DEV)
            seeds = torch.arange(B, dtype=torch.int32, device=DEV)
            ws = hip.sample_ws(V, B, DEV)
            wv = torch.empty(256 * B, dtype=torch.float32, device=DEV)
            wi = torch.empty(256 * B, dtype=torch.int32, device=DEV)
            tk = tokens if B > 1 else tokens[0]
            for T in (0.1, 1.0):
                def base():
                    step.zero_()
                    hip.argmax(x, wv, wi, tk, cur, step, T, 0)
                ref_us = _time(base)
                for p in (0.9, 0.999, 0.0):
                    def run():
                        step.zero_()
                        hip.sample(x, tk, cur, step, seeds, ws, T, p)
                    us = _time(run)
                    rows.append({"V": V, "B": B, "T": T, "top_p": p, "us_per_call": round(us, 2),
                                 "argmax_us_per_call": round(ref_us, 2)})
                    print(json.dumps(rows[-1]), flush=True)
    return rows


def step_times() -> list:
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    rng = np.random.default_rng(0)
    modes = {"off": (None, False), "top_p=0.9": (0.9, False), "seed": (None, True)}
    out = []
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {m: [] for m in modes}
    for _ in range(5):
        for m, (tp, seeded) in modes.items():
            eng._begin_sampling(tp, seeded)
            eng.prefill(ids, [], max_new_tokens=64, temperature=1.0, seed=3)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    eng._end_sampling()
    for m in modes:
        out.append({"B": 1, "sampling": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    eng._begin_sampling(None, True)          # the prompt passes write every slot's row seed
    eng.prefill_many(reqs, max_new_tokens=400, temperature=1.0, seed=3)
    res = {m: [] for m in modes}
    for _ in range(5):
        for m, (tp, seeded) in modes.items():
            eng._begin_sampling(tp, seeded)
            g = eng._ensure_graph(B)
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    eng._end_sampling()
    for m in modes:
        out.append({"B": B, "sampling": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)
