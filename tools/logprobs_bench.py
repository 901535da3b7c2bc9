"""Cost of token logprobs (vis_logprobs_f32) on the MI355X.

    python tools/logprobs_bench.py kernel [out.json]     # kernel time at V = 152064 / 128256, B = 1 / 4 / 32 / 64, k = 0 / 5 / 20
    python tools/logprobs_bench.py step [out.json]       # synthetic:7b decode step, logprobs off / k = 0 / k = 20, B = 1 and 64

kernel: 50 launches captured in one graph, replayed 20 times after a warm-up, device events; the row is what the lm_head
has just written (a row of 608 KB at V = 152064), so the logits are L2 / MALL resident here as in the engine.  Kernel-only times
come from a `rocprofv3 --kernel-trace --stats` run of the `kernel` mode (logprobs_stage1/2_kernel rows).
step: the engine's own decode step (B = 1: graph-replayed, chained layer head; B = 64: the batched step's graph) with the three
settings alternated in one process, 5 rounds, median ms per step."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_inspection_system_amd import hip  # noqa: E402

DEV = torch.device("cuda:0")


def kernel_times() -> list:
    rows = []
    for V in (152064, 128256):
        for B in (1, 4, 32, 64):
            x = torch.randn((B, V), device=DEV) * 4.0
            T = 64
            tokens = torch.randint(0, V, (B, T), dtype=torch.int32, device=DEV)
            step = torch.full((B,), 10, dtype=torch.int32, device=DEV)
            lp = torch.empty((B, T, 21), dtype=torch.float32, device=DEV)
            ids = torch.empty((B, T, 20), dtype=torch.int32, device=DEV)
            ws = hip.logprobs_ws(V, B, DEV)
            for k in (0, 5, 20):
                def run():
                    hip.logprobs(x, tokens, step, k, lp, ids, ws)
                run()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(50):
                        run()
                g.replay()
                torch.cuda.synchronize()
                ts = []
                for _ in range(20):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    g.replay()
                    e.record()
                    torch.cuda.synchronize()
                    ts.append(s.elapsed_time(e) * 1e3 / 50)
                us = float(np.median(ts))
                rows.append({"V": V, "B": B, "k": k, "us_per_call": round(us, 2),
                             "row_GB_per_s": round(B * V * 4 / us / 1e3, 1)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def step_times() -> list:
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    rng = np.random.default_rng(0)
    modes = [None, 0, 20]
    out = []
    # B = 1: the request path's single-sequence step (graph replay, chained layer head), ~1300-token context
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {m: [] for m in modes}
    for _ in range(5):
        for m in modes:
            eng._begin_logprobs(m)
            eng.prefill(ids, [], max_new_tokens=64)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    eng.lp_k = None
    for m in modes:
        out.append({"B": 1, "logprobs": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    # B = 64: the batched step's graph, 64 sequences of ~1300 tokens
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    eng.prefill_many(reqs, max_new_tokens=400)
    res = {m: [] for m in modes}
    for _ in range(5):
        for m in modes:
            eng.lp_k = m
            if m is not None and eng._lp is None:
                eng._begin_logprobs(m)
            g = eng._ensure_graph(B)
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    eng.lp_k = None
    for m in modes:
        out.append({"B": B, "logprobs": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)
