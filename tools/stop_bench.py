"""Cost of stop strings (vis_stop_scan) on the MI355X.

    python tools/stop_bench.py kernel [out.json]   # per call at V = 152064 / 128256, B = 1 / 16 / 64, 1 and 4 stop strings
    python tools/stop_bench.py step [out.json]     # synthetic:7b decode step, stop off / on, 1 and 64 sequences

kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events.  Every launch folds ONE new token
per row, as in a decode step: the graph zeroes the records once and advances the step by one in front of every launch (the
same graph without the launches is timed too and subtracted).  The rows hold random ids of a synthetic vocabulary (single
bytes, then strings of 1..40 bytes; 7 bytes per token on average); the stop strings occur nowhere, so every row stays open
and walks all its bytes.  step: the engine's own decode step (1 sequence: graph-replayed single-sequence step; 64: the batched
step's graph), off and on alternated in one process, 5 rounds, median ms per step."""
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_inspection_system_amd import hip, stop  # noqa: E402
from vision_inspection_system_amd.json_grammar import build_token_table  # noqa: E402

DEV = torch.device("cuda:0")
STOPS = {1: ["```"], 4: ["```", "~~~", "<|end|>", "END OF REPORT"]}      # no synthetic token holds a backquote, 'D' or '<'
N = 20


class _Vocab:
    def __init__(self, V: int, seed: int):
        rng = random.Random(seed)
        pieces = [b"{", b"}", b'"', b":", b",", b" ", b"\n", b"  ", b"0", b"1", b"9", b"-", b".", b"e", b"true", b"false", b"null",
                  b"abc", b"key", b"_x", "é".encode(), "日本".encode()]
        self.toks = [bytes([b]) for b in range(256)]
        while len(self.toks) < V:
            self.toks.append(b"".join(rng.choice(pieces) for _ in range(rng.randint(1, 12)))[:rng.randint(1, 40)])

    def token_bytes(self, t: int) -> bytes:
        return self.toks[t]


class _Share:
    def __init__(self, table):
        self.table = table
        self.off, self.data = torch.from_numpy(table.off).to(DEV), torch.from_numpy(table.data).to(DEV)
        self.flags, self.eos = torch.from_numpy(table.flags).to(DEV), torch.from_numpy(table.eos_ids).to(DEV)


def _time(body, reps=10) -> float:
    """us per replay of the graph of ``body``."""
    body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return float(np.median(ts))


def kernel_times() -> list:
    rows = []
    for V in (152064, 128256):
        table = build_token_table(_Vocab(V, seed=11), V, [V - 1])
        share = _Share(table)
        mean_bytes = float(np.diff(table.off)[256:].mean())
        for B in (1, 16, 64):
            for n_stops in (1, 4):
                buf = stop.StopBuffers(None, V, [V - 1], B, DEV, share=share)
                buf.load(STOPS[n_stops])
                tokens = torch.randint(256, V - 1, (B, 64), dtype=torch.int32, device=DEV)
                step = torch.zeros(B, dtype=torch.int32, device=DEV)

                def frame(launch: bool):
                    buf.state.zero_()
                    step.fill_(8)
                    for _ in range(N):
                        step.add_(1)
                        if launch:
                            buf.scan(tokens, step, 0, True)

                us = (_time(lambda: frame(True)) - _time(lambda: frame(False))) / N
                torch.cuda.synchronize()
                rec = buf.records(range(B))
                assert all(r[stop.REASON] == 0 and r[stop.N_TOKENS] == N for r in rec), "the rows must stay open"
                rows.append({"V": V, "B": B, "stops": n_stops, "us_per_call": round(us, 2),
                             "bytes_walked_per_row": round(mean_bytes, 1)})
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
            eng._begin_stop(stop.check_stop(STOPS[4]) if m == "on" else None)
            eng.prefill(ids, [], max_new_tokens=64)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    for m in res:
        out.append({"B": 1, "stop": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    eng._begin_stop(stop.check_stop(STOPS[4]))       # the prompt passes start every slot's record
    eng.prefill_many(reqs, max_new_tokens=400)
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng.stop_on = m == "on"
            g = eng._ensure_graph(B)
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    open_rows = sum(r[stop.REASON] == 0 for r in eng._stop.records(range(B)))
    eng.stop_on = False
    for m in res:
        out.append({"B": B, "stop": m, "ms_per_step": round(float(np.median(res[m])), 4), "rows_still_open": int(open_rows)})
        print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)
