"""Cost of JSON mode (vis_json_mask + the masked pick) on the MI355X.

    python tools/json_mode_bench.py kernel [out.json]    # vis_json_mask at V = 152064 / 128256, B = 1 / 16 / 64, three states
    python tools/json_mode_bench.py step [out.json]      # synthetic:7b decode step, JSON mode off / on, B = 1 and 64

kernel: the vocabulary is synthetic (ids 0..255 the single bytes, the rest random JSON-heavy byte strings of 1..40 bytes,
the length mix of a byte-level BPE vocabulary is shorter), the state one of value-start (after '"a": '), after-key (after
'"key"': only ':' and whitespace survive the first byte) and in-string (every token walked or taken by the PLAIN fast path).
50 launches captured in one graph, replayed 20 times after a warm-up, device events, median us per launch.  The launch
re-folds nothing (step == the state's position), as in steady state after the first token.  Also reports the host-side
token-table build time of the 152064-token vocabulary.
step: the engine's own decode step (B = 1: graph-replayed, chained layer head, fused masked lm_head pick; B = 64: the batched
step's graph) with JSON mode off and on (B = 1 alternated, B = 64 one phase each), 5 rounds, median ms per step.  The synthetic:7b model's
tokenizer is byte level (ids 0..255), so its table is small; the kernel figures above are the ones of a real vocabulary."""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_inspection_system_amd import hip  # noqa: E402
from vision_inspection_system_amd import json_grammar as G  # noqa: E402

DEV = torch.device("cuda:0")
STATES = {"value_start": b'{"a": ', "after_key": b'{"key"', "in_string": b'{"k": "abc'}


class _Vocab:
    def __init__(self, V: int, seed: int = 0):
        rng = random.Random(seed)
        pieces = [b"{", b"}", b"[", b"]", b'"', b":", b",", b" ", b"\n", b"\\n", b"0", b"1", b"-", b".", b"e", b"true",
                  b"null", b"abc", b"ing", b" the", b"_x", b"Key", "é".encode(), "日本".encode(), b"\xe6", b"\x97"]
        self.toks = [bytes([b]) for b in range(256)]
        while len(self.toks) < V:
            self.toks.append(b"".join(rng.choice(pieces) for _ in range(rng.randint(1, 8)))[:rng.randint(1, 40)])

    def token_bytes(self, t: int) -> bytes:
        return self.toks[t]


def _time_graph(run, n: int = 50, reps: int = 20) -> float:
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
        voc = _Vocab(V)
        t0 = time.perf_counter()
        table = G.build_token_table(voc, V, [V - 1])
        build_s = time.perf_counter() - t0
        rows.append({"V": V, "table_build_s": round(build_s, 3), "table_bytes": int(table.data.nbytes + table.off.nbytes
                                                                                       + table.flags.nbytes)})
        print(json.dumps(rows[-1]), flush=True)
        dt = [torch.from_numpy(a).to(DEV) for a in (table.off, table.data, table.flags, table.eos_ids)]
        for B in (1, 16, 64):
            for name, prefix in STATES.items():
                st = G.initial_state()
                for b in prefix:
                    G.advance(st, b, table)
                P = len(prefix)
                state = torch.zeros((B, G.STATE_INTS), dtype=torch.int32)
                for s in (0, 1):            # both parity slots hold the folded state: every launch re-reads it
                    state[:, s * G.SLOT_INTS:s * G.SLOT_INTS + G.LEX_WORDS] = torch.tensor(st[:G.LEX_WORDS])
                    state[:, s * G.SLOT_INTS + G.POS] = P
                    state[:, s * G.SLOT_INTS + G.ANCHOR] = 1
                state = state.to(DEV)
                tokens = torch.zeros((B, 64), dtype=torch.int32, device=DEV)
                step = torch.full((B,), P, dtype=torch.int32, device=DEV)
                allow = torch.zeros((B, (V + 63) // 64), dtype=torch.int64, device=DEV)
                us = _time_graph(lambda: hip.json_mask(state, tokens, step, *dt, allow))
                allowed = int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in allow[0].cpu().tolist()))
                rows.append({"V": V, "B": B, "state": name, "us_per_call": round(us, 2), "allowed": allowed})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def step_times() -> list:
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    rng = np.random.default_rng(0)
    modes = [False, True]
    out = []
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {m: [] for m in modes}
    for _ in range(5):
        for m in modes:
            eng._begin_json(m)
            eng.prefill(ids, [], max_new_tokens=64)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    eng.json_on = False
    for m in modes:
        out.append({"B": 1, "json_mode": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    res = {m: [] for m in modes}
    for m in modes:     # one phase per mode, each after its own prompt passes (JSON mode resets the slots' grammar states)
        eng._begin_json(m)
        eng.prefill_many(reqs, max_new_tokens=400)
        g = eng._ensure_graph(B)
        g.replay()
        for _ in range(5):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    eng.json_on = False
    for m in modes:
        out.append({"B": B, "json_mode": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)
