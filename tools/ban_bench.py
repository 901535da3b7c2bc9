"""Cost of the token bans (vis_ban_f32: no_repeat_ngram_size / bad_words / min_tokens) on the MI355X.

    python tools/ban_bench.py kernel [out.json]   # per call at V = 152064 / 128256, B = 1 / 16 / 64, a history of 2300 ids
                                                  # (2000 prompt + 300 generated), n-gram 3 + 4 bad words + min_tokens, next
                                                  # to vis_argmax_f32 on the same rows
    python tools/ban_bench.py step [out.json]     # synthetic:7b decode step, bans off / on, B = 1 and 64
    python tools/ban_bench.py all [out.json]      # both; the second only when the first ended well

Each of kernel and step runs in a child process of its own under a time limit; this process never opens the GPU.  A child
that fails or runs out of time ends the run: nothing more is started on the GPU.
kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events; the rows are N(0, 4) logits as
the lm_head writes them (L2 / MALL resident).  Bytes per call = B x V x 8 (one read, one write of every id; the history is a
few KB per row).  step: the engine's own decode step (B = 1: graph-replayed single-sequence step; B = 64: the batched
step's graph), off and on alternated in one process, 5 rounds, median ms per step; on = n-gram 3, 4 bad words and
min_tokens 8 at temperature 0.7.  Off issues exactly the launches of the commit before the switch existed
(tests/test_decode_transcript_gpu.py), so its figure is that commit's; the project's budget for a switch is 1 % of a step."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernel": 300, "step": 540}          # seconds per child
NGRAM, MIN_TOKENS, TEMP, PROMPT, GENERATED = 3, 8, 0.7, 2000, 300
WORDS = [(11, 12), (13,), (14, 15, 16, 17), (21, 22, 23, 24, 25, 26, 27, 28)]


def _time(run, n=20, reps=10) -> float:
    import numpy as np
    import torch
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
    import torch
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.ban import BanBuffers
    dev = torch.device("cuda:0")
    rows = []
    T = PROMPT + GENERATED + 64
    for V in (152064, 128256):
        for B in (1, 16, 64):
            x = torch.randn((B, V), device=dev) * 4.0
            tokens = torch.randint(0, V, (B, T), dtype=torch.int32, device=dev)
            cur = torch.zeros(B, dtype=torch.int32, device=dev)
            step = torch.full((B,), PROMPT + GENERATED, dtype=torch.int32, device=dev)
            wv = torch.empty(256 * B, dtype=torch.float32, device=dev)
            wi = torch.empty(256 * B, dtype=torch.int32, device=dev)
            xs, tk = (x, tokens) if B > 1 else (x[0], tokens[0])
            bn = BanBuffers(B, T, V, (V - 1, V - 2), dev)
            bn.load(WORDS)
            start = torch.full((1,), PROMPT, dtype=torch.int32, device=dev)
            for b in range(B):
                bn.begin(b, torch.randint(0, V, (PROMPT,), dtype=torch.int32, device=dev), start, NGRAM,
                         PROMPT + GENERATED)      # more than generated: the EOS ids are banned in every call

            def pick():
                step.fill_(PROMPT + GENERATED)
                hip.argmax(xs, wv, wi, tk, cur, step, 0.0, 0)

            def fill():
                step.fill_(PROMPT + GENERATED)

            fill_us = _time(fill)
            us = _time(lambda: bn.apply(xs, tk, step))
            row = {"V": V, "B": B, "history": PROMPT + GENERATED, "argmax_us_per_call": round(_time(pick) - fill_us, 2),
                   "ban_us_per_call": round(us, 2), "ban_GBps": round(B * V * 8 / us / 1e3, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_times() -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd.ban import BanRequest
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    rng = np.random.default_rng(0)
    out = []
    words = ("ab", "c", "defg", "hijklmno")       # 2, 1, 4 and 8 ids with the synthetic model's byte tokenizer
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng._begin_ban(BanRequest([(NGRAM, MIN_TOKENS)], words) if m == "on" else None)
            eng._slot_ban[0] = (NGRAM, MIN_TOKENS)
            eng.prefill(ids, [], max_new_tokens=64, temperature=TEMP, seed=1)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    eng._end_ban()
    for m in res:
        out.append({"B": 1, "bans": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    eng._begin_ban(BanRequest([(NGRAM, MIN_TOKENS)] * B, words))      # the prompt passes write every slot's parameters
    eng.prefill_many(reqs, max_new_tokens=400, temperature=TEMP, seed=1, ban=[(NGRAM, MIN_TOKENS)] * B)
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng.ban_on = m == "on"
            g = eng._ensure_graph(B)
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    eng._end_ban()
    for m in res:
        out.append({"B": B, "bans": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


def _child(what: str) -> None:
    from vision_inspection_system_amd import hip
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    print("RESULT " + json.dumps(rows), flush=True)


def _run_child(what: str) -> list:
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], stdout=subprocess.PIPE, text=True,
                           timeout=LIMITS[what])
    except subprocess.TimeoutExpired:
        raise SystemExit(f"ban_bench {what}: no result within {LIMITS[what]} s - stopping")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        raise SystemExit(f"ban_bench {what}: the child ended with status {p.returncode} - stopping")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        _child(sys.argv[2])
        sys.exit(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what not in ("kernel", "step", "all"):
        raise SystemExit(__doc__)
    result = {w: _run_child(w) for w in (("kernel", "step") if what == "all" else (what,))}
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(result if what == "all" else result[what], f, indent=1)
