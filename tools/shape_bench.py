"""Cost of logit shaping (vis_shape_f32: top_k / min_p / logit_bias) on the MI355X.

    python tools/shape_bench.py kernel [out.json]   # per call at V = 152064 / 128256, B = 1 / 16 / 64: k = 40, min_p = 0.05
                                                    # and 8 biases, each alone and all three together, next to
                                                    # vis_argmax_f32 on the same rows
    python tools/shape_bench.py step [out.json]     # synthetic:7b decode step, shaping off / on, B = 1 and 64
    python tools/shape_bench.py all [out.json]      # both; the second only when the first ended well

Each of kernel and step runs in a child process of its own under a time limit; this process never opens the GPU.  A child
that fails or runs out of time ends the run: nothing more is started on the GPU.
kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events; the rows are N(0, 4) logits as
the lm_head writes them (L2 / MALL resident).  Bytes per call = B x V x 4 x (passes + 1): every pass reads the row, the last
writes it - 2 passes with a bias list alone, 3 with min_p, 5 with top_k.  step: the engine's own decode step (B = 1:
graph-replayed single-sequence step; B = 64: the batched step's graph), off and on alternated in one process, 5 rounds,
median ms per step; on = top_k 40, min_p 0.05 and 8 biases at temperature 0.7."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernel": 300, "step": 540}          # seconds per child
TOP_K, MIN_P, N_BIAS, TEMP = 40, 0.05, 8, 0.7
SETTINGS = {"top_k": (TOP_K, None, 0), "min_p": (0, MIN_P, 0), "logit_bias": (0, None, N_BIAS), "all": (TOP_K, MIN_P, N_BIAS)}
PASSES = {"top_k": 5, "min_p": 3, "logit_bias": 2, "all": 5}


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
    from vision_inspection_system_amd.shaping import ShapeBuffers
    dev = torch.device("cuda:0")
    rows = []
    for V in (152064, 128256):
        for B in (1, 16, 64):
            x = torch.randn((B, V), device=dev) * 4.0
            tokens = torch.zeros((B, 64), dtype=torch.int32, device=dev)
            cur = torch.zeros(B, dtype=torch.int32, device=dev)
            step = torch.full((B,), 8, dtype=torch.int32, device=dev)
            wv = torch.empty(256 * B, dtype=torch.float32, device=dev)
            wi = torch.empty(256 * B, dtype=torch.int32, device=dev)
            xs, tk = (x, tokens) if B > 1 else (x[0], tokens[0])
            shp = ShapeBuffers(B, V, dev)
            bias = tuple((int(i), -3.0) for i in torch.randperm(V)[:N_BIAS])

            def pick():
                step.fill_(8)
                hip.argmax(xs, wv, wi, tk, cur, step, 0.0, 0)

            def fill():
                step.fill_(8)

            fill_us = _time(fill)
            row = {"V": V, "B": B, "argmax_us_per_call": round(_time(pick) - fill_us, 2)}
            for name, (k, p, nb) in SETTINGS.items():
                for b in range(B):
                    shp.begin(b, k, p, bias[:nb], TEMP)
                us = _time(lambda: shp.apply(xs))
                row[name + "_us_per_call"] = round(us, 2)
                row[name + "_GBps"] = round(B * V * 4 * (PASSES[name] + 1) / us / 1e3, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_times() -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    rng = np.random.default_rng(0)
    out = []
    on = (TOP_K, MIN_P, tuple((int(i), -3.0) for i in rng.permutation(150000)[:N_BIAS]))
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng._begin_shaping([on] if m == "on" else None)
            eng._slot_shape[0] = on
            eng.prefill(ids, [], max_new_tokens=64, temperature=TEMP, seed=1)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    eng._end_shaping()
    for m in res:
        out.append({"B": 1, "shaping": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    eng._begin_shaping([on] * B)                # the prompt passes write every slot's parameters
    eng.prefill_many(reqs, max_new_tokens=400, temperature=TEMP, seed=1, shaping=[on] * B)
    res = {"off": [], "on": []}
    for _ in range(5):
        for m in res:
            eng.shape_on = m == "on"
            g = eng._ensure_graph(B)
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(16):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 16)
    eng._end_shaping()
    for m in res:
        out.append({"B": B, "shaping": m, "ms_per_step": round(float(np.median(res[m])), 4)})
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
        raise SystemExit(f"shape_bench {what}: no result within {LIMITS[what]} s - stopping")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        raise SystemExit(f"shape_bench {what}: the child ended with status {p.returncode} - stopping")
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
