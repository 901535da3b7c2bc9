"""Cost and gain of ``n`` choices per request (forked decode attention) on the MI355X.

    python tools/fork_bench.py kernel [out.json]   # vis_decode_attn_parts_forked next to vis_decode_attn_parts at 7B head
                                                   # shapes (28 / 4 heads): 8 and 64 sequences, context 2304, fork_len 2240
                                                   # from one parent, against shared_len 960 and against none
    python tools/fork_bench.py step [out.json]     # synthetic:7b, one image: n=8 in one request against the same request
                                                   # eight times in complete_many (eight slot seeds): prompt-pass ms,
                                                   # decode-step ms and the wall time of the call, three repeats, alternated
    python tools/fork_bench.py all [out.json]      # both; the second only when the first ended well

Each of kernel and step runs in a child process of its own under a time limit; this process never opens the GPU.  A child
that fails or runs out of time ends the run: nothing more is started on the GPU.
kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events, median us per launch; every
sequence steps at the last row of the context, so each launch reads the whole context."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernel": 240, "step": 560}          # seconds per child
HQ, HKV, HD, CTX, T = 28, 4, 128, 2304, 2560
FORK_LEN, SHARED_LEN, N = 2240, 960, 8


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
    dev = torch.device("cuda:0")
    nq = (HQ + 2 * HKV) * HD
    ns = -(-T // hip.DECODE_KEYS_PER_SPLIT)
    rows = []
    for B in (8, 64):
        kc = torch.randn((B, HKV, T, HD), device=dev).to(torch.bfloat16)
        vc = torch.randn((B, HKV, T, HD), device=dev).to(torch.bfloat16)
        kc[:, :, :FORK_LEN] = kc[0:1, :, :FORK_LEN]       # every sequence holds the parent's rows: all variants compute the same
        vc[:, :, :FORK_LEN] = vc[0:1, :, :FORK_LEN]
        cos = torch.ones((T, HD), device=dev).expand(B, -1, -1)
        sin = torch.zeros((T, HD), device=dev).expand(B, -1, -1)
        pr = hip.part_rows(B)
        part = torch.randn((pr * nq,), device=dev)
        step = torch.full((B,), CTX - 1, dtype=torch.int32, device=dev)
        po = torch.empty(B * HQ * ns * HD, dtype=torch.float32, device=dev)
        pml = torch.empty(B * HQ * ns * 2, dtype=torch.float32, device=dev)
        out = torch.empty((B, HQ * HD), dtype=torch.bfloat16, device=dev)
        parent = torch.zeros(B, dtype=torch.int32, device=dev)
        flen = torch.full((B,), FORK_LEN, dtype=torch.int32, device=dev)
        flen[0] = 0

        def run(**share):
            hip.decode_attn_parts(part, 1, cos, sin, kc, vc, step, po, pml, out, HQ, HKV, HD, ns, HD ** -0.5, **share)

        row = {"B": B, "context": CTX, "form": "streaming" if HKV * B >= 128 else "split",
               "parts_us": round(_time(lambda: run()), 2),
               f"parts_shared_{SHARED_LEN}_us": round(_time(lambda: run(shared_len=SHARED_LEN)), 2),
               f"parts_forked_{FORK_LEN}_us": round(_time(lambda: run(fork=(parent, flen))), 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_times() -> list:
    import io
    import base64
    import numpy as np
    from PIL import Image
    os.environ["VIS_IGNORE_EOS"] = "1"           # both calls decode the same number of steps
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (448, 448, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=85)
    url = "data:image/jpeg;base64," + base64.b64encode(buf.getvalue()).decode()
    m = [{"role": "user", "content": [{"type": "text", "text": "Inspect this part and list every defect. " * 40},
                                      {"type": "image_url", "image_url": {"url": url}}]}]
    kw = dict(temperature=0.7, max_tokens=64)
    model = "synthetic:7b"

    def one(forked: bool) -> dict:
        t0 = time.perf_counter()
        if forked:
            r = c.chat.completions.create(model=model, messages=m, n=N, **kw)
            steps = sum(1 for _ in r.choices)
        else:
            r = c.complete_many(model, [m] * N, **kw)[0]
            steps = N
        wall = (time.perf_counter() - t0) * 1e3
        t = r.timings
        assert steps == N and t["sequences"] == N
        return {"call": f"n={N}" if forked else f"{N} requests", "prompt_tokens": r.usage["prompt_tokens"],
                "prompt_pass_ms": round(t["prefill_ms"], 2), "decode_step_ms": round(t["decode_ms"] / max(1, t["decode_steps"]), 4),
                "wall_ms": round(wall, 1)}

    one(False)          # warm-up: model load, graphs, prefix cache
    one(True)
    rows = []
    for rep in range(3):
        for forked in (False, True):
            row = dict(one(forked), repeat=rep)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


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
        raise SystemExit(f"fork_bench {what}: no result within {LIMITS[what]} s - stopping")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        raise SystemExit(f"fork_bench {what}: the child ended with status {p.returncode} - stopping")
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
