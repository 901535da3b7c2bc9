"""Cost of ``stream=True`` (vis_stream_publish) and what it buys on the MI355X.

    python tools/stream_bench.py kernel [out.json]   # vis_stream_publish per call at 1 / 16 / 64 rows (behind a stop scan on
                                                     # the same rows, whose time is reported next to it)
    python tools/stream_bench.py step [out.json]     # synthetic:7b decode step with streaming off / on at 1 and 64 sequences
                                                     # (device time per step, three repeats, alternated), against the 1 %
                                                     # budget of the README; with STREAM_BENCH_PARENT=<checkout of the parent
                                                     # commit, built> the off figure of that tree too, in the same session
    python tools/stream_bench.py e2e [out.json]      # one request of 256 tokens: time to the first content chunk and the largest
                                                     # gap between chunks, against the wall time of the same request not streamed
    python tools/stream_bench.py all [out.json]      # all three; each only when the one before ended well

Each part runs in a child process of its own under a time limit; this process never opens the GPU.  A child that fails or
runs out of time ends the run: nothing more is started on the GPU."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"kernel": 180, "step": 560, "step_parent": 400, "e2e": 400}          # seconds per child
V, T = 152064, 4608
MODEL = "synthetic:7b"


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
    """Every launch of the timed graph publishes: the step counter is advanced on the device between two launches."""
    import torch
    from vision_inspection_system_amd import stop, stream
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    dev = torch.device("cuda:0")
    tok = ByteTokenizer(V, V - 4, V - 3, V - 2, (V - 1,))
    rows = []
    for B in (1, 16, 64):
        sb = stop.StopBuffers(tok, V, (V - 1,), B, dev)
        dfa = sb.load(("\n\n", "</report>"))
        st = stream.StreamBuffers(B, T, dev)
        st.load(dfa)
        tokens = torch.randint(97, 123, (B, T), dtype=torch.int32, device=dev)
        step = torch.ones(B, dtype=torch.int32, device=dev)

        def begin():
            for b in range(B):
                st.reset(b)
            sb.state.zero_()
            step.fill_(1)

        def scan_only():
            sb.scan(tokens, step)
            step.add_(1)

        def both():
            sb.scan(tokens, step)
            st.launch(sb.state, tokens, step)
            step.add_(1)

        begin()
        scan = _time(scan_only)         # 1 + 20 + 20 * 11 steps: within T
        begin()
        pair = _time(both)
        torch.cuda.synchronize()
        assert int(st.count.min()) > 200, "the timed launches did not publish"
        row = {"B": B, "stop_scan_us": round(scan, 2), "stop_scan_and_publish_us": round(pair, 2),
               "publish_us": round(pair - scan, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _image_messages():
    import base64
    import io
    import numpy as np
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (448, 448, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=85)
    url = "data:image/jpeg;base64," + base64.b64encode(buf.getvalue()).decode()
    return [{"role": "user", "content": [{"type": "text", "text": "Inspect this part and list every defect. " * 40},
                                         {"type": "image_url", "image_url": {"url": url}}]}]


def step_times(parent: bool = False) -> list:
    os.environ["VIS_IGNORE_EOS"] = "1"           # every call decodes the same number of steps
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    m = _image_messages()
    kw = dict(temperature=0.0, max_tokens=128)

    def one(B: int, on: bool) -> dict:
        if on:
            for _ in c.complete_many(MODEL, [m] * B, stream=True, **kw):
                pass
            from vision_inspection_system_amd.client import TIMING_LOG
            t = TIMING_LOG[-1]
        else:
            t = c.complete_many(MODEL, [m] * B, **kw)[0].timings
        assert t["sequences"] == B
        return {"sequences": B, "stream": on, "tree": "parent" if parent else "this",
                "decode_step_ms": round(t["decode_ms"] / max(1, t["decode_steps"]), 4)}

    rows = []
    for B in (1, 64):
        for on in ((False,) if parent else (False, True)):
            one(B, on)          # warm-up: model load, graphs, prefix cache
        for rep in range(3):
            for on in ((False,) if parent else (False, True)):
                row = dict(one(B, on), repeat=rep)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if not parent:
        for B in (1, 64):
            off = min(r["decode_step_ms"] for r in rows if r["sequences"] == B and not r["stream"])
            on = min(r["decode_step_ms"] for r in rows if r["sequences"] == B and r["stream"])
            row = {"sequences": B, "off_ms": off, "on_ms": on, "added_us": round((on - off) * 1e3, 1),
                   "budget_us": round(off * 10, 1), "within_1_percent": on - off <= off * 0.01}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def e2e_times() -> list:
    os.environ["VIS_IGNORE_EOS"] = "1"
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    m = _image_messages()
    kw = dict(temperature=0.0, max_tokens=256)
    rows = []
    c.chat.completions.create(model=MODEL, messages=m, **kw)          # warm-up
    for _ in c.chat.completions.create(model=MODEL, messages=m, stream=True, **kw):
        pass
    for rep in range(3):
        t0 = time.perf_counter()
        c.chat.completions.create(model=MODEL, messages=m, **kw)
        whole = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        stamps = [time.perf_counter() for ch in c.chat.completions.create(model=MODEL, messages=m, stream=True, **kw)
                  if ch.choices and ch.choices[0].delta.content]
        total = (time.perf_counter() - t0) * 1e3
        gaps = [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])]
        row = {"repeat": rep, "not_streamed_wall_ms": round(whole, 1), "streamed_wall_ms": round(total, 1),
               "first_content_chunk_ms": round((stamps[0] - t0) * 1e3, 1), "content_chunks": len(stamps),
               "largest_gap_ms": round(max(gaps), 2) if gaps else None}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _child(what: str) -> None:
    tree = os.environ.get("STREAM_BENCH_PARENT") if what == "step_parent" else ROOT
    sys.path.insert(0, tree)
    from vision_inspection_system_amd import hip
    hip.load()
    rows = {"kernel": kernel_times, "step": step_times, "step_parent": lambda: step_times(True), "e2e": e2e_times}[what]()
    print("RESULT " + json.dumps(rows), flush=True)


def _run_child(what: str) -> list:
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], stdout=subprocess.PIPE, text=True,
                           timeout=LIMITS[what])
    except subprocess.TimeoutExpired:
        raise SystemExit(f"stream_bench {what}: no result within {LIMITS[what]} s - stopping")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        raise SystemExit(f"stream_bench {what}: the child ended with status {p.returncode} - stopping")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        _child(sys.argv[2])
        sys.exit(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what not in ("kernel", "step", "e2e", "all"):
        raise SystemExit(__doc__)
    parts = ("kernel", "step", "e2e") if what == "all" else (what,)
    result = {}
    for w in parts:
        result[w] = _run_child(w)
        if w == "step" and os.environ.get("STREAM_BENCH_PARENT"):
            result["step_parent"] = _run_child("step_parent")
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(result if len(result) > 1 else result[what], f, indent=1)
