"""Cost of a speculative decode step on the Auditor (MllamaEngine(.., speculative=True)) on the MI355X, and with it the
acceptance at which it pays.

    python tools/auditor_spec_bench.py kernel [out.json]   # vis_decode_cross_attn_draft and vis_decode_cross_attn_fp8_draft at
                                                           # R = 2, 3, 4 next to R single-row launches (vis_decode_cross_attn /
                                                           # _fp8): 32 / 8 heads, the 11B key count (4 tiles x 1601 = 6404 keys
                                                           # in 6464 rows, 101 splits); us and GB/s on algorithmic bytes
    python tools/auditor_spec_bench.py step [out.json]     # synthetic:mllama-11b, per decode_weights (bf16, fp8, mxfp4) x
                                                           # cross_kv (bf16, fp8), one process: the plain single-sequence step
                                                           # as the engine runs it (chained for bf16) next to the speculative
                                                           # step at R = 2, 3, 4; t_R / t_1 - 1 = the drafts a step must get
                                                           # accepted, on average, to break even
    python tools/auditor_spec_bench.py all [out.json]      # both; default out: profiles/auditor_speculative.json

Each mode runs in a child process of its own under a time limit; this process never opens the GPU.  A child that fails or
runs out of time ends the run: nothing more is started on the GPU.  Times are device events around graph replays, median of
the repeats.  The yardsticks are the single-row kernels and the plain step of the same process; no threshold is fixed in
advance.  The weights are seeded noise: acceptance on a real checkpoint is not measured here."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernel": 240, "step": 900}          # seconds per child
HQ, HKV, HD, NKEYS, TK = 32, 8, 128, 6404, 6464
FORMATS = ("bf16", "fp8", "mxfp4")
CROSS_KV = ("bf16", "fp8")


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
    ns = TK // hip.DECODE_KEYS_PER_SPLIT
    k = torch.randn((HKV, TK, HD), device=dev).to(torch.bfloat16)
    v = torch.randn((HKV, TK, HD), device=dev).to(torch.bfloat16)
    kq, vq = torch.empty_like(k, dtype=torch.uint8), torch.empty_like(v, dtype=torch.uint8)
    ksc, vsc = torch.empty((HKV, TK), device=dev), torch.empty((HKV, TK), device=dev)
    hip.quantize_cross_kv(k, kq, ksc)
    hip.quantize_cross_kv(v, vq, vsc)
    w = torch.ones(HD, device=dev).to(torch.bfloat16)
    nk = torch.full((1,), NKEYS - 1, dtype=torch.int32, device=dev)
    nq = (HQ + 2 * HKV) * HD
    # what one pass must move: the live K and V rows (and their scales), every row's q in and output out
    kv_bytes = {"bf16": 2 * HKV * NKEYS * HD * 2, "fp8": 2 * HKV * NKEYS * (HD + 4)}
    forms = {"bf16": (hip.decode_cross_attn, hip.decode_cross_attn_draft, (k, v)),
             "fp8": (hip.decode_cross_attn_fp8, hip.decode_cross_attn_fp8_draft, (kq, ksc, vq, vsc))}
    rows = []
    for fmt, (single, draft, kv) in forms.items():
        for R in (1, 2, 3, 4):
            qbuf = torch.randn((R, nq), device=dev).to(torch.bfloat16)
            q = qbuf[:, :HQ * HD]
            qs = [q[r].contiguous() for r in range(R)]
            po = torch.empty(R * HQ * ns * HD, dtype=torch.float32, device=dev)
            pml = torch.empty(R * HQ * ns * 2, dtype=torch.float32, device=dev)
            out = torch.empty((R, HQ * HD), dtype=torch.bfloat16, device=dev)

            def singles():
                for r in range(R):
                    single(qs[r], w, *kv, nk, po, pml, out[r], HQ, HKV, HD, ns, HD ** -0.5, 1e-5)

            t_d = _time(lambda: draft(q, w, *kv, nk, po, pml, out, HQ, HKV, HD, ns, HD ** -0.5, 1e-5))
            t_s = _time(singles)
            io = R * HQ * HD * 2 * 2
            row = {"cross_kv": fmt, "R": R, "keys": NKEYS, "draft_us": round(t_d, 2),
                   "draft_GBps": round((kv_bytes[fmt] + io) / t_d / 1e3, 1),
                   "single_row_launches_us": round(t_s, 2),
                   "single_row_launches_GBps": round(R * (kv_bytes[fmt] + io // R) / t_s / 1e3, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_times() -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd import mllama_weights as MW
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.spec import SpecConfig
    dev = torch.device("cuda:0")
    cfg = MW.MllamaConfig.mllama_11b()
    w = MW.random_device_weights(cfg, dev, 0)
    frame = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)).to(dev)
    phrase = np.random.default_rng(0).integers(1000, 100000, 24).tolist()
    ids = [cfg.image_token_id] + [9] + phrase * 12               # an image and 289 ids that repeat themselves every 24
    n, reps = 16, 5

    def timed(run) -> float:
        ts = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) / n)
        return float(np.median(ts))

    rows = []
    for fmt in FORMATS:
        for xkv in CROSS_KV:
            eng = MllamaEngine(cfg, w, dev, max_ctx=1024, decode_weights=fmt, cross_kv=xkv, speculative=True)
            eng.prefill(ids, frame)
            eng.decode(4)                                            # graph capture and warm-up
            t1 = timed(lambda: eng.decode(n))
            rows.append({"decode_weights": fmt, "cross_kv": xkv, "R": 1,
                         "step": "plain (chained)" if eng.chain_sync is not None else "plain", "step_ms": round(t1, 4)})
            print(json.dumps(rows[-1]), flush=True)
            for R in (2, 3, 4):
                eng.prefill(ids, frame)
                eng._spec_begin(SpecConfig(R - 1, 4, 2), 10 ** 6)
                eng._decode_steps_spec(4, R, True)
                tr = timed(lambda: eng._decode_steps_spec(n, R, True))
                rows.append({"decode_weights": fmt, "cross_kv": xkv, "R": R, "step": "speculative", "step_ms": round(tr, 4),
                             "break_even_accepted_per_step": round(tr / t1 - 1, 4)})
                print(json.dumps(rows[-1]), flush=True)
            del eng
            torch.cuda.empty_cache()
    return rows


def _child(what: str) -> None:
    from vision_inspection_system_amd import hip
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    print("RESULT " + json.dumps(rows), flush=True)


def _run_child(what: str) -> list:
    import threading
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", what], stdout=subprocess.PIPE, text=True)
    late = threading.Timer(LIMITS[what], p.kill)      # the child's lines are passed on as they come; the limit ends it
    late.start()
    try:
        lines = []
        for ln in p.stdout:
            lines.append(ln)
            if not ln.startswith("RESULT "):
                sys.stdout.write(ln)
                sys.stdout.flush()
        rc = p.wait()
    finally:
        fired = not late.is_alive()
        late.cancel()
    if rc != 0:
        why = f"no result within {LIMITS[what]} s" if fired else f"the child ended with status {rc}"
        raise SystemExit(f"auditor_spec_bench {what}: {why} - stopping")
    return json.loads([ln for ln in lines if ln.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        _child(sys.argv[2])
        sys.exit(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what not in ("kernel", "step", "all"):
        raise SystemExit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "auditor_speculative.json")
    result = {}
    if what in ("kernel", "all"):
        result["kernel"] = _run_child("kernel")
    if what in ("step", "all"):
        result["step"] = _run_child("step")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
