"""MXFP4 decode weights on the MI355X: the W4A16 GEMV next to the bf16 and e4m3 ones, and the decode step on each.

    python tools/mxfp4_bench.py kernel [out.json]   # vis_gemv_mxfp4w per call at the five 7B decode shapes, next to
                                                    # vis_gemv_bf16 and vis_gemv_fp8w on the same shapes; then the batched
                                                    # projection vis_gemm_decode_mxfp4 at 8 / 16 / 32 / 64 rows next to
                                                    # vis_gemm_decode_bf16 on the de-quantised weights
    python tools/mxfp4_bench.py step [out.json]     # synthetic:7b decode step at 1 / 4 / 16 / 32 / 64 sequences: bf16, fp8 (up
                                                    # to 16), mxfp4 on the rows step, mxfp4 with mxfp4_gemm_from=5
    python tools/mxfp4_bench.py all [out.json]      # both, each in a child process under its own timeout

kernel: 20 launches captured in one graph, replayed 10 times after a warm-up, device events, median.  Every launch of a graph
reads its OWN copy of the weights (20 copies, 0.3-5.4 GB per format and shape), so no byte comes from the 256 MB MALL.  GB/s
on algorithmic bytes: N K 2 (bf16), N K + 4 N (fp8), N K / 2 + N K / 32 (mxfp4), plus B K 2 of activations for the batched
projections (the partial slabs are not counted); frac_8TBps = GB/s / 8000.
step: one engine per precision in one process (the 7B weights are random; contexts of 1289 prompt tokens), the engine's own
graph-replayed step (1 sequence: the single-sequence step; more: the batched step), 5 rounds alternated, median ms.
"mxfp4_mfma" is decode_weights="mxfp4" with mxfp4_gemm_from=5: at 1 and 4 sequences it runs the same launches as "mxfp4"."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_inspection_system_amd import hip  # noqa: E402

DEV = torch.device("cuda:0")
# (name, N, K, norm prologue, act): the five projections of a 7B decode step
SHAPES = [("qkv", 4608, 3584, True, 0), ("o", 3584, 3584, False, 0), ("gate_up", 37888, 3584, True, 3),
          ("down", 3584, 18944, False, 0), ("lm_head", 152064, 3584, True, 0)]
COPIES = 20
GEMM_ROWS = (8, 16, 32, 64)
TIMEOUTS = {"kernel": 600, "step": 900}


def _time(run, reps=10) -> float:
    """us per launch: ``run(i)`` for i in 0..COPIES-1 captured as one graph."""
    for i in range(COPIES):
        run(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(COPIES):
            run(i)
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / COPIES)
    return float(np.median(ts))


def kernel_times() -> list:
    rows = []
    for name, N, K, norm, act in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(N + K)
        w = (torch.randn((N, K), generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16)
        x = torch.randn((K,), generator=g, device=DEV).to(torch.bfloat16)
        nw = torch.ones((K,), dtype=torch.bfloat16, device=DEV) if norm else None
        y = torch.empty((N // 2 if act else N,), dtype=torch.bfloat16, device=DEV)
        q8, s8 = hip.quantize_fp8_rows(w)
        q4, s4 = hip.quantize_mxfp4_rows(w)
        w16 = [w.clone() for _ in range(COPIES)]
        w8 = [q8.clone() for _ in range(COPIES)]
        w4 = [(q4.clone(), s4.clone()) for _ in range(COPIES)]
        del w, q8, q4
        res = {
            "bf16": (_time(lambda i: hip.gemv(x, w16[i], y, norm_w=nw, act=act)), N * K * 2),
            "fp8": (_time(lambda i: hip.gemv_fp8(x, w8[i], s8, y, norm_w=nw, act=act)), N * K + 4 * N),
            "mxfp4": (_time(lambda i: hip.gemv_mxfp4(x, *w4[i], y, norm_w=nw, act=act)), N * K // 2 + N * K // 32),
        }
        row = {"shape": name, "N": N, "K": K}
        for k, (us, nbytes) in res.items():
            row[k] = {"us_per_call": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1),
                      "frac_8TBps": round(nbytes / us / 1e3 / 8000, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del w16, w8, w4
        torch.cuda.empty_cache()
    return rows


def gemm_times() -> list:
    """The batched decode projection: vis_gemm_decode_mxfp4 next to vis_gemm_decode_bf16 on the same (de-quantised) weights;
    partial slabs for the layer projections, direct f32 logits for the lm_head, as the engine issues them."""
    rows = []
    for name, N, K, _, _ in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(N + K)
        w = (torch.randn((N, K), generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16)
        q4, s4 = hip.quantize_mxfp4_rows(w)
        w = hip.dequantize_mxfp4(q4, s4).to(torch.bfloat16)
        w16 = [w.clone() for _ in range(COPIES)]
        w4 = [(q4.clone(), s4.clone()) for _ in range(COPIES)]
        del w, q4
        direct = name == "lm_head"
        for B in GEMM_ROWS:
            x = torch.randn((B, K), generator=g, device=DEV).to(torch.bfloat16)
            if direct:
                kw = {"out": torch.empty((B, N), dtype=torch.float32, device=DEV)}
            else:
                kw = {"part": torch.empty(16 * hip.part_rows(B) * N, dtype=torch.float32, device=DEV)}
            res = {
                "bf16": (_time(lambda i: hip.decode_gemm(x, w16[i], **kw)), N * K * 2 + B * K * 2),
                "mxfp4": (_time(lambda i: hip.decode_gemm_mxfp4(x, *w4[i], **kw)), N * K // 2 + N * K // 32 + B * K * 2),
            }
            row = {"shape": name, "N": N, "K": K, "rows": B, "kernel": "gemm_decode"}
            for k, (us, nbytes) in res.items():
                row[k] = {"us_per_call": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1),
                          "frac_8TBps": round(nbytes / us / 1e3 / 8000, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, w4
        torch.cuda.empty_cache()
    return rows


def step_times() -> list:
    from vision_inspection_system_amd import weights as W
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg = Qwen2VLConfig.qwen2_vl_7b()
    w = W.random_device_weights(cfg, DEV, 0)
    engines = {p: Qwen2VLEngine(cfg, w, DEV, max_ctx=2048, max_batch=64, decode_weights=p) for p in ("bf16", "fp8", "mxfp4")}
    engines["mxfp4_mfma"] = Qwen2VLEngine(cfg, w, DEV, max_ctx=2048, max_batch=64, decode_weights="mxfp4", mxfp4_gemm_from=5)
    rng = np.random.default_rng(0)
    out = []
    for B in (1, 4, 16, 32, 64):
        reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
        steps = {}
        live = {p: e for p, e in engines.items() if p != "fp8" or B <= 16}
        for p, eng in live.items():
            if B == 1:
                eng.prefill(reqs[0][0], [], max_new_tokens=400)
                steps[p] = lambda eng=eng: eng.decode(16)
            else:
                eng.prefill_many(reqs, max_new_tokens=400)
                steps[p] = lambda g=eng._ensure_graph(B): [g.replay() for _ in range(16)]
            steps[p]()
        res = {p: [] for p in live}
        for _ in range(5):
            for p in live:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                steps[p]()
                e.record()
                torch.cuda.synchronize()
                res[p].append(s.elapsed_time(e) / 16)
        for p in live:
            out.append({"sequences": B, "decode_weights": p, "ms_per_step": round(float(np.median(res[p])), 4)})
            print(json.dumps(out[-1]), flush=True)
    return out


def run_all(path) -> list:
    """kernel, then step, each a fresh child under its own time limit; nothing more is started after a failure."""
    rows = []
    for what in ("kernel", "step"):
        part = f"{path}.{what}" if path else os.devnull
        r = subprocess.run(["timeout", "-k", "10", str(TIMEOUTS[what]), sys.executable, os.path.abspath(__file__), what]
                           + ([part] if path else []))
        if r.returncode != 0:
            raise SystemExit(f"mxfp4_bench {what} ended with status {r.returncode}; nothing more is started")
        if path:
            with open(part) as f:
                rows.append({what: json.load(f)})
    return rows


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    path = sys.argv[2] if len(sys.argv) > 2 else None
    if what == "all":
        rows = run_all(path)
    else:
        hip.load()
        rows = kernel_times() + gemm_times() if what == "kernel" else step_times()
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)
