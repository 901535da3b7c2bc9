"""Cost of a speculative decode step (spec.py) on the MI355X, and with it the acceptance at which it pays.

    python tools/spec_bench.py kernel [out.json]   # vis_decode_attn_draft (28 / 4 heads, context 2304), vis_spec_accept
                                                   # (V = 152064) and vis_spec_draft (history 2304) at R = 2, 3, 4, next to
                                                   # vis_decode_attn / vis_argmax_f32 for one row
    python tools/spec_bench.py step [out.json]     # synthetic:7b, per decode_weights format (bf16, fp8, mxfp4): the plain
                                                   # chained step next to the speculative step at R = 2, 3, 4 in one process;
                                                   # t_R / t_1 - 1 = the drafts a step must get accepted, on average, to break
                                                   # even; tokens per step on a synthetic prompt that repeats itself
    python tools/spec_bench.py all [out.json]      # both; default out: profiles/speculative.json
    python tools/spec_bench.py sampled [out.json] [formats]   # the sampled speculative step (spec.SpecConfig.sampled): kernel -
                                                   # vis_spec_accept_sampled next to vis_spec_accept at R = 2, 3, 4 - and step,
                                                   # per format of the comma-separated list (default: all three; "-": none), in
                                                   # one process: the plain SAMPLED step at T = 0.1, the greedy speculative step
                                                   # and the sampled speculative step at T = 0.1; the break-even of the last is
                                                   # t_R / t_1 - 1 against the plain sampled step; every time with the spread
                                                   # (min .. max) of its repeats; default out: profiles/spec_sampled.json
    python tools/spec_bench.py batch [out.json] [formats]     # the speculative step of a BATCH (spec_batch.py): synthetic:7b, per
                                                   # format (bf16, fp8; one child each), B = 2, 4, 8, 16 sequences: the plain
                                                   # batched step, then the speculative step at R = 1..4 rows per sequence
                                                   # (B * R <= 64) in the same process; t_R / t_1 - 1 = the drafts a sequence
                                                   # must get accepted per step, on average, to break even; every time
                                                   # [median, min, max] ms; default out: profiles/spec_batch.json

Every measurement runs in a child process of its own under a time limit (step: one child per format); this process never
opens the GPU.  A child that fails or runs out of time ends the run: nothing more is started on the GPU.  Times are device
events around graph replays, median of the repeats.  The weights are seeded noise: the tokens-per-step figure says what the
drafter finds in a prompt that repeats itself when the model does NOT follow it - a floor, not the acceptance of a real
checkpoint, which is unmeasured here."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernel": 240, "step": 420, "batch": 540}          # seconds per child
HQ, HKV, HD, CTX, T, V = 28, 4, 128, 2304, 2560, 152064
FORMATS = ("bf16", "fp8", "mxfp4")


def _time(run, n=20, reps=10, spread=False):
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
    if spread:
        return [round(float(v), 2) for v in (np.median(ts), min(ts), max(ts))]
    return float(np.median(ts))


def kernel_times(sampled: bool = False) -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd import hip
    dev = torch.device("cuda:0")
    nq = (HQ + 2 * HKV) * HD
    ns = -(-T // hip.DECODE_KEYS_PER_SPLIT)
    kc = torch.randn((HKV, T, HD), device=dev).to(torch.bfloat16)
    vc = torch.randn((HKV, T, HD), device=dev).to(torch.bfloat16)
    cos, sin = torch.ones((T, HD), device=dev), torch.zeros((T, HD), device=dev)
    step = torch.full((1,), CTX - 4, dtype=torch.int32, device=dev)      # never advanced: every replay does the same work
    ints = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)     # noqa: E731
    prompt = torch.randint(0, 4, (T,), dtype=torch.int32, device=dev)
    tokens = torch.randint(0, 4, (T,), dtype=torch.int32, device=dev)
    half = ints(1024)                                                   # prompt length and start of the reply: history 2300
    rows = []
    for R in (1, 2, 3, 4):
        qkv = torch.randn((R, nq), device=dev).to(torch.bfloat16)
        po = torch.empty(R * HQ * ns * HD, dtype=torch.float32, device=dev)
        pml = torch.empty(R * HQ * ns * 2, dtype=torch.float32, device=dev)
        out = torch.empty((R, HQ * HD), dtype=torch.bfloat16, device=dev)
        logits = torch.randn((R, V), device=dev)
        wv, wi = torch.empty(256 * R, device=dev), torch.empty(256 * R, dtype=torch.int32, device=dev)
        draft, nd, lim, cur, cnt = ints(1, 2, 3), ints(R - 1), ints(-1), ints(0), ints(0, 0, 0)      # limit -1: no state moves
        if sampled:      # the same logits through both accepts, each [median, min, max] of the repeats; T = 0.1, seed 1
            params = torch.from_numpy(np.array([np.float32(10.0).view(np.uint32), 1], dtype=np.uint32).view(np.int32)).to(dev)
            rows.append({"R": R, "V": V,
                         "accept_us": _time(lambda: hip.spec_accept(logits, draft, nd, lim, wv, wi, tokens, cur, step, cnt), spread=True),
                         "accept_sampled_us": _time(lambda: hip.spec_accept_sampled(logits, draft, nd, lim, wv, wi, tokens, cur, step,
                                                                                    cnt, params), spread=True)})
            print(json.dumps(rows[-1]), flush=True)
            continue
        row = {"R": R, "context": CTX,
               "attn_draft_us": round(_time(lambda: hip.decode_attn_draft(qkv, cos, sin, kc, vc, step, po, pml, out, HQ, HKV, HD,
                                                                          ns, HD ** -0.5)), 2),
               "accept_us": round(_time(lambda: hip.spec_accept(logits, draft, nd, lim, wv, wi, tokens, cur, step, cnt)), 2)}
        if R == 1:
            row["decode_attn_us"] = round(_time(lambda: hip.decode_attn(qkv[0], cos, sin, kc, vc, step, po, pml, out[0], HQ, HKV,
                                                                        HD, ns, HD ** -0.5)), 2)
        else:
            row["draft_us"] = round(_time(lambda: hip.spec_draft(prompt, half, tokens, half, step, R - 1, 4, 2, V,
                                                                 draft, nd)), 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_times(fmt: str, sampled: bool = False) -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd import weights as W
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.spec import SpecConfig
    dev = torch.device("cuda:0")
    cfg = Qwen2VLConfig.qwen2_vl_7b()
    eng = Qwen2VLEngine(cfg, W.random_device_weights(cfg, dev, 0), dev, max_ctx=1024, decode_weights=fmt)
    phrase = np.random.default_rng(0).integers(1000, 100000, 24).tolist()
    ids = [9] + phrase * 16                                      # 385 ids that repeat themselves every 24
    n, reps = 16, 5

    def timed(run, spread=False):
        ts = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) / n)
        if spread:
            return [round(float(v), 4) for v in (np.median(ts), min(ts), max(ts))]
        return float(np.median(ts))

    rows = []
    if sampled:
        return sampled_step_times(eng, fmt, ids, n, timed)
    eng.prefill(ids, [], max_new_tokens=500)
    eng.decode(4)                                                # graph capture and warm-up
    t1 = timed(lambda: eng.decode(n))
    rows.append({"format": fmt, "R": 1, "step": "plain (chained)" if eng.chain_sync is not None else "plain", "step_ms": round(t1, 4)})
    print(json.dumps(rows[-1]), flush=True)
    for R in (2, 3, 4):
        eng.prefill(ids, [], max_new_tokens=500)
        eng._spec_begin(SpecConfig(R - 1, 4, 2), 10 ** 6)
        eng._decode_steps_spec(4, R, True)
        tr = timed(lambda: eng._decode_steps_spec(n, R, True))
        toks = eng.generate(ids, [], max_new_tokens=64, ignore_eos=True, speculative=R - 1)
        t = eng.last_timing
        rows.append({"format": fmt, "R": R, "step": "speculative", "step_ms": round(tr, 4),
                     "break_even_accepted_per_step": round(tr / t1 - 1, 4),
                     "tokens_per_step_on_a_self_repeating_synthetic_prompt_noise_weights": round((len(toks) - 1) / t["spec_steps"], 3),
                     "proposed": t["spec_proposed"], "accepted": t["spec_accepted"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def sampled_step_times(eng, fmt, ids, n, timed) -> list:
    """One process: the plain sampled step (T = 0.1, seed 1), then per R the greedy speculative step and the sampled one; each
    time [median, min, max] ms."""
    from vision_inspection_system_amd.spec import SpecConfig
    T, seed = 0.1, 1
    eng.prefill(ids, [], max_new_tokens=500, temperature=T, seed=seed)
    eng.decode(4)
    t1 = timed(lambda: eng.decode(n), spread=True)
    rows = [{"format": fmt, "R": 1, "step": "plain sampled" + (" (chained)" if eng.chain_sync is not None else ""),
             "temperature": T, "step_ms": t1}]
    print(json.dumps(rows[-1]), flush=True)
    for R in (2, 3, 4):
        ts = {}
        for name, cfg, draw in (("greedy", SpecConfig(R - 1, 4, 2), {}),
                                ("sampled", SpecConfig(R - 1, 4, 2, True), dict(temperature=T, seed=seed))):
            eng.prefill(ids, [], max_new_tokens=500, **draw)
            eng._spec_begin(cfg, 10 ** 6)
            eng._decode_steps_spec(4, R, True)
            ts[name] = timed(lambda: eng._decode_steps_spec(n, R, True), spread=True)
        rows.append({"format": fmt, "R": R, "temperature": T, "speculative_greedy_step_ms": ts["greedy"],
                     "speculative_sampled_step_ms": ts["sampled"],
                     "sampled_minus_greedy_ms": round(ts["sampled"][0] - ts["greedy"][0], 4),
                     "break_even_accepted_per_step_vs_plain_sampled": round(ts["sampled"][0] / t1[0] - 1, 4)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def batch_times(fmt: str) -> list:
    """One process: per batch size the plain batched step (captured, 5 x 16 replays), then the speculative step of R rows per
    sequence.  The speculative steps run with every sequence's limit at -1: the accept launch moves no state, so every replay
    does the same work at the same positions (context ~390 keys), drafts of the prompt lookup in the rows."""
    import numpy as np
    import torch
    from vision_inspection_system_amd import spec_batch, weights as W
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.spec import SpecConfig
    dev = torch.device("cuda:0")
    cfg = Qwen2VLConfig.qwen2_vl_7b()
    eng = Qwen2VLEngine(cfg, W.random_device_weights(cfg, dev, 0), dev, max_ctx=1024, max_batch=64, decode_weights=fmt)
    phrase = np.random.default_rng(0).integers(1000, 100000, 24).tolist()
    n, reps = 16, 5

    def timed(g):
        ts = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) / n)
        return [round(float(v), 4) for v in (np.median(ts), min(ts), max(ts))]

    rows = []
    for B in (2, 4, 8, 16):
        reqs = [([9 + b] + phrase * 16, []) for b in range(B)]      # 385 ids each that repeat themselves every 24
        eng.prefill_many(reqs, max_new_tokens=600)
        assert eng._batched_step_kind(B) == "streamk"
        g = eng._batch_graph(B)
        for _ in range(4):
            g.replay()
        t1 = timed(g)
        rows.append({"format": fmt, "B": B, "R": 1, "step": "plain batched (stream-K)", "step_ms": t1})
        print(json.dumps(rows[-1]), flush=True)
        starts = [eng.slot_prompt_len[b] - 1 for b in range(B)]
        for R in (1, 2, 3, 4):
            if B * R > 64:
                continue
            sc = SpecConfig(R - 1, 4, 2)
            spec_batch.buffers(eng).begin([eng._slot_ids[b] for b in range(B)], starts, [-1] * B, 0.0, [0] * B)
            if R > 1:
                spec_batch.draft(eng, sc, B)
            gr = spec_batch.graph(eng, sc, B)
            for _ in range(4):
                gr.replay()
            tr = timed(gr)
            rows.append({"format": fmt, "B": B, "R": R, "rows": B * R, "step": "speculative batch", "step_ms": tr,
                         "t_R_over_t_1": round(tr[0] / t1[0], 4), "break_even_accepted_per_step": round(tr[0] / t1[0] - 1, 4)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def _child(what: str, arg: str) -> None:
    from vision_inspection_system_amd import hip
    hip.load()
    if what == "batch":
        print("RESULT " + json.dumps(batch_times(arg)), flush=True)
        return
    if what.endswith("_sampled"):
        rows = kernel_times(True) if what == "kernel_sampled" else step_times(arg, True)
    else:
        rows = kernel_times() if what == "kernel" else step_times(arg)
    print("RESULT " + json.dumps(rows), flush=True)


def _run_child(what: str, arg: str = "-") -> list:
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, arg], stdout=subprocess.PIPE, text=True,
                           timeout=LIMITS[what.split("_")[0]])
    except subprocess.TimeoutExpired:
        raise SystemExit(f"spec_bench {what} {arg}: no result within {LIMITS[what.split('_')[0]]} s - stopping")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        raise SystemExit(f"spec_bench {what} {arg}: the child ended with status {p.returncode} - stopping")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        _child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what not in ("kernel", "step", "all", "sampled", "batch"):
        raise SystemExit(__doc__)
    default = {"sampled": "spec_sampled.json", "batch": "spec_batch.json"}.get(what, "speculative.json")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", default)
    result = {}
    if what == "batch":
        fmts = sys.argv[3].split(",") if len(sys.argv) > 3 else ["bf16", "fp8"]
        if any(f not in ("bf16", "fp8") for f in fmts):
            raise SystemExit(__doc__)
        result["times"] = "[median, min, max] of 5 repeats of 16 replayed steps (ms); synthetic:7b, context ~390 keys per sequence"
        result["acceptance_on_a_real_checkpoint"] = "not measured"
        result["batch"] = [row for fmt in fmts for row in _run_child("batch", fmt)]
        result["formats_not_measured"] = [f for f in ("bf16", "fp8") if f not in fmts]
    if what == "sampled":
        fmts = [f for f in (sys.argv[3].split(",") if len(sys.argv) > 3 else FORMATS) if f != "-"]
        if any(f not in FORMATS for f in fmts):
            raise SystemExit(__doc__)
        result["times"] = "[median, min, max] of the repeats: kernel 10 x 20 replayed launches (us), step 5 x 16 replayed steps (ms)"
        result["kernel"] = [r for r in _run_child("kernel_sampled") if r["R"] > 1]
        result["step"] = [row for fmt in fmts for row in _run_child("step_sampled", fmt)]
        result["step_formats_not_measured"] = [f for f in FORMATS if f not in fmts]
    if what in ("kernel", "all"):
        result["kernel"] = _run_child("kernel")
    if what in ("step", "all"):
        result["step"] = [row for fmt in FORMATS for row in _run_child("step", fmt)]
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
