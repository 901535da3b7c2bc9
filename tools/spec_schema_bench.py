"""Cost of the speculative step under a JSON Schema (spec.py "grammar") on the MI355X, and the acceptance at which it pays.

    python tools/spec_schema_bench.py kernel [out.json]   # vis_schema_mask_rows at R = 1..4 next to vis_schema_mask at one row
                                                          # (report schema, V = 152064, four states); vis_spec_accept_masked
                                                          # next to vis_spec_accept at R = 2, 3, 4; vis_spec_draft_schema
    python tools/spec_schema_bench.py step [out.json]     # synthetic:7b under the report schema, one process: the plain
                                                          # schema-constrained step, then the speculative step at R = 2 / 4
                                                          # with the schema's drafts; t_R / t_1 - 1 = the accepted drafts per
                                                          # step at which it breaks even
    python tools/spec_schema_bench.py all [out.json]      # both; default out: profiles/spec_schema.json

Every measurement runs in a child process of its own under a time limit; this process never opens the GPU.  A child that
fails or runs out of time ends the run: nothing more is started on the GPU, and what was not run is written as "not
measured".  kernel: tools/json_mode_bench.py's synthetic vocabulary and timing (50 launches captured in one graph, replayed
20 times, device events, median us per launch; the launches re-fold nothing, as in steady state).  step: device events
around 16 replayed steps, [median, min, max] ms of 5 repeats.  The weights are seeded noise: what share of a real
checkpoint's drafts is accepted cannot be measured here - only the schema's share of forced bytes (schema_draft.simulate on
any reply) and the break-even above can."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"kernel": 300, "step": 480}          # seconds per child
V = 152064
STATES = {"start": b"", "after_key": b'{"object_identified"', "in_string": b'{"object_identified":"a steel bo',
          "in_enum": b'{"object_identified":"bolt","overall_condition":"da'}


def kernel_times() -> list:
    import numpy as np
    import torch
    from json_mode_bench import _Vocab, _time_graph
    from vision_inspection_system_amd import hip, schema_draft
    from vision_inspection_system_amd import json_grammar as G
    from vision_inspection_system_amd import json_schema as S
    from vision_inspection_system_amd.schemas import REPORT_SCHEMA
    dev = torch.device("cuda:0")
    dfa = S.compile_schema(REPORT_SCHEMA)
    table = G.build_token_table(_Vocab(V), V, [V - 1])
    dt = [torch.from_numpy(a).to(dev) for a in (table.off, table.data, table.flags, table.eos_ids)]
    header = torch.tensor([dfa.n_states, dfa.n_classes, dfa.start, 0], dtype=torch.int32, device=dev)
    trans = torch.full((S.SCHEMA_MAX_STATES, S.SCHEMA_MAX_CLASSES), -1, dtype=torch.int16, device=dev)
    trans.view(-1)[:dfa.trans.size].copy_(torch.from_numpy(dfa.trans.reshape(-1).view(np.int16).copy()))
    cls = torch.from_numpy(dfa.byte_class.copy()).to(dev)
    sflags = torch.zeros(S.SCHEMA_MAX_STATES, dtype=torch.uint8, device=dev)
    sflags[:dfa.n_states].copy_(torch.from_numpy(dfa.state_flags.copy()))
    tables = schema_draft.build(dfa, table)
    jt, jn = torch.from_numpy(tables.jump_tok).to(dev), torch.from_numpy(tables.jump_next).to(dev)
    ints = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
    nw = (V + 63) // 64
    rows = [{"schema": "report", "states": dfa.n_states, "V": V,
             "states_with_a_draft": int((tables.jump_tok >= 0).sum())}]
    for name, prefix in STATES.items():
        P, s = len(prefix), S.walk(dfa, dfa.start, prefix)
        tokens = torch.zeros(64, dtype=torch.int32, device=dev)
        tokens[:P] = ints(*prefix) if P else tokens[:0]
        step = ints(P)
        sstate = torch.zeros((1, S.STATE_INTS), dtype=torch.int32)
        for slot in (0, 1):
            sstate[0, slot * S.SLOT_INTS + S.STATE], sstate[0, slot * S.SLOT_INTS + S.POS] = s, P
            sstate[0, slot * S.SLOT_INTS + S.ANCHOR] = 1
        sstate = sstate.to(dev)
        allow1 = torch.zeros((1, nw), dtype=torch.int64, device=dev)
        row = {"state": name, "schema_mask_us": round(_time_graph(lambda: hip.schema_mask(
            sstate, tokens.view(1, -1), step, *dt, allow1, header, trans, cls, sflags)), 2)}
        # drafts that keep every row live: the schema's own where it has them, else allowed single bytes
        draft, st = [], s
        for _ in range(3):
            t = int(tables.jump_tok[st])
            if t < 0:
                ok, _ = S.allowed(dfa, [st, 0], table)
                t = int(np.flatnonzero(ok & (table.flags == 0))[0])
            draft.append(t)
            st = S.walk(dfa, st, table.tokens[t])
        for R in (1, 2, 3, 4):
            rec = ints(*([s, 0, P, 1] + [0] * 28))
            allow = torch.zeros((R, nw), dtype=torch.int64, device=dev)
            d, nd = ints(*draft), ints(R - 1)
            row[f"mask_rows_R{R}_us"] = round(_time_graph(lambda: hip.schema_mask_rows(
                rec, tokens, step, d, nd, *dt, allow, header, trans, cls, sflags)), 2)
            assert (allow != 0).any(dim=1).all()
        rec, d, nd = ints(*([s, 0, P, 1] + [0] * 28)), ints(0, 0, 0), ints(0)
        row["draft_schema_us"] = round(_time_graph(lambda: hip.spec_draft_schema(
            rec, tokens, step, dt[0], dt[1], dt[2], header, trans, cls, sflags, jt, jn, 3, d, nd)), 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    tokens, step = torch.zeros(2560, dtype=torch.int32, device=dev), ints(2300)
    for R in (2, 3, 4):
        logits = torch.randn((R, V), device=dev)
        wv, wi = torch.empty(256 * R, device=dev), torch.empty(256 * R, dtype=torch.int32, device=dev)
        draft, nd, lim, cur, cnt = ints(1, 2, 3), ints(R - 1), ints(-1), ints(0), ints(0, 0, 0)      # limit -1: no state moves
        params = torch.from_numpy(np.array([np.float32(10.0).view(np.uint32), 1], dtype=np.uint32).view(np.int32)).to(dev)
        row = {"R": R, "V": V, "accept_us": round(_time_graph(lambda: hip.spec_accept(
            logits, draft, nd, lim, wv, wi, tokens, cur, step, cnt)), 2)}
        for kind, frac in (("a_tenth_allowed", 0.1), ("all_allowed", 1.0)):
            bits = torch.rand((R, nw * 64), device=dev) < frac
            w = (bits.view(R, nw, 64).to(torch.int64) << torch.arange(64, device=dev)).sum(dim=2)
            row[f"accept_masked_{kind}_us"] = round(_time_graph(lambda: hip.spec_accept_masked(
                logits, draft, nd, lim, wv, wi, tokens, cur, step, cnt, w)), 2)
            row[f"accept_masked_sampled_{kind}_us"] = round(_time_graph(lambda: hip.spec_accept_masked(
                logits, draft, nd, lim, wv, wi, tokens, cur, step, cnt, w, params)), 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_times() -> list:
    import numpy as np
    import torch
    from vision_inspection_system_amd import json_schema as S
    from vision_inspection_system_amd.client import get_model
    from vision_inspection_system_amd.schemas import REPORT_SCHEMA
    from vision_inspection_system_amd.spec import SpecConfig
    eng = get_model("synthetic:7b", "cuda:0").engine
    dfa = S.compile_schema(REPORT_SCHEMA)
    ids = np.random.default_rng(0).integers(0, 150000, 1289).tolist()
    n, reps = 16, 5

    def timed(run):
        ts = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) / n)
        return [round(float(v), 4) for v in (np.median(ts), min(ts), max(ts))]

    rows = []
    with eng._pick_request(None, False, dfa, None, False, None):
        eng.prefill(ids, [], max_new_tokens=600)
        eng.decode(4)                                                # graph capture and warm-up
        t1 = timed(lambda: eng.decode(n))
        rows.append({"R": 1, "step": "plain, json_schema" + (" (chained)" if eng.chain_sync is not None else ""), "step_ms": t1})
        print(json.dumps(rows[-1]), flush=True)
        for R in (2, 4):
            eng.prefill(ids, [], max_new_tokens=600)
            eng._spec_begin(SpecConfig(R - 1, 4, 2, False, True), 10 ** 6)
            eng._decode_steps_spec(4, R, True)
            tr = timed(lambda: eng._decode_steps_spec(n, R, True))
            rows.append({"R": R, "step": "speculative, grammar + schema_drafts", "step_ms": tr,
                         "break_even_accepted_per_step": round(tr[0] / t1[0] - 1, 4)})
            print(json.dumps(rows[-1]), flush=True)
    # what the schema drafts of one reply of these noise weights (model-free counters; not a checkpoint's acceptance)
    toks = eng.generate(ids, [], max_new_tokens=96, ignore_eos=True, json_schema=dfa,
                        speculative={"num_speculative_tokens": 3, "grammar": True})
    t = eng.last_timing
    rows.append({"reply_tokens": len(toks), "spec_steps": t["spec_steps"], "spec_proposed": t["spec_proposed"],
                 "spec_accepted": t["spec_accepted"], "note": "noise weights: the reply's free text is noise, its forced bytes are not"})
    print(json.dumps(rows[-1]), flush=True)
    return rows


def _run_child(what: str):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], stdout=subprocess.PIPE, text=True,
                           timeout=LIMITS[what])
    except subprocess.TimeoutExpired:
        return None, f"no result within {LIMITS[what]} s"
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        return None, f"the child ended with status {p.returncode}"
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]), None


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        from vision_inspection_system_amd import hip
        hip.load()
        print("RESULT " + json.dumps(kernel_times() if sys.argv[2] == "kernel" else step_times()), flush=True)
        sys.exit(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what not in ("kernel", "step", "all"):
        raise SystemExit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "spec_schema.json")
    result = {"times": "kernel: median us per launch of 20 x 50 replayed launches; step: [median, min, max] ms of 5 x 16 replayed steps",
              "kernel": "not measured", "step": "not measured",
              "acceptance_on_a_real_checkpoint": "not measured (the weights here are seeded noise)"}
    failed = None
    for part in ("kernel", "step"):
        if what in (part, "all") and failed is None:
            rows, failed = _run_child(part)
            if rows is not None:
                result[part] = rows
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    if failed:
        raise SystemExit(f"spec_schema_bench: {failed} - stopped")
