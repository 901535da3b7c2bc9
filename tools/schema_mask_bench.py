"""Cost of schema-constrained decoding (vis_schema_mask) next to JSON mode (vis_json_mask) on the MI355X.

    python tools/schema_mask_bench.py kernel [out.json]   # both masks, V = 152064 / 128256, B = 1 / 16 / 64, four states
    python tools/schema_mask_bench.py step [out.json]     # synthetic:7b decode step: mask off / json_object / json_schema

kernel: tools/json_mode_bench.py's synthetic vocabulary and timing (50 launches captured in one graph, replayed 20 times
after a warm-up, device events, median us per launch; the launch re-folds nothing, as in steady state).  The schema is the
agents' report schema (schemas.REPORT_SCHEMA); each state is reached by a prefix of one report, and BOTH kernels are timed
on that same prefix, the same token table and the same rows: after-key (only ':' and whitespace survive the first byte),
value-start (for the schema: the start of an enum value - a handful of tokens; for JSON mode any value), in-string (every
token walked or taken by the PLAIN fast path) and in-enum (for JSON mode an ordinary string body).  Also reports the
schema's compile time and table size.
step: json_mode_bench.py's decode-step measurement with a third mode, the report schema."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from json_mode_bench import _Vocab, _time_graph  # noqa: E402
from vision_inspection_system_amd import hip  # noqa: E402
from vision_inspection_system_amd import json_grammar as G  # noqa: E402
from vision_inspection_system_amd import json_schema as S  # noqa: E402
from vision_inspection_system_amd.schemas import REPORT_SCHEMA  # noqa: E402

DEV = torch.device("cuda:0")
STATES = {"after_key": b'{"object_identified"', "value_start": b'{"object_identified":"bolt","overall_condition":',
          "in_string": b'{"object_identified":"a steel bo', "in_enum": b'{"object_identified":"bolt","overall_condition":"da'}


def _bits(row: torch.Tensor) -> int:
    return int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in row.cpu().tolist()))


def kernel_times() -> list:
    t0 = time.perf_counter()
    dfa = S.compile_schema(REPORT_SCHEMA)
    rows = [{"schema": "report", "compile_s": round(time.perf_counter() - t0, 3), "states": dfa.n_states,
             "classes": dfa.n_classes, "table_bytes": dfa.table_bytes, "max_ws": S.SCHEMA_MAX_WS}]
    print(json.dumps(rows[-1]), flush=True)
    header = torch.tensor([dfa.n_states, dfa.n_classes, dfa.start, 0], dtype=torch.int32, device=DEV)
    trans = torch.full((S.SCHEMA_MAX_STATES, S.SCHEMA_MAX_CLASSES), -1, dtype=torch.int16, device=DEV)
    trans.view(-1)[:dfa.trans.size].copy_(torch.from_numpy(dfa.trans.reshape(-1).view(np.int16).copy()))
    cls = torch.from_numpy(dfa.byte_class.copy()).to(DEV)
    sflags = torch.zeros(S.SCHEMA_MAX_STATES, dtype=torch.uint8, device=DEV)
    sflags[:dfa.n_states].copy_(torch.from_numpy(dfa.state_flags.copy()))
    for V in (152064, 128256):
        table = G.build_token_table(_Vocab(V), V, [V - 1])
        dt = [torch.from_numpy(a).to(DEV) for a in (table.off, table.data, table.flags, table.eos_ids)]
        for B in (1, 16, 64):
            for name, prefix in STATES.items():
                P = len(prefix)
                tokens = torch.zeros((B, 64), dtype=torch.int32, device=DEV)
                step = torch.full((B,), P, dtype=torch.int32, device=DEV)
                allow = torch.zeros((B, (V + 63) // 64), dtype=torch.int64, device=DEV)
                jst = G.accepts(G.initial_state(), prefix)
                sst = S.walk(dfa, dfa.start, prefix)
                assert jst is not None and sst != S.DEAD, name
                jstate = torch.zeros((B, G.STATE_INTS), dtype=torch.int32)
                sstate = torch.zeros((B, S.STATE_INTS), dtype=torch.int32)
                for s in (0, 1):            # both parity slots hold the folded state: every launch re-reads it
                    jstate[:, s * G.SLOT_INTS:s * G.SLOT_INTS + G.LEX_WORDS] = torch.tensor(jst[:G.LEX_WORDS])
                    jstate[:, s * G.SLOT_INTS + G.POS] = P
                    jstate[:, s * G.SLOT_INTS + G.ANCHOR] = 1
                    sstate[:, s * S.SLOT_INTS + S.STATE] = sst
                    sstate[:, s * S.SLOT_INTS + S.POS] = P
                    sstate[:, s * S.SLOT_INTS + S.ANCHOR] = 1
                jstate, sstate = jstate.to(DEV), sstate.to(DEV)
                us_j = _time_graph(lambda: hip.json_mask(jstate, tokens, step, *dt, allow))
                n_j = _bits(allow[0])
                us_s = _time_graph(lambda: hip.schema_mask(sstate, tokens, step, *dt, allow, header, trans, cls, sflags))
                n_s = _bits(allow[0])
                rows.append({"V": V, "B": B, "state": name, "json_mask_us": round(us_j, 2), "schema_mask_us": round(us_s, 2),
                             "json_allowed": n_j, "schema_allowed": n_s})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def step_times() -> list:
    from vision_inspection_system_amd.client import get_model
    eng = get_model("synthetic:7b", "cuda:0").engine
    dfa = S.compile_schema(REPORT_SCHEMA)
    rng = np.random.default_rng(0)
    modes = ["off", "json_object", "json_schema"]

    def begin(m):
        eng._begin_schema(False, dfa if m == "json_schema" else None)
        eng._begin_json(m == "json_object")

    out = []
    ids = rng.integers(0, 150000, 1289).tolist()
    res = {m: [] for m in modes}
    for _ in range(5):
        for m in modes:
            begin(m)
            eng.prefill(ids, [], max_new_tokens=64)
            eng.decode(4)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.decode(48)
            e.record()
            torch.cuda.synchronize()
            res[m].append(s.elapsed_time(e) / 48)
    begin("off")
    for m in modes:
        out.append({"B": 1, "mask": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    B = 64
    reqs = [(rng.integers(0, 150000, 1289).tolist(), []) for _ in range(B)]
    res = {m: [] for m in modes}
    for m in modes:     # one phase per mode, each after its own prompt passes (a mask resets the slots' grammar states)
        begin(m)
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
    begin("off")
    for m in modes:
        out.append({"B": B, "mask": m, "ms_per_step": round(float(np.median(res[m])), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    hip.load()
    rows = kernel_times() if what == "kernel" else step_times()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)
