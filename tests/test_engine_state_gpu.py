"""What an engine holds right after construction, on MI355X: for every configuration of tests/golden/gen_engine_state.py
(both engines; 1, 4 and 6 slots; bf16, fp8 and MXFP4 decode weights; the fused, fold and chain switches; the fp8 prompt pass,
the fp8 cross-attention keys, the speculative Auditor) the flattened ``vars(engine)`` - every tensor's shape, strides, dtype,
storage and offset, every plain value - is that of tests/golden/engine_state.json, recorded before the decode stage took
over the allocation; the storages the engine holds take no more bytes than they did then; and every buffer the
constructors zero-initialise is all zero.  A change that is meant to alter what an engine allocates re-runs the generator."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_engine_state as G  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "engine_state.json")) as _f:
    GOLDEN = json.load(_f)["configs"]

ABSENT, TENSOR = "<absent>", "<a tensor>"


def _mllama_rows_only(c, want):
    return c["model"] == "mllama" and c["engine"].get("decode_weights") == "mxfp4" and "mxfp4_gemm_from" not in c["engine"]


def _chain_was_off(c, want):
    return want.get("chain_sync") == "None"


# The differences from the golden that are meant: (path, in the golden, now, where [None: everywhere], why).
ALLOWED = [
    ("streamk_part", ABSENT, "True", None, "the one b_part rule's result, kept as a flag: the slabs exist"),
    ("streamk_part", ABSENT, "False", None, "the one b_part rule's result, kept as a flag: no step reads the slabs"),
    ("b_part", TENSOR, ABSENT, _mllama_rows_only, "Mllama allocated the slabs unconditionally; with MXFP4 weights and no "
                                                  "mxfp4_gemm_from every batch size is the rows step's, which never reads them"),
    ("chain_ws", ABSENT, "None", None, "None instead of absent on an engine without the chained step"),
    ("chain_ws", TENSOR, "None", _chain_was_off, "Qwen2-VL kept the workspace when the context limit came out non-positive"),
    ("kpad", ABSENT, "None", None, "None instead of absent where no fp8 MFMA reads the down projection"),
    ("q8_lm_head", ABSENT, "None", None, "None instead of absent on an engine without e4m3 weights"),
    ("q4_lm_head", ABSENT, "None", None, "None instead of absent on an engine without MXFP4 weights"),
    ("last_timing", ABSENT, "dict[0]", None, "Mllama set it with its first request; empty instead of absent until then"),
    ("_prefill_streams", ABSENT, "list[0]", None, "Mllama made the list on first use; empty instead of absent until then"),
]

# Zero-initialised by the constructors at the commit the golden names (torch.zeros there): caches, counters and token rows,
# the per-slot rope rows (Qwen2-VL), the cross-attention keys / values, their e4m3 copies and key counts (Mllama), the fp8
# activation rows and scales, the fused step's sums of squares and workspace, the chain's workspace and sync block.
ZEROED = ("kcache_b", "vcache_b", "step_b", "cur_b", "tokens_b", "cos_b", "sin_b", "xk_b", "xv_b", "xkq_b", "xvq_b", "xks_b",
          "xvs_b", "nkeys_b", "b_xq", "b_x2q", "b_actq", "b_sx", "b_xqs", "b_x2qs", "b_actqs", "b_ssq1", "b_ssq2", "b_proj_ws",
          "chain_ws", "chain_sync")


def _meant(c, want, path, w, g) -> bool:
    w = TENSOR if " strides " in w else w
    return any(path == p and w == was and g == now and (where is None or where(c, want)) for p, was, now, where, _ in ALLOWED)


def test_golden_covers_every_configuration():
    assert sorted(GOLDEN) == sorted(G.CONFIGS)


@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_engine_state_matches_golden(device, name):
    c, want = G.CONFIGS[name], GOLDEN[name]["state"]
    eng, alloc = G.build(name, device)
    got = G.flatten(eng)
    diffs = []
    for path in sorted(set(want) | set(got)):
        w, g = want.get(path, ABSENT), got.get(path, ABSENT)
        if w != g and not _meant(c, want, path, w, g):
            diffs.append(f"{path}: golden {w} | now {g}")
    assert not diffs, f"{name}: {len(diffs)} differences\n" + "\n".join(diffs)
    # device memory: the bytes of the storages the engine holds (what memory_allocated() grew by depends on the blocks the
    # caching allocator has lying around: printed, not asserted)
    print(f"{name}: {G.storage_bytes(got)} bytes of storages, {G.storage_bytes(want)} in the golden; memory_allocated() "
          f"grew by {alloc}, {GOLDEN[name]['alloc_bytes']} when the golden was recorded")
    assert G.storage_bytes(got) <= G.storage_bytes(want)
    tensors = G.tensors_of(eng)
    present = [n for n in ZEROED if tensors.get(n) is not None]
    assert {"kcache_b", "vcache_b", "step_b", "cur_b", "tokens_b"} <= set(present)
    dirty = [n for n in present if bool(tensors[n].any())]
    assert not dirty, f"{name}: not all zero after construction: {dirty}"
    pads = [p for p in tensors if p.startswith("dec_layers[") and p.endswith(".down_w_pad[0]")]
    assert bool(pads) == (getattr(eng, "kpad", None) is not None and eng.kpad != eng.cfg.intermediate)
    for p in pads:      # the codes, then zero columns up to kpad
        assert tensors[p].shape[1] == eng.kpad and not bool(tensors[p][:, eng.cfg.intermediate:].any())
        assert bool((tensors[p][:, :eng.cfg.intermediate] == tensors[p.replace("down_w_pad", "down_w")]).all())
