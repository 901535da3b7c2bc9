"""The Auditor's prompt pass on MI355X against the record of the commit that still carried it twice (a single pass next to a
group pass, a single-image tower next to a stacked one): for every configuration of tests/golden/gen_mllama_prompt_pass.py the
result bytes - tower output, caches, cross-attention rows, logits, taps, tokens - are those of
tests/golden/mllama_prompt_pass.json, and so are the library calls, entry by entry and argument by argument.

One difference is permitted, and only in the configurations that run the tower over a SINGLE image (every ``single_*``, ``many_1``,
and ``many_2_one_stream``, whose one stream leaves every request its own tower): an image owns round_up(N, 64) rows of the
stack for every stack size, so the row count of the tower's row-wise launches is NS where the single-image tower passed N.
ROW_ARGS lists, per entry, the argument positions that may carry it; there the golden must say N and the run NS, and nothing
else may differ.  The JSON is never regenerated for this: it is the earlier commit's record."""
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_mllama_prompt_pass as T  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "mllama_prompt_pass.json")) as _f:
    GOLDEN = json.load(_f)

SINGLE_IMAGE_TOWER = {"single_image", "single_text", "single_slot1", "single_cross_fp8", "many_1", "many_2_one_stream"}
# entry -> positions of the arguments that are the tower's row count: rows of the norm and of add_rows, M of the GEMM, S and the
# key rows T of the q / k split and of the attention.  Leading dimensions do not change: V^T already had round_up(N, 64) columns.
ROW_ARGS = {"vis_layernorm_bf16": (4,), "vis_gemm_bf16": (5,), "vis_qkv_rope_split": (7, 12), "vis_attn_prefill_rows": (9, 10),
            "vis_add_rows_bf16": (3,)}


def _tower_rows():
    from vision_inspection_system_amd.mllama_weights import MllamaConfig
    cfg = MllamaConfig.tiny()
    n = cfg.max_tiles * (cfg.tile_tokens + (8 - cfg.tile_tokens % 8) % 8)
    return n, (n + 63) // 64 * 64


def _split(call: str):
    name, args = re.fullmatch(r"(\w+)\((.*)\)", call).groups()
    return name, args.split(", ")


def call_difference(got: list, want: list, single_image_tower: bool) -> str:
    """'' when the two call lists agree (up to the permitted row count), else a sentence naming the first call that does not."""
    n, ns = _tower_rows()
    if len(got) != len(want):
        return T.first_difference(got, want) or f"{len(got)} calls now, {len(want)} in the golden"
    for i, (a, b) in enumerate(zip(got, want)):
        if a == b:
            continue
        (name_a, args_a), (name_b, args_b) = _split(a), _split(b)
        where = [p for p, (x, y) in enumerate(zip(args_a, args_b)) if x != y]
        allowed = single_image_tower and n != ns and name_a == name_b and len(args_a) == len(args_b) \
            and set(where) <= set(ROW_ARGS.get(name_a, ())) and all(args_b[p] == str(n) and args_a[p] == str(ns) for p in where)
        if not allowed:
            return f"call {i} differs:\n  recorded now: {a}\n  golden:       {b}"
    return ""


def test_golden_covers_every_configuration():
    assert sorted(GOLDEN["configs"]) == sorted(T.CONFIGS)


def test_synthetic_weights_are_those_of_the_record(device):
    assert T.weight_digest(device) == GOLDEN["weights"], \
        "synth_state_dict(cfg, seed=0) / pack_device_weights give other weights than when the golden was recorded: every digest " \
        "below will differ for that reason, not because the prompt pass changed"


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_prompt_pass_matches_the_record(device, name):
    assert T.weight_digest(device) == GOLDEN["weights"], "other synthetic weights than the golden's (see the test above)"
    got, want = T.record(name, device), GOLDEN["configs"][name]
    assert got["tokens"] == want["tokens"]
    assert got["digests"] == want["digests"]
    assert len(got["calls"]) == len(want["calls"]), "another number of issuing threads"
    for t, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        diff = call_difference(g, w, name in SINGLE_IMAGE_TOWER)
        assert not diff, f"{name}, thread {t}: {diff}"
