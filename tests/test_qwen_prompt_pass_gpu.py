"""The Inspector's prompt pass on MI355X against the record of the commit that still carried it twice (a single-request pass
next to a group pass, the decoder layer body written four times): for every configuration of
tests/golden/gen_qwen_prompt_pass.py the result bytes - caches, rope rows, logits, taps, prefix bundle, tokens - are those of
tests/golden/qwen_prompt_pass.json, and so are the library calls, entry by entry and argument by argument.

One difference is permitted, and only in the configurations where ``prefill`` runs the tower itself (TOWER_IN_PREFILL: the
single requests with frames, and prefill_many on one stream, which a batch of one request is too): the recorded commit issued
a request's embedding gather (vis_gather_rows) in front of its tower's calls, the one pass issues it behind them.  There the
golden is compared with that one call moved to just in front of the request's vis_scatter_rows; nothing else may move or
differ, and no argument may differ.  The JSON is never regenerated for this: it is the earlier commit's record."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_qwen_prompt_pass as T  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "qwen_prompt_pass.json")) as _f:
    GOLDEN = json.load(_f)

TOWER_IN_PREFILL = {"single_image", "single_two_images", "single_slot1", "single_fp8", "single_pairs_off",
                    "single_prefix_pairs_off", "single_prefix", "single_prefix_fp8", "single_wide", "single_wide_fp8",
                    "many_1", "many_3_one_stream"}


def gather_behind_tower(calls: list) -> list:
    """The golden's calls with, for every vis_scatter_rows, the request's vis_gather_rows (the last one in front of it) moved
    to just in front of it."""
    out, last_gather = [], None
    for c in calls:
        if c.startswith("vis_scatter_rows("):
            assert last_gather is not None, "a scatter without a gather in front of it"
            out.append(out.pop(last_gather))
            last_gather = None
        elif c.startswith("vis_gather_rows("):
            last_gather = len(out)
        out.append(c)
    return out


def test_gather_behind_tower_moves_that_call_only():
    calls = ["vis_gather_rows(1)", "vis_gemm_bf16(p)", "vis_gather_rows(2)", "vis_patchify_u8(a)", "vis_gemm_bf16(t)",
             "vis_scatter_rows(2)", "vis_gemm_bf16(q)", "vis_gather_rows(3)", "vis_gemv_bf16(x)"]
    assert gather_behind_tower(calls) == [
        "vis_gather_rows(1)", "vis_gemm_bf16(p)", "vis_patchify_u8(a)", "vis_gemm_bf16(t)", "vis_gather_rows(2)",
        "vis_scatter_rows(2)", "vis_gemm_bf16(q)", "vis_gather_rows(3)", "vis_gemv_bf16(x)"]


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
        diff = T.first_difference(g, gather_behind_tower(w) if name in TOWER_IN_PREFILL else w)
        assert not diff, f"{name}, thread {t}: {diff}"
