"""The decode step's launch transcript on MI355X: for every configuration of tests/golden/gen_decode_transcript.py (both
engines; single sequence and batched; bf16, fp8 and MXFP4 weights; chained, GEMV, multi-row, stream-K and fused steps) the
library calls of two consecutive eager decode steps - entry, arguments, buffers, order - are exactly those of
tests/golden/decode_transcript.json.  A change that is meant to alter the step's launches re-runs the generator."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_decode_transcript as T  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "decode_transcript.json")) as _f:
    GOLDEN = json.load(_f)["configs"]


def test_golden_covers_every_configuration():
    assert sorted(GOLDEN) == sorted(T.CONFIGS)


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_decode_step_calls_match_golden(device, name):
    got = T.record(name, device)
    assert got["chained"] == GOLDEN[name]["chained"]
    diff = T.first_difference(got["calls"], GOLDEN[name]["calls"])
    assert not diff, f"{name}: {diff}"
