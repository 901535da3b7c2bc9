"""The six decode-step cross-attention entry points against bits recorded from the commit named in
tests/golden/cross_attn_bits.json (tests/golden/gen_cross_attn_bits.py, run once with VIS_HIP_LIB on that commit's build):
single, batch (B = 3, own counts, a batch stride that skips a layer; bf16 in both the split and the streaming form) and draft
(R = 1..4 while R * G <= 16, q the leading columns of packed rows) over 192 key rows at counts 1, 64, 65, 191, 192, every
instantiated group size, bf16 and fp8 keys.  The draft-row == single-row test of tests/test_auditor_spec_gpu.py says that a
column does not depend on the others; this one says the bits are the recorded ones."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_cross_attn_bits", os.path.join(GOLDEN, "gen_cross_attn_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = gen.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "cross_attn_bits.json")) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_the_recorded_ones(device, recorded, case):
    from vision_inspection_system_amd import hip
    hip.load()
    cid, fmt, Hq, Hkv, form, stream = case
    want = recorded[cid]
    got = gen.run_case(hip, device, fmt, Hq, Hkv, form, stream)
    assert sorted(got) == sorted(want), "the generator's launches of this case are not the recorded ones"
    for sub in got:
        assert got[sub]["in"] == want[sub]["in"], f"{cid} {sub}: the generator no longer builds the recorded INPUTS (not a kernel fault)"
    for sub in got:
        for key in ("out", "part_o", "part_ml"):
            assert got[sub].get(key) == want[sub].get(key), f"{cid} {sub}: {key} differs from the recorded bits"
