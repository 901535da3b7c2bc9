"""What the prefill attention kernels' K-tile loads read past the last key.

csrc/attn_tile_dma.hip.h holds the one buffer LDS-DMA helper that attn_vit32_kernel and attn_prefill_pair_kernel stage their
tiles with.  tools/probes/buffer_range_probe.hip (built next to the library as csrc/buffer_range_probe) calls that helper on a
buffer of its own: data below the descriptor's num_records, a poison word behind it, every address it can form asserted on the
host to lie inside its allocation.  The recorded output of an MI355X run is profiles/buffer_range_probe.txt.

The extra keys of a ragged last tile are masked with a select, so no output test can see whether their rows were zeros or the
memory behind the head; this test reads the LDS image itself.
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "buffer_range_probe")
ROW_BYTES = (160, 256)          # K rows of the head_dim 80 and the head_dim 128 kernel


def _cases(text):
    out = {}
    for m in re.finditer(r"^CASE (\w+) (.*)$", text, re.M):
        out[m.group(1)] = {k: int(v) for k, v in (kv.split("=") for kv in m.group(2).split())}
    return out


def test_tile_loads_never_return_memory_past_num_records():
    """One run of the probe (a child process, one wave per launch, eight launches).  Per row size:
    a  scalar and vector offset in range: every piece is the data at its address;
    b  vector offsets that straddle num_records: data below, zeros from num_records on - the documented check every descriptor
       user in this library relies on;
    d  the load form the kernels use on a ragged last tile (the tile's position in the scalar offset, the sum straddles
       num_records): data below, and NO piece past num_records is poison - all of them are zeros;
    c  the scalar offset alone past num_records: zeros as well.
    Measured on the MI355X: `soffset range-checked: yes` (profiles/buffer_range_probe.txt).  Were it `no`, d would fail here until
    att_tile_dma16 put the tile's position into the vector offset on that tile."""
    assert os.path.exists(PROBE), f"{PROBE} is missing: make -C vision-inspection-system_amd/csrc builds it"
    r = subprocess.run([PROBE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, f"buffer_range_probe exited with {r.returncode}:\n{r.stdout}"
    verdict = re.findall(r"^soffset range-checked: (yes|no)$", r.stdout, re.M)
    assert len(verdict) == 1, r.stdout
    cases = _cases(r.stdout)
    for rb in ROW_BYTES:
        a, b, c, d = (cases[f"{name}{rb}"] for name in "abcd")
        assert a["past"] == 0 and a["in"] == 64 and a["in_data"] == 64, (rb, a, r.stdout)
        assert b["in"] == 32 and b["in_data"] == 32 and b["past"] == 32 and b["past_zeros"] == 32, (rb, b, r.stdout)
        assert d["in"] > 0 and d["in_data"] == d["in"], (rb, d, r.stdout)
        assert d["past"] >= 32 and d["past_poison"] == 0 and d["past_zeros"] == d["past"], (rb, d, r.stdout)
        assert c["in"] == 0 and c["past"] == 64 and c["past_poison"] == 0 and c["past_zeros"] == 64, (rb, c, r.stdout)
    assert verdict == ["yes"], r.stdout
