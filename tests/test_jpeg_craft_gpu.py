"""Crafted-JPEG parity on the GPU: every crafted file (tests/jpeg_craft.py) that the host parser accepts goes through
vis_jpeg_to_rgb and must equal PIL's decode of the same bytes bit for bit - samples beyond [-512, 511] (the kernel
saturates, as libjpeg-turbo's SIMD code does), saturated chroma under every subsampling, 1x1 and odd sizes.  Files the
parser declines for range never reach the kernel: the CPU test (tests/test_jpeg_craft.py) asserts the reason."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_craft as JC
from vision_inspection_system_amd import jpeg as J

pytestmark = pytest.mark.gpu

CASES = JC.crafted_cases()


def test_every_accepted_crafted_file_equals_pil_on_the_gpu(device):
    decoded = out_of_range = 0
    for case in CASES:
        jc, reason = J.parse_status(case.data)
        if jc is None:
            assert reason == "range", case.name
            continue
        ref = np.array(Image.open(io.BytesIO(case.data)).convert("RGB"))
        got = J.to_rgb_device(jc, device)
        assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape, case.name
        assert np.array_equal(got.cpu().numpy(), ref), case.name
        decoded += 1
        out_of_range += not case.domain()["in_range"]
    print(f"decoded on the GPU: {decoded} of {len(CASES)} crafted files, {out_of_range} of them beyond [-512, 511]")
    assert decoded >= 150 and out_of_range >= 20


@pytest.mark.parametrize("level", [-513, -512, -129, -128, 127, 128, 511, 512, 1000])
def test_flat_block_saturates_at_the_limits(device, level):
    """DC-only block, quantiser 8: the sample before +128 is exactly ``level``."""
    b = [np.zeros((2, 3, 64), dtype=np.int64)]
    b[0][..., 0] = level
    data = JC.build(17, 9, "grey", b, [[8] * 64])
    got = J.to_rgb_device(J.parse(data), device).cpu().numpy()
    assert (got == min(max(level + 128, 0), 255)).all()
    assert np.array_equal(got, np.array(Image.open(io.BytesIO(data)).convert("RGB")))
