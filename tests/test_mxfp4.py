"""MXFP4 decode weights, host side (no GPU): hip.quantize_mxfp4_rows / hip.dequantize_mxfp4 against a table-driven E2M1
reference written here, and the engine's argument checks.

Format: OCP E2M1 codes (sign << 3 | exp << 1 | man: +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}; code 8 is -0), one E8M0 byte b per 32
consecutive K-elements of a row (X = 2^(b-127)), byte j of a row = element 2j (low nibble) and 2j+1 (high nibble).
Scale rule: X the smallest power of two with block_amax / X <= 6, i.e. amax = m 2^E, m in [1, 2): b = E + 125 when
m <= 1.5, else E + 126.  Elements round to nearest, ties to the even mantissa bit."""
import dataclasses
import math

import pytest
import torch

from vision_inspection_system_amd import hip

E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]        # magnitude of code & 7


def ref_code(v: float) -> int:
    """Nearest E2M1 code of a scaled value by brute force over the grid; a tie goes to the code with mantissa bit 0."""
    a = abs(v)
    best = min(range(8), key=lambda c: (abs(E2M1[c] - a), c & 1))
    return best | (8 if math.copysign(1.0, v) < 0 else 0)


def ref_scale_byte(amax: float) -> int:
    if amax == 0.0:
        return 127
    m, e = math.frexp(amax)          # amax = m 2^e, m in [0.5, 1)  ->  (2m) 2^(e-1)
    m, e = 2 * m, e - 1
    return min(max(e + (125 if m <= 1.5 else 126), 3), 250)


def planted():
    """[64, 256] f32: random rows, then blocks with planted maxima, exact ties, zeros and negative zeros."""
    g = torch.Generator().manual_seed(11)
    w = torch.randn((64, 256), generator=g) * torch.logspace(-3, 2, 64)[:, None]
    w[0, 0:32] = 0.0                                             # all-zero block
    w[0, 32:64] = 0.0
    w[0, 40] = -0.0                                              # all zero, one of them negative
    for i, e in enumerate((-9, 0, 5)):                           # amax exactly 6 2^e, 1.5 2^e, and just above both
        r = 1 + i
        base = torch.randn(32, generator=g).clamp(-1, 1)
        for j, top in enumerate((6.0, 1.5, float.fromhex("0x1.800002p+0"), float.fromhex("0x1.800002p+2"))):
            blk = base * 2.0 ** e
            blk[3 + j] = -top * 2.0 ** e if j & 1 else top * 2.0 ** e
            w[r, 32 * j:32 * j + 32] = blk
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    for i, e in enumerate((-4, 0, 7)):                           # exact ties x X, both signs, amax = 6 X pins X = 2^e
        blk = torch.zeros(32)
        blk[0] = 6.0
        blk[1:8] = torch.tensor(ties)
        blk[8:15] = -torch.tensor(ties)
        blk[15] = -0.0
        blk[16:24] = torch.tensor(E2M1)
        blk[24:32] = -torch.tensor(E2M1)
        w[4 + i, 64:96] = blk * 2.0 ** e
    return w


@pytest.fixture(scope="module")
def quantised():
    w = planted()
    wq, ws = hip.quantize_mxfp4_rows(w)
    return w, wq, ws


def test_shapes_and_scale_bytes_follow_the_rule(quantised):
    w, wq, ws = quantised
    assert wq.dtype == torch.uint8 and wq.shape == (64, 128) and ws.dtype == torch.uint8 and ws.shape == (64, 8)
    amax = w.reshape(64, 8, 32).abs().amax(-1)
    want = torch.tensor([[ref_scale_byte(float(a)) for a in row] for row in amax], dtype=torch.uint8)
    assert torch.equal(ws, want)
    # the planted maxima: 6 2^e and 1.5 2^e take X = 2^e / 2^(e-2); one ulp above 1.5 2^e (1.5 2^(e+2)) takes the next X
    for i, e in enumerate((-9, 0, 5)):
        assert ws[1 + i, :4].tolist() == [127 + e, 127 + e - 2, 127 + e - 1, 127 + e + 1]
    assert ws[0, 0] == 127 and ws[0, 1] == 127
    # X is the SMALLEST power of two that does not saturate: amax / X in (3, 6]
    X = torch.ldexp(torch.ones(64, 8), ws.int() - 127)
    nz = amax > 0
    assert ((amax / X)[nz] <= 6).all() and ((amax / X)[nz] > 3).all()


def test_codes_match_the_table_reference_and_nibble_order(quantised):
    w, wq, ws = quantised
    X = torch.ldexp(torch.ones(64, 8), ws.int() - 127).repeat_interleave(32, dim=1)
    scaled = (w.double() / X.double())
    want = torch.tensor([[ref_code(float(v)) for v in row] for row in scaled], dtype=torch.uint8)
    lo, hi = wq & 15, wq >> 4
    assert torch.equal(lo, want[:, 0::2]), "low nibble of byte j must be element 2j"
    assert torch.equal(hi, want[:, 1::2]), "high nibble of byte j must be element 2j+1"
    assert int((want & 7).max()) == 7 and (scaled.abs() <= 6).all()      # 6 is reached, nothing saturates
    # the planted ties: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4 (codes 0, 2, 2, 4, 4, 6, 6)
    for r in (4, 5, 6):
        codes = want[r, 64:96].tolist()
        assert codes[0] == 7 and codes[1:8] == [0, 2, 2, 4, 4, 6, 6] and codes[8:15] == [8, 10, 10, 12, 12, 14, 14]
        assert codes[15] == 8 and codes[16:24] == list(range(8)) and codes[24:32] == list(range(8, 16))
    assert want[0, 40] == 8 and want[0, :40].eq(0).all()                 # negative zero keeps its sign bit: code 8


def test_dequantize_inverts_the_packing_and_error_bound(quantised):
    w, wq, ws = quantised
    d = hip.dequantize_mxfp4(wq, ws)
    assert d.dtype == torch.float32 and d.shape == w.shape
    code = torch.stack((wq & 15, wq >> 4), dim=-1).reshape(64, 256)
    X = torch.ldexp(torch.ones(64, 8), ws.int() - 127).repeat_interleave(32, dim=1)
    table = torch.tensor(E2M1 + [-v for v in E2M1])
    assert torch.equal(d, table[code.long()] * X)
    assert d[0, 40] == 0 and d[0, :64].eq(0).all()                       # code 8 decodes to 0
    assert ((d - w).abs() <= X).all()                                    # widest grid gap is 2 X
    amax = w.reshape(64, 8, 32).abs().amax(-1).repeat_interleave(32, dim=1)
    assert ((d - w).abs()[amax > 0] < (amax / 3)[amax > 0]).all()
    assert (d.abs() <= 6 * X).all()
    # a wider scale row (lds > K/32) reads the same
    wide = torch.cat([ws, torch.full((64, 3), 77, dtype=torch.uint8)], dim=1)
    assert torch.equal(hip.dequantize_mxfp4(wq, wide), d)


def test_quantiser_takes_bf16_and_scale_clamp():
    g = torch.Generator().manual_seed(12)
    w = torch.randn((8, 64), generator=g)
    a = hip.quantize_mxfp4_rows(w.to(torch.bfloat16))
    b = hip.quantize_mxfp4_rows(w.to(torch.bfloat16).float())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    tiny = torch.full((1, 32), 2.0 ** -140)
    huge = torch.full((1, 32), 2.0 ** 127)
    assert hip.quantize_mxfp4_rows(tiny)[1].item() == 3 and hip.quantize_mxfp4_rows(huge)[1].item() == 250
    assert int((hip.quantize_mxfp4_rows(huge)[0] & 7).max()) == 7       # clamped scale: elements saturate at 6 X
    with pytest.raises(hip.HipLibraryError):
        hip.quantize_mxfp4_rows(torch.zeros(4, 48))


def test_engine_refuses_unknown_precision_and_unblocked_shapes():
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg = Qwen2VLConfig.tiny()
    with pytest.raises(ValueError):
        Qwen2VLEngine(cfg, None, "cpu", decode_weights="int3")
    Qwen2VLEngine.check_decode_weights(cfg, "mxfp4")                     # the tiny model fits
    Qwen2VLEngine.check_decode_weights(cfg, "fp8")
    odd = dataclasses.replace(cfg, intermediate=720)                     # 720 = 22.5 blocks
    with pytest.raises(ValueError, match="intermediate=720"):
        Qwen2VLEngine.check_decode_weights(odd, "mxfp4")
    with pytest.raises(ValueError, match="multiples of 32"):
        Qwen2VLEngine.check_decode_weights(dataclasses.replace(cfg, hidden=272, heads=2), "mxfp4")
    with pytest.raises(ValueError):    # through the constructor too (the kernel shape check may speak first)
        Qwen2VLEngine(odd, None, "cpu", decode_weights="mxfp4")
    Qwen2VLEngine.check_decode_weights(odd, "bf16")
