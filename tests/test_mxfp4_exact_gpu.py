"""The MXFP4 decode kernels (vis_gemv_mxfp4w / _rows, vis_gemm_decode_mxfp4) against float64 on operands for which f32 is exact
in any order (tests/mxfp4_exact.py).  Every output buffer starts as NaN or a sentinel and every comparison is bit for bit,
except the one bf16 ulp gemv_exact.swiglu_tolerance grants silu_fast in the SwiGLU test.

The edge each shape was chosen for (asserted from the restated walks in tests/test_mxfp4_exact.py):

vis_gemv_mxfp4w (a task = ROWS weight rows x one segment of SEG x 64 MX blocks; a wave owns the groups g_begin .. g_end):
  (40968, 32)        <8, 2> above 1024 blocks (1056); waves with 1 and with 2 groups (A -> B)
  (152064, 64)       the lm_head row count on 1490 blocks: 3 and 4 groups per wave, odd and even task counts, A -> B and B -> A
  (300032, 32)       the 2048-block cap: 4 and 5 groups per wave
  (75776, 64) SwiGLU <8, 2> SwiGLU (four outputs per task) with 2 groups per wave
  (8200, 10272)      <2, 5>, nseg = 2, four waves with 2 groups: the ring A B A B, the reset in the B half, B -> A
  (8200, 20512)      nseg = 3: 3 and 6 tasks, ONE live block in the last segment (63 idle lanes), A -> B
  (6, 4128) norm     516 chunks of x: the loop path of gv_stage_x_rmsnorm<true>.  (More than 512 chunks means K > 4096, which
                     the launcher gives to <2, 5>; <2, 2> with a norm is the next shape.)
  (1002, 704) norm   <2, 2>, the register path, K not a multiple of 128
vis_gemm_decode_mxfp4 (a workgroup owns `per` consecutive (tile, K-step) pairs and NSEG accumulator sets; a range that
touches more tiles stores the tile of its last set on the spot and reuses the set):
  (131200, 64)  B = 33, 64     5 whole tiles per range > NSEG = 4; 2 valid blocks in the only K-step
  (131200, 512) B = 64         per = 9 on 2 K-steps: ranges that start inside a tile; a cut tile that starts in the just-reset
                               set (slot 0, tile_done false) and is completed by the next workgroup (slot 1); 2 slots
  (131200, 768) B = 33         per = 13 on 3 K-steps: ranges start at every K-step of a tile
  (262272, 64)  B = 5, 17      9 tiles per range > NSEG = 8, MB = 1 and 2
  (262272, 512) B = 17         the cut case for NSEG = 8
  (65664, 384)  B = 5, 17, 33  4 valid blocks in the ragged last K-step at every MB, with cut tiles
  A tile flushed on the spot always ran to its last K-step (steps are left in the range), so that flush passes
  tile_done = true for every shape: asserted from the walk.
"""
import numpy as np
import pytest
import torch

import gemv_exact as G
import mxfp4_exact as M
from test_gemv_exact_gpu import _check_swiglu, _expect, _same, _sentinel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


_DEV = {}


def _dev(key, c, device):
    """The device copies of one case's weights (the latest case only)."""
    if _DEV.get("key") != key:
        _DEV.clear()
        _DEV.update(key=key, wq=c["wq"].to(device), ws=c["ws"].to(device))
    return _DEV["wq"], _DEV["ws"]


def _same_dev(got, want, what):
    """torch.equal on the device, with the first wrong element in the message."""
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).flatten() | torch.isnan(got).flatten()).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} wrong, first at flat index {i}: got "
                             f"{float(got.flatten()[i])!r} want {float(want.flatten()[i])!r} (last wrong {int(bad[-1])})")


GEMV_CASES = [(f, n, k) for n, k in M.GEMV_SHAPES for f in M.FAMILIES if f == "narrow" or k <= M.WIDE_MAX_K]


# ----------------------------------------------------------------------------- 1. GEMV: exact sums
@pytest.mark.parametrize("family,N,K", GEMV_CASES, ids=[f"{f}-{n}x{k}" for f, n, k in GEMV_CASES])
def test_gemv_exact_sums(hip, device, family, N, K):
    """Plain, bias + residual, f32 and bf16 output; up to N = 1002 again with padded ldq / lds (0xFF fill)."""
    c = M.case(family, N, K)
    wq, ws = _dev((family, N, K, 1), c, device)
    x, bias, r = c["x"][0].to(device), c["bias"].to(device), c["R"][0].to(device)
    wide = M.padded(wq, ws) if N <= M.PADDED_MAX_N else None
    for dtype in (torch.float32, torch.bfloat16):
        for full in (False, True):
            kw = dict(bias=bias, residual=r) if full else {}
            want = _expect((c["ref_br"] if full else c["ref"])[0], dtype)
            y = _sentinel((N,), dtype, device)
            hip.gemv_mxfp4(x, wq, ws, y, **kw)
            _same(y, want, f"gemv_mxfp4 {family} {N}x{K} {dtype} bias+residual={full}")
            if wide is not None:
                assert wide[0].stride(0) == K // 2 + 16 and wide[1].stride(0) == K // 32 + 3
                y2 = _sentinel((N,), dtype, device)
                hip.gemv_mxfp4(x, wide[0], wide[1], y2, **kw)
                _same(y2, want, f"gemv_mxfp4 {family} {N}x{K} padded {dtype} bias+residual={full}")


# ----------------------------------------------------------------------------- 2. GEMV: SwiGLU pairing
@pytest.mark.parametrize("N,K", M.GEMV_SWIGLU_SHAPES, ids=[f"{n}x{k}" for n, k in M.GEMV_SWIGLU_SHAPES])
def test_gemv_swiglu_pairing(hip, device, N, K):
    """(64, 256): <2, 2>, one output per task; (16448, 64): <8, 2>, four outputs per task; (75776, 64): two such groups per
    wave.  Tolerance and purpose: test_gemv_exact_gpu._check_swiglu."""
    c = M.swiglu_case(N, K)
    y = _sentinel((N // 2,), torch.bfloat16, device)
    hip.gemv_mxfp4(c["x"].to(device), c["wq"].to(device), c["ws"].to(device), y, act=hip.ACT_SWIGLU)
    _check_swiglu(c, y, f"gemv_mxfp4 swiglu {N}x{K}")


# ----------------------------------------------------------------------------- 3. GEMV: the fused RMSNorm, exactly
@pytest.mark.parametrize("N,K", M.GEMV_NORM_SHAPES, ids=[f"{n}x{k}" for n, k in M.GEMV_NORM_SHAPES])
def test_gemv_fused_rmsnorm_exact(hip, device, N, K):
    """gv_stage_x_rmsnorm<true> (the swizzled staging) on gemv_exact.norm_operands: the staged row is sign * norm_w."""
    c = M.norm_case(N, K)
    wq, ws = c["wq"].to(device), c["ws"].to(device)
    x, nw, bias = c["x"][0].to(device), c["norm_w"].to(device), c["bias"].to(device)
    for dtype in (torch.float32, torch.bfloat16):
        for with_bias in (False, True):
            y = _sentinel((N,), dtype, device)
            hip.gemv_mxfp4(x, wq, ws, y, bias=bias if with_bias else None, norm_w=nw, eps=G.NORM_EPS)
            _same(y, _expect((c["ref_b"] if with_bias else c["ref"])[0], dtype), f"gemv_mxfp4 norm {N}x{K} {dtype} bias={with_bias}")


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("N,K", M.GEMV_ROWS_NORM_SHAPES, ids=[f"{n}x{k}" for n, k in M.GEMV_ROWS_NORM_SHAPES])
def test_gemv_rows_fused_rmsnorm_exact(hip, device, N, K, B):
    """vis_gemv_mxfp4w_rows: every row has its own sign pattern and its own |x|, staged one after the other through the
    same reduction scratch (the __syncthreads between rows).  (40968, 32): waves with two groups in the rows form.
    x has ldx = K + 8 (NaN in the padding); the output sits in a wider sentinel buffer with a row below."""
    c = M.norm_case(N, K, B)
    wq, ws = c["wq"].to(device), c["ws"].to(device)
    nw, bias = c["norm_w"].to(device), c["bias"].to(device)
    xb = torch.full((B, K + 8), G.NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    xb[:, :K] = c["x"]
    x = xb.to(device)[:, :K]
    for dtype in (torch.float32, torch.bfloat16):
        ob = _sentinel((B + 1, N + 16), dtype, device)
        hip.gemv_mxfp4_rows(x, wq, ws, ob[:B, :N], bias=bias, norm_w=nw, eps=G.NORM_EPS)
        _same(ob[:B, :N], _expect(c["ref_b"], dtype), f"gemv_mxfp4_rows norm B={B} {N}x{K} {dtype}")
        outside = torch.ones(ob.shape, dtype=torch.bool)
        outside[:B, :N] = False
        assert bool((ob.cpu()[outside] == G.SENTINEL).all()), "a sentinel outside [B, N] was overwritten"


# ----------------------------------------------------------------------------- 4. MFMA projection: partial slots
def _slot_counts(w, N):
    """Per column: the number of slots its tile is cut into."""
    cnt = np.zeros(w["tiles"], dtype=np.int64)
    for r in w["ranges"]:
        for e in r:
            cnt[e[0]] = max(cnt[e[0]], e[6] + 1)
    return torch.from_numpy(np.repeat(cnt, 128)[:N])


def _check_part(hip, device, family, N, K, B):
    c = M.case(family, N, K, 64)
    wq, ws = _dev((family, N, K, 64), c, device)
    x = c["x"][:B].to(device)
    ref = c["ref"][:B].to(device)
    w = M.walk_gemm(N, K, B)
    need = hip.decode_gemm_mxfp4_ksplit(N, K)
    assert need == w["nslots"]
    cnt = _slot_counts(w, N).to(device)
    R = hip.part_rows(B)
    for ks in (need, need + 1):
        part = torch.full((ks * R * N,), float("nan"), dtype=torch.float32, device=device)
        assert hip.decode_gemm_mxfp4(x, wq, ws, part=part, ksplit=ks) == ks
        slabs = part.view(ks, R, N)[:, :B]
        assert bool(torch.isfinite(slabs).all()), f"ksplit={ks}: a slot was left unwritten"
        _same_dev(slabs.double().sum(0), ref, f"decode_gemm_mxfp4 {family} {N}x{K} B={B} ksplit={ks}")
        for z in range(ks):
            cols = cnt <= z
            assert bool((slabs[z][:, cols] == 0).all()), f"ksplit={ks}: slot {z} is not zero where the tile has fewer slots"
        del part, slabs


GEMM_CASES = [(n, k, b) for n, k, bs in M.GEMM_SHAPES for b in bs]
GEMM_WIDE_CASES = [(n, k, b) for n, k, bs in M.GEMM_WIDE_SHAPES for b in bs]


@pytest.mark.parametrize("N,K,B", GEMM_CASES, ids=[f"{n}x{k}-B{b}" for n, k, b in GEMM_CASES])
def test_gemm_part_exact(hip, device, N, K, B):
    """ksplit = the geometry's count and one more: the slots summed in float64 equal the reference, every slot is finite,
    and every slot from the tile's own count upward is zero."""
    _check_part(hip, device, "narrow", N, K, B)


@pytest.mark.parametrize("N,K,B", GEMM_WIDE_CASES, ids=[f"{n}x{k}-B{b}" for n, k, b in GEMM_WIDE_CASES])
def test_gemm_part_exact_wide_scales(hip, device, N, K, B):
    """Scale bytes 3 .. 250 with x scaled against them: a scale byte of the neighbouring row or block is a factor of two."""
    _check_part(hip, device, "wide", N, K, B)


# ----------------------------------------------------------------------------- 5. MFMA projection: direct output
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_direct_exact(hip, device, dtype):
    """part=None on (131200, 64) at B = 40: 5 whole tiles per workgroup on 4 accumulator sets; the columns past N of a wider
    ldc keep the sentinel."""
    N, K, B = M.GEMM_DIRECT
    c = M.case("narrow", N, K, 64)
    wq, ws = _dev(("narrow", N, K, 64), c, device)
    wide = torch.full((B, N + 8), -777.0, dtype=dtype, device=device)
    hip.decode_gemm_mxfp4(c["x"][:B].to(device), wq, ws, out=wide[:, :N])
    _same_dev(wide[:, :N], _expect(c["ref"][:B], dtype).to(device), f"decode_gemm_mxfp4 direct {dtype}")
    assert bool((wide[:, N:] == -777.0).all()), "columns past N were written"


# ----------------------------------------------------------------------------- 6. every code with every scale byte
def test_every_code_and_scale_byte(hip, device):
    """mxfp4_exact.every_code_case on both kernels: output 16 j + c is the E2M1 value of code c (times 1, 2 or 4 by input
    row), read through scale byte 3 + j and x = 2^(127 - byte).  Bytes outside 3 .. 250 are not quantiser output and are
    left out.  Value equality: the -0 code sums to +0."""
    c = M.every_code_case()
    wq, ws, x = c["wq"].to(device), c["ws"].to(device), c["x"].to(device)
    N, K, B = M.EVERY_N, M.EVERY_K, M.EVERY_B
    for dtype in (torch.float32, torch.bfloat16):
        y = _sentinel((N,), dtype, device)
        hip.gemv_mxfp4(x[0], wq, ws, y)
        _same(y, _expect(c["want"][0], dtype), f"gemv_mxfp4 every code {dtype}")
    ob = _sentinel((4, N), torch.float32, device)
    hip.gemv_mxfp4_rows(x[:4], wq, ws, ob)
    _same(ob, c["want"][:4].float(), "gemv_mxfp4_rows every code")
    need = hip.decode_gemm_mxfp4_ksplit(N, K)
    R = hip.part_rows(B)
    part = torch.full((need * R * N,), float("nan"), dtype=torch.float32, device=device)
    assert hip.decode_gemm_mxfp4(x, wq, ws, part=part) == need
    slabs = part.view(need, R, N)[:, :B]
    assert bool(torch.isfinite(slabs).all())
    _same(slabs.double().sum(0), c["want"], "decode_gemm_mxfp4 every code")
    out = torch.full((B, N), -777.0, dtype=torch.float32, device=device)
    hip.decode_gemm_mxfp4(x, wq, ws, out=out)
    _same(out, c["want"].float(), "decode_gemm_mxfp4 direct every code")
