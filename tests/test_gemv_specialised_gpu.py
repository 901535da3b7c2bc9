"""The shape-specialised single-row bf16 GEMV instances (csrc/decode.hip, gemv_bf16_shape_body) against the generic body.

The specialised body multiplies the same bytes in the same order as the generic one, so every output must be equal BIT FOR
BIT: the generic body is reached in the same process with VIS_GEMV_GENERIC=1 (read per launch).  K = 3584 is specialised;
K = 18944 is asked for by the same cases and stays on the generic body (its specialised form exceeded the register budget,
DESIGN.md section 4), so for it the comparison is generic against generic.  N is small and awkward: one pair, one
workgroup, just past the 1024-workgroup knee of the grid rule (several pairs per wave), an odd row count.

The partition test is host arithmetic only and carries no gpu mark.  Shapes that must keep the generic path (K not a
multiple of 512, K = 4096, two input rows) are checked against a float64 reference with the tolerance of
tests/test_kernels_gpu.py::test_gemv_plain (atol 3e-2, rtol 1e-2 at weights of scale 1 / sqrt(K)).
"""
import math
import os

import numpy as np
import pytest
import torch

KS = [3584, 18944]
PLAIN_NS = [2, 8, 4100, 4101]
SWIGLU_NS = [64, 2080]


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _randn(shape, device, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(device)


_CACHE = {}


def _operands(device, N, K):
    """seeded N(0, 1) bf16 x, W, bias, residual, norm weight for (N, K): made once, shared, never written"""
    key = (N, K)
    if key not in _CACHE:
        _CACHE[key] = (_randn((K,), device, 1000 + N), _randn((N, K), device, 2000 + N + K), _randn((N,), device, 3000 + N),
                       _randn((N,), device, 4000 + N), _randn((K,), device, 5000 + K))
    return _CACHE[key]


class _generic:
    def __enter__(self):
        os.environ["VIS_GEMV_GENERIC"] = "1"

    def __exit__(self, *a):
        del os.environ["VIS_GEMV_GENERIC"]


def _both(run):
    """run() under the default dispatch and under VIS_GEMV_GENERIC=1; returns the two results as CPU byte tensors"""
    assert "VIS_GEMV_GENERIC" not in os.environ
    new = run()
    with _generic():
        old = run()
    torch.cuda.synchronize()
    as_bytes = lambda t: t.contiguous().cpu().view(torch.uint8)
    if isinstance(new, tuple):
        return [as_bytes(t) for t in new], [as_bytes(t) for t in old]
    return [as_bytes(new)], [as_bytes(old)]


def _assert_same(new, old, what):
    for i, (a, b) in enumerate(zip(new, old)):
        assert torch.equal(a, b), f"{what}: output {i} differs in {int((a != b).sum())} of {a.numel()} bytes"


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", PLAIN_NS)
@pytest.mark.parametrize("kind", ["plain", "bias", "residual", "rmsnorm", "f32"])
def test_specialised_equals_generic(hip, device, kind, N, K):
    x, w, b, r, nw = _operands(device, N, K)

    def run():
        out = torch.full((N,), float("nan"), dtype=torch.float32 if kind == "f32" else torch.bfloat16, device=device)
        hip.gemv(x, w, out, bias=b if kind == "bias" else None, residual=r if kind == "residual" else None,
                 norm_w=nw if kind == "rmsnorm" else None)
        return out
    new, old = _both(run)
    assert not torch.isnan(new[0].view(torch.float32 if kind == "f32" else torch.bfloat16).float()).any()
    _assert_same(new, old, f"gemv {kind} N={N} K={K}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", SWIGLU_NS)
@pytest.mark.parametrize("norm", [False, True])
def test_specialised_swiglu_equals_generic(hip, device, norm, N, K):
    x, w, _, _, nw = _operands(device, N, K)

    def run():
        out = torch.full((N // 2,), float("nan"), dtype=torch.bfloat16, device=device)
        hip.gemv(x, w, out, norm_w=nw if norm else None, act=hip.ACT_SWIGLU)
        return out
    new, old = _both(run)
    _assert_same(new, old, f"gemv swiglu N={N} K={K} norm={norm}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", PLAIN_NS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_specialised_argmax_equals_generic(hip, device, temperature, masked, N, K):
    x, w, _, _, nw = _operands(device, N, K)
    allow = None
    if masked:
        bits = np.random.default_rng(N + K).integers(0, 2 ** 63, (N + 63) // 64, dtype=np.int64)
        bits[0] |= 2                                    # at least one allowed id
        allow = torch.from_numpy(bits).to(device)

    def run():
        logits = torch.full((N,), float("nan"), dtype=torch.float32, device=device)
        ws_val = torch.full((2048,), float("nan"), dtype=torch.float32, device=device)
        ws_idx = torch.full((2048,), -1, dtype=torch.int32, device=device)
        tokens = torch.zeros((4,), dtype=torch.int32, device=device)
        cur = torch.zeros((1,), dtype=torch.int32, device=device)
        step = torch.ones((1,), dtype=torch.int32, device=device)
        if masked:
            hip.gemv_argmax_masked(x, w, logits, ws_val, ws_idx, tokens, cur, step, allow, norm_w=nw, temperature=temperature, seed=11)
        else:
            hip.gemv_argmax(x, w, logits, ws_val, ws_idx, tokens, cur, step, norm_w=nw, temperature=temperature, seed=11)
        blocks = hip.gemv_grid(N)[1]
        return logits, ws_val[:blocks], ws_idx[:blocks], tokens, cur, step
    new, old = _both(run)
    _assert_same(new, old, f"gemv argmax N={N} K={K} masked={masked} T={temperature}")


@pytest.mark.parametrize("N,swiglu", [(n, False) for n in PLAIN_NS] + [(n, True) for n in SWIGLU_NS]
                         + [(37888, True), (3584, False), (152064, False)])
def test_partition_equals_division(hip, N, swiglu):
    """every wave's [p_begin, p_end) by the division the generic body makes and by the multiply-shift of the specialised one
    (constants from the library), for the grids of the cases above and of the 7B decode step"""
    n_pairs, blocks = hip.gemv_grid(N, hip.ACT_SWIGLU if swiglu else hip.ACT_NONE)
    n_waves = 4 * blocks
    q, r, m, s = hip.gemv_partition(n_pairs, n_waves)
    assert q * n_waves + r == n_pairs and 0 <= r < n_waves and m < 2 ** 32
    for wid in range(n_waves + 1):
        assert r * wid < 2 ** 31
        assert q * wid + ((r * wid * m) >> s) == n_pairs * wid // n_waves, (N, wid)
    assert n_pairs * n_waves // n_waves == n_pairs          # the last wave ends at the last pair


def _ref64(w, x, b=None):
    y = w.double().cpu().numpy() @ x.double().cpu().numpy()
    return torch.from_numpy(y if b is None else y + b.double().cpu().numpy())


def _assert_close(got, ref, atol, rtol, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    print(f"{what}: max err {err.max().item():.5f}, bound at that element {(atol + rtol * ref.abs())[err.argmax()].item():.5f}")
    assert not (err > atol + rtol * ref.abs()).any(), f"{what}: max err {err.max().item():.6f}"


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,nb", [(520, 3576, 1), (520, 4096, 1), (520, 3584, 2)])
def test_generic_fallback_shapes(hip, device, N, K, nb):
    w = _randn((N, K), device, 71, 1.0 / math.sqrt(K))
    b = _randn((N,), device, 72)
    x = _randn((nb, K), device, 73)
    out = torch.empty((nb, N), dtype=torch.bfloat16, device=device)
    if nb == 1:
        hip.gemv(x[0], w, out[0], bias=b)
    else:
        hip.gemv_rows(x, w, out, bias=b)
    for i in range(nb):
        _assert_close(out[i], _ref64(w, x[i], b), atol=3e-2, rtol=1e-2, what=f"generic gemv N={N} K={K} row {i} of {nb}")
