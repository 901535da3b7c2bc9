"""The chained layer head's request order (csrc/decode_chain.hip, the K = Ko = 3584 instance): x ahead of the weights, the
bias and residual pairs requested before the weights instead of after the sums, exact lane sweeps.  None of it may change a
bit: the chained head - that instance and a generic one - is compared with the four launches it replaces.
The single-row GEMV (csrc/decode.hip) still fetches bias / R after the sum: requesting them early measured no gain and cost
four registers (profiles/decode_tail_operands.json, item D), so it was not kept.  Its tests below pin what any such change
must keep: the tail additions are the IEEE f32 additions in the order sum, bias, R, nothing is read past element N - 1, and
the shape-specialised body agrees with the generic one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _randn(shape, device, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(device)


_HEADS = {}


def _head(device, Hq, Hkv, K, T):
    """weights, caches and rope tables of one head shape: made once, never written (the launches get clones of the caches)"""
    key = (Hq, Hkv, K, T)
    if key not in _HEADS:
        nq = (Hq + 2 * Hkv) * HD
        g = torch.Generator(device="cpu").manual_seed(Hq * 1000 + K + T)
        ang = torch.rand((T, HD // 2), generator=g) * 6.28
        emb = torch.cat((ang, ang), -1)
        _HEADS[key] = dict(
            wqkv=_randn((nq, K), device, 11, K ** -0.5), bq=_randn((nq,), device, 12, 0.1),
            nw=(1 + 0.1 * torch.randn((K,), generator=g)).to(torch.bfloat16).to(device),
            wo=_randn((K, Hq * HD), device, 13, (Hq * HD) ** -0.5),
            kc=_randn((Hkv, T, HD), device, 14), vc=_randn((Hkv, T, HD), device, 15),
            cos=emb.cos().to(device).contiguous(), sin=emb.sin().to(device).contiguous())
    return _HEADS[key]


# (Hq, Hkv, K, context, x as row 3 of a 5-row table): the exact-sweep instance on and off the 64-key split edge, a generic
# instance (K = 4096: two full chunks per thread in the norm), and the exact-sweep instance through the embedding-row form
@pytest.mark.parametrize("Hq,Hkv,K,ctx,indexed", [(28, 4, 3584, 63, False), (28, 4, 3584, 64, False), (28, 4, 3584, 130, False),
                                                  (32, 8, 4096, 65, False), (28, 4, 3584, 130, True)])
def test_chained_head_equals_four_launches(hip, device, Hq, Hkv, K, ctx, indexed):
    """y, the merged attention row, the packed qkv row and both caches of vis_decode_chain equal those of gemv + decode_attn +
    gemv bit for bit, with random non-zero bias, norm weight and x; two launches back to back on one workspace."""
    T = 256
    h = _head(device, Hq, Hkv, K, T)
    nq = (Hq + 2 * Hkv) * HD
    ns = -(-T // hip.DECODE_KEYS_PER_SPLIT)
    assert hip.decode_chain_supported(Hq, Hkv, HD, K)
    ws, sync = hip.decode_chain_state(device, Hq, Hkv, ns)
    po = torch.empty(Hq * ns * HD, dtype=torch.float32, device=device)
    pml = torch.empty(Hq * ns * 2, dtype=torch.float32, device=device)
    step = torch.tensor([ctx], dtype=torch.int32, device=device)
    for rep in range(2):
        x = _randn((K,), device, 400 + ctx + rep)
        k1, v1 = h["kc"].clone(), h["vc"].clone()
        qkv1 = torch.empty(nq, dtype=torch.bfloat16, device=device)
        att1 = torch.empty(Hq * HD, dtype=torch.bfloat16, device=device)
        y1 = torch.empty(K, dtype=torch.bfloat16, device=device)
        hip.gemv(x, h["wqkv"], qkv1, bias=h["bq"], norm_w=h["nw"], eps=1e-6)
        hip.decode_attn(qkv1, h["cos"], h["sin"], k1, v1, step, po, pml, att1, Hq, Hkv, HD, ns, HD ** -0.5)
        hip.gemv(att1, h["wo"], y1, residual=x)
        k2, v2 = h["kc"].clone(), h["vc"].clone()
        y2 = torch.full((K,), 3.0, dtype=torch.bfloat16, device=device)
        if indexed:
            table = torch.stack([_randn((K,), device, 70 + i) if i != 3 else x for i in range(5)])
            hip.decode_chain(table, h["wqkv"], h["bq"], h["nw"], h["wo"], y2, h["cos"], h["sin"], k2, v2, step, ws, sync, Hq, Hkv,
                             HD, ns, HD ** -0.5, 1e-6, x_index=torch.tensor([3], dtype=torch.int32, device=device))
        else:
            hip.decode_chain(x, h["wqkv"], h["bq"], h["nw"], h["wo"], y2, h["cos"], h["sin"], k2, v2, step, ws, sync, Hq, Hkv, HD, ns,
                             HD ** -0.5, 1e-6)
        torch.cuda.synchronize()
        qkv2, att2 = hip.decode_chain_rows(ws, Hq, Hkv)
        assert int(sync[hip.CHAIN_STATUS_WORD]) == 0, "a wait inside the chained launch timed out"
        assert int(sync[0]) == rep + 1
        assert torch.equal(qkv2, qkv1), f"launch {rep}: packed qkv row differs"
        assert torch.equal(k2, k1) and torch.equal(v2, v1), f"launch {rep}: KV append differs"
        assert torch.equal(att2, att1), f"launch {rep}: merged attention row differs"
        assert torch.equal(y2, y1), f"launch {rep}: y differs"


def _gemv_tail_case(hip, device, N, K):
    """y0 = W x in f32 without bias / residual, then the same launch with both, to f32 and to bf16.  bias and R are the LAST N
    elements of larger tensors (an odd element offset: 2-byte alignment only), so row N - 1's operands are the last elements
    there are and, for odd N, element N does not exist."""
    gen = torch.Generator(device=device).manual_seed(N * 31 + K)
    w = (torch.randn((N, K), generator=gen, device=device) * K ** -0.5).to(torch.bfloat16)
    x = _randn((K,), device, 5)
    bias = _randn((N + 9,), device, 6)[9:]
    res = _randn((N + 3,), device, 7, 2.0)[3:]
    assert bias.numel() == N and res.numel() == N
    y0 = torch.empty(N, dtype=torch.float32, device=device)
    y1 = torch.empty(N, dtype=torch.float32, device=device)
    yb = torch.empty(N, dtype=torch.bfloat16, device=device)
    hip.gemv(x, w, y0)
    hip.gemv(x, w, y1, bias=bias, residual=res)
    hip.gemv(x, w, yb, bias=bias, residual=res)
    torch.cuda.synchronize()
    return y0, y1, yb, bias, res


GEMV_SHAPES = [(3584, 18944), (7, 64), (6, 3584), (4608, 3584)]


@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_gemv_tail_operands_exact(hip, device, N, K):
    """sum, then bias, then residual: y1 == (y0 + bias) + R exactly (IEEE f32 additions), the bf16 output is its rounding -
    every row, the last one (N - 1, whose neighbour does not exist when N is odd) named on its own."""
    y0, y1, yb, bias, res = _gemv_tail_case(hip, device, N, K)
    want = (y0 + bias.float()) + res.float()
    assert bool((bias != 0).any()) and bool((res != 0).any())
    assert torch.equal(y1[N - 1:], want[N - 1:]), "row N - 1"
    assert torch.equal(y1, want)
    assert torch.equal(yb, want.to(torch.bfloat16))


@pytest.mark.parametrize("N,K", [s for s in GEMV_SHAPES if s[1] == 3584])
def test_gemv_generic_and_specialised_body_agree(hip, device, monkeypatch, N, K):
    """K = 3584 takes the shape-specialised body; VIS_GEMV_GENERIC=1 (read per launch) the generic one: same bits."""
    monkeypatch.delenv("VIS_GEMV_GENERIC", raising=False)
    spec = _gemv_tail_case(hip, device, N, K)
    monkeypatch.setenv("VIS_GEMV_GENERIC", "1")
    gen = _gemv_tail_case(hip, device, N, K)
    for a, b, what in zip(spec[:3], gen[:3], ("f32 sums", "f32 with bias and residual", "bf16 with bias and residual")):
        assert torch.equal(a, b), what
    want = (gen[0] + gen[3].float()) + gen[4].float()
    assert torch.equal(gen[1], want) and torch.equal(gen[2], want.to(torch.bfloat16))
