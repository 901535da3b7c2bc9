"""fp8 (e4m3) cross-attention keys / values at kernel level (csrc/cross_attn.hip): the row quantiser bit for bit against the
numpy restatement, vis_decode_cross_attn_fp8 against float64 on the SAME codes and scales inside the derived slack of
tests/cross_kv_ref.py (no element excluded), an exact mean, poisoned rows past the key count, the batch form against the
single launch, and the refusals."""
import numpy as np
import pytest
import torch

import cross_kv_ref as X
from test_auditor_quant import BOUND_NKEYS, BOUND_SHAPES, TK, edge_rows

EPS = 1e-5


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip
    hip.load()
    return hip


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t.to(dtype) if dtype is not None else t


def _run(hip, device, q, w, kq, ksc, vq, vsc, nkeys, scale=X.SCALE):
    """One single-sequence launch; q, w float arrays of bf16 values.  Returns the bf16 output as float64 [Hq, 128]."""
    Hq, Hkv, T = q.shape[0], kq.shape[0], kq.shape[1]
    ns = -(-T // hip.DECODE_KEYS_PER_SPLIT)
    out = torch.full((Hq * 128,), float("nan"), dtype=torch.bfloat16, device=device)
    part_o = torch.full((Hq * ns * 128,), float("nan"), dtype=torch.float32, device=device)
    part_ml = torch.full((Hq * ns * 2,), float("nan"), dtype=torch.float32, device=device)
    hip.decode_cross_attn_fp8(_dev(q, device, torch.bfloat16).reshape(-1), _dev(w, device, torch.bfloat16), _dev(kq, device),
                              _dev(ksc, device), _dev(vq, device), _dev(vsc, device),
                              torch.tensor([nkeys - 1], dtype=torch.int32, device=device), part_o, part_ml, out, Hq, Hkv, 128,
                              ns, scale, EPS)
    return out.view(Hq, 128).to(torch.float64).cpu().numpy()


@pytest.mark.gpu
def test_row_quantiser_bit_for_bit(hip, device):
    """Codes and scales of the K / V row quantiser against the numpy restatement: an all-zero row, amax exactly 448 * 2^k,
    values that round up to the next binade, +-max, a denormal-range row, rows on the scale floor, and Gaussian rows."""
    rows = edge_rows()
    rng = np.random.default_rng(1)
    more = torch.from_numpy((rng.standard_normal((500, 128)) * rng.uniform(1e-3, 50, (500, 1))).astype(np.float32)) \
        .to(torch.bfloat16).float().numpy()
    x = np.concatenate([rows, more]).reshape(2, -1, 128)[:, :, :]            # [2, rows / 2, 128]: a leading dim like [Hkv, T, 128]
    xd = _dev(x, device, torch.bfloat16)
    codes = torch.full(x.shape, 0xAA, dtype=torch.uint8, device=device)
    scales = torch.full(x.shape[:-1], -1.0, dtype=torch.float32, device=device)
    hip.quantize_cross_kv(xd, codes, scales)
    want_c, want_s = X.quantize_rows(x)
    got_c, got_s = codes.cpu().numpy(), scales.cpu().numpy()
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
    mag = (want_c & 0x7F) != 0                                               # the sign of a zero code is not pinned
    assert np.array_equal(got_c & 0x7F, want_c & 0x7F) and np.array_equal(got_c[mag], want_c[mag])


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv", BOUND_SHAPES)
def test_attention_inside_the_derived_slack(hip, device, Hq, Hkv):
    """vis_decode_cross_attn_fp8 against float64 on the same codes and scales; Tk = 256 spans four splits, nkeys 1, 63, 64, 65
    and one below / at / one above the second split boundary, and Tk.  Bound (tests/cross_kv_ref.py): every f32 operation of
    the scheme counted - rel = (7 Smax + NS + 48) 2^-24 of a_d = sum p t |v| / sum p, Smax the largest |score|, NS the splits
    that ran; the kernel may write any bf16 in [rne(o - rel a), rne(o + rel a)] and NO element is excluded.  The float32
    emulation of the fault-free kernel stays inside it on these inputs (tests/test_auditor_quant.py)."""
    q, w, kq, ksc, vq, vsc = X.bound_inputs(Hq, Hkv, TK, 0)
    qn = X.q_norm(q, w, EPS)
    for nkeys in BOUND_NKEYS:
        o, a, smax = X.attention(qn, kq, ksc, vq, vsc, nkeys)
        lo, hi = X.interval(o, a, smax, nkeys)
        got = _run(hip, device, q, w, kq, ksc, vq, vsc, nkeys)
        bad = ~((got >= lo) & (got <= hi))
        print(f"Hq {Hq} nkeys {nkeys}: max |got - o| / a = {float((np.abs(got - o) / np.maximum(a, 1e-30)).max()):.3e}, "
              f"rel {X.rel_slack(smax, -(-nkeys // 64)):.3e}, outside {int(bad.sum())}")
        assert not bad.any(), (nkeys, int(bad.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv", BOUND_SHAPES)
def test_attention_with_arbitrary_k_codes(hip, device, Hq, Hkv):
    """The same comparison with ANY finite K code (fractional, denormal, up to +-448) through the fp8 -> bf16 conversion: the
    dot product is then inexact, so the slack gains the 128-term accumulation error, 360 Sabs 2^-24 (tests/cross_kv_ref.py:
    two units for each of the 127 additions of the MFMA, whose order is not published), Sabs = the largest
    kscale 2^-3 sum |q k| of a valid key.  No element is excluded."""
    q, w, kq, ksc, vq, vsc = X.general_inputs(Hq, Hkv, TK, 0)
    qn = X.q_norm(q, w, EPS)
    for nkeys in BOUND_NKEYS:
        o, a, smax = X.attention(qn, kq, ksc, vq, vsc, nkeys)
        sabs = X.dot_abs(qn, kq, ksc, nkeys)
        lo, hi = X.interval(o, a, smax, nkeys, sabs)
        got = _run(hip, device, q, w, kq, ksc, vq, vsc, nkeys)
        bad = ~((got >= lo) & (got <= hi))
        print(f"general K, Hq {Hq} nkeys {nkeys}: Smax {smax:.1f} Sabs {sabs:.1f} outside {int(bad.sum())}")
        assert not bad.any(), (nkeys, int(bad.sum()))


@pytest.mark.gpu
def test_exact_mean(hip, device):
    """Power-of-two scales, integer codes and a q that scores every key alike: p = 1 for every key, the output is the mean of
    vscale * vcode - exactly representable, so torch.equal.  (i) every key contributes the same c_d over 150 keys (three
    splits, the last ragged); (ii) contributions in {-2, 0, 2} over 128 keys: the mean is a multiple of 2^-6 below 2."""
    Hq, Hkv, T = 2, 1, 192
    rng = np.random.default_rng(5)
    code_of = {float(X.E4M3[c]): c for c in X.INT_CODES}
    enc = np.vectorize(lambda v: code_of[float(v)], otypes=[np.uint8])
    q = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(Hq, 128))
    w = np.concatenate([rng.integers(1, 4, 64), np.zeros(64)]).astype(np.float32)      # dims 64.. do not score
    e = rng.integers(-1, 2, size=(Hkv, T))                                             # scales 2^e
    ksc, vsc = np.exp2(e).astype(np.float32), np.exp2(rng.integers(-1, 2, size=(Hkv, T))).astype(np.float32)
    base = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(Hkv, 1, 64))
    kval = np.concatenate([base * 2.0 / ksc[..., None], rng.integers(-8, 9, size=(Hkv, T, 64))], axis=-1)
    kq = enc(kval)
    for nkeys, contrib in ((150, np.broadcast_to(rng.choice(np.array([-8.0, -4.0, -2.0, 2.0, 4.0, 6.0]), size=(Hkv, 1, 128)),
                                                 (Hkv, T, 128))),
                           (128, rng.choice(np.array([-2.0, 0.0, 2.0]), size=(Hkv, T, 128)))):
        vq = enc(contrib / vsc[..., None])
        want = (contrib[:, :nkeys].sum(axis=1) / nkeys).repeat(Hq // Hkv, axis=0)
        assert np.array_equal(X.bf16r(want), want)
        got = _run(hip, device, q, w, kq, ksc, vq, vsc, nkeys)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), nkeys


def _random_case(Hq, Hkv, T, seed):
    rng = np.random.default_rng(seed)
    q = torch.from_numpy(rng.standard_normal((Hq, 128)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    w = torch.from_numpy((1 + 0.1 * rng.standard_normal(128)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    kq, vq = rng.choice(X.FINITE_CODES, size=(Hkv, T, 128)), rng.choice(X.FINITE_CODES, size=(Hkv, T, 128))
    ksc = (rng.uniform(0.5, 1.5, (Hkv, T)) * 2.0 ** -9).astype(np.float32)
    vsc = (rng.uniform(0.5, 1.5, (Hkv, T)) * 2.0 ** -7).astype(np.float32)
    return q, w, kq, ksc, vq, vsc


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv", BOUND_SHAPES)
def test_rows_past_the_key_count_are_never_used(hip, device, Hq, Hkv):
    """Rows at or past nkeys filled with NaN codes (0x7F) and inf scales: the output does not change by a bit."""
    q, w, kq, ksc, vq, vsc = _random_case(Hq, Hkv, TK, 11)
    for nkeys in (1, 63, 64, 65, 129, 255):
        clean = _run(hip, device, q, w, kq, ksc, vq, vsc, nkeys, scale=128 ** -0.5)
        assert np.isfinite(clean).all() and np.abs(clean).max() > 0
        kq2, vq2, ksc2, vsc2 = kq.copy(), vq.copy(), ksc.copy(), vsc.copy()
        kq2[:, nkeys:], vq2[:, nkeys:] = 0x7F, 0x7F
        ksc2[:, nkeys:], vsc2[:, nkeys:] = np.inf, np.inf
        dirty = _run(hip, device, q, w, kq2, ksc2, vq2, vsc2, nkeys, scale=128 ** -0.5)
        assert np.array_equal(clean, dirty), nkeys


@pytest.mark.gpu
def test_batch_form_equals_the_single_launch(hip, device):
    """B = 3 slots with three key counts, strided batch views: slot b equals the single launch on slot b's data bit for bit."""
    Hq, Hkv, T, B = 32, 8, TK, 3
    ns = T // 64
    cases = [_random_case(Hq, Hkv, T, 20 + b) for b in range(B)]
    nkeys = [65, 256, 1]
    qb = torch.zeros((B, (Hq + 2 * Hkv) * 128), dtype=torch.bfloat16, device=device)     # q = the leading columns of a packed row
    for b in range(B):
        qb[b, :Hq * 128] = _dev(cases[b][0], device, torch.bfloat16).reshape(-1)
    stack = lambda i, extra: torch.stack([_dev(np.stack([c[i]] * extra), device) for c in cases])   # [B, layers, ...]
    kq, ksc, vq, vsc = stack(2, 2), stack(3, 2), stack(4, 2), stack(5, 2)
    out = torch.zeros((B, Hq * 128), dtype=torch.bfloat16, device=device)
    part_o = torch.empty(B * Hq * ns * 128, dtype=torch.float32, device=device)
    part_ml = torch.empty(B * Hq * ns * 2, dtype=torch.float32, device=device)
    w = cases[0][1]
    hip.decode_cross_attn_fp8_batch(qb[:, :Hq * 128], _dev(w, device, torch.bfloat16), kq[:, 1], ksc[:, 1], vq[:, 1], vsc[:, 1],
                                    torch.tensor([n - 1 for n in nkeys], dtype=torch.int32, device=device), part_o, part_ml,
                                    out, Hq, Hkv, 128, ns, 128 ** -0.5, EPS)
    for b in range(B):
        c = cases[b]
        one = _run(hip, device, c[0], w, c[2], c[3], c[4], c[5], nkeys[b], scale=128 ** -0.5)
        assert np.array_equal(out[b].view(Hq, 128).to(torch.float64).cpu().numpy(), one), b


def test_refusals_launch_nothing():
    """Null pointers, HD != 128, misaligned pointers, nsplit not covering Tk, a Tk that is no multiple of 64, batch > 64 and bad
    strides: VIS_ERR_ARG before any HIP call (the pointers are never dereferenced, so this needs no GPU)."""
    from vision_inspection_system_amd import hip
    lib = hip.load()
    P = 4096                                                                  # an aligned fake address

    def single(q=P, nw=P, kq=P, ks=P, vq=P, vs=P, nk=P, po=P, pm=P, out=P, Hq=32, Hkv=8, HD=128, T=256, ns=4):
        return lib.vis_decode_cross_attn_fp8(q, nw, kq, ks, vq, vs, nk, po, pm, out, Hq, Hkv, HD, T, ns, 0.088, 1e-5, None)

    def batch(B=3, q_bs=4096, kv_bs=8 * 256 * 128, sc_bs=8 * 256, **kw):
        a = dict(q=P, nw=P, kq=P, ks=P, vq=P, vs=P, nk=P, po=P, pm=P, out=P)
        a.update(kw)
        return lib.vis_decode_cross_attn_fp8_batch(a["q"], a["nw"], a["kq"], a["ks"], a["vq"], a["vs"], a["nk"], a["po"], a["pm"],
                                                   a["out"], 32, 8, 128, 256, 4, 0.088, 1e-5, B, q_bs, kv_bs, sc_bs, None)

    for name in ("q", "nw", "kq", "ks", "vq", "vs", "nk", "po", "pm", "out"):
        assert single(**{name: None}) == 1, name
        assert batch(**{name: None}) == 1, name
    assert single(HD=64) == 1 and single(HD=256) == 1
    assert single(Hq=30) == 1 and single(Hq=24, Hkv=8) == 1                   # Hq % Hkv, a group size without an instantiation
    for name, off in (("kq", 8), ("vq", 4), ("ks", 4), ("vs", 8), ("nk", 2), ("po", 2), ("pm", 1), ("q", 1), ("out", 1), ("nw", 1)):
        assert single(**{name: P + off}) == 1, name
    assert single(ns=3) == 1 and single(ns=0) == 1 and single(ns=257) == 1     # nsplit must cover Tk
    assert single(T=250) == 1 and single(T=0) == 1                             # whole splits only
    assert batch(B=65) == 1 and batch(B=0) == 1
    assert batch(q_bs=0) == 1 and batch(kv_bs=0) == 1 and batch(sc_bs=0) == 1
    assert batch(q_bs=4100) == 1 and batch(kv_bs=8 * 256 * 128 + 8) == 1 and batch(sc_bs=8 * 256 + 2) == 1
