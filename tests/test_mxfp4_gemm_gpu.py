"""vis_gemm_decode_mxfp4 on the GPU: the MFMA batched-decode projection on MXFP4 weights against hip.dequantize_mxfp4 -
bit for bit where the arithmetic is exact (one-hot rows; integer x with power-of-two scales, where every f32 summation
order gives the same sum), bit-invariant to batch size and row position on random data, within the bf16 projection's
tolerance of vis_gemm_decode_bf16 on the de-quantised weights - and the Qwen2-VL engine with ``mxfp4_gemm_from=5``."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden, oracle_inputs, ref_config
from test_mxfp4_gpu import LOGIT_TOL, _assert_close, _check_tokens, _dequantised_sd, _random_codes, _randn, _requests

pytestmark = pytest.mark.gpu
SLOTS = 16                                 # slots a partial workspace holds


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _part(hip, B, N, device, fill=float("nan")):
    return torch.full((SLOTS * hip.part_rows(B) * N,), fill, dtype=torch.float32, device=device)


def _finalized(hip, x, wq, ws, **kw):
    B, N = x.shape[0], wq.shape[0]
    part = _part(hip, B, N, x.device)
    ks = hip.decode_gemm_mxfp4(x, wq, ws, part=part)
    assert ks == hip.decode_gemm_mxfp4_ksplit(N, wq.shape[1] * 2)
    swiglu = kw.get("swiglu", False)
    y = torch.empty((B, N // 2 if swiglu else N), dtype=torch.bfloat16, device=x.device)
    hip.skinny_finalize(part, ks, y, N, **kw)
    return y


# ----------------------------------------------------------------------------- 1. element order
def test_element_order_one_hot(hip, device):
    """Rows of A are one-hot e_k: the finalised output is column k of the de-quantised matrix (every value an exact bf16),
    which catches nibble, byte-select, scale-index and MFMA lane-map mistakes bit for bit."""
    N, K, B = 128, 128, 5
    wq, ws = _random_codes(N, K, device, 700)
    deq = hip.dequantize_mxfp4(wq, ws)
    assert len(torch.unique(wq & 15)) == 16 and len(torch.unique(ws)) > 1
    eye = torch.eye(K, dtype=torch.bfloat16, device=device)
    got = torch.empty((K, N), dtype=torch.float32, device=device)
    for k0 in list(range(0, K - B, B)) + [K - B]:
        got[k0:k0 + B] = _finalized(hip, eye[k0:k0 + B], wq, ws).float()
    assert torch.equal(got.t(), deq), "y(e_k) must be column k of dequantize_mxfp4"


# ----------------------------------------------------------------------------- 2. exact sums
_EXACT = {}


def _exact_case(hip, device, N, K):
    """Codes, scales, 64 rows of integer x and the f64 reference of one (N, K): computed once, shared, never changed."""
    if (N, K) not in _EXACT:
        wq, ws = _random_codes(N, K, device, 710 + N)
        g = torch.Generator(device="cpu").manual_seed(711 + K)
        x = torch.randint(-8, 9, (64, K), generator=g).to(torch.bfloat16).to(device)
        deq = hip.dequantize_mxfp4(wq, ws).double()
        ref = x.double() @ deq.t()
        # every product is a multiple of 2^-3; below 2^21 every partial sum in ANY order is exact in f32
        bound = float((x.double().abs() @ deq.abs().t()).max())
        _EXACT[(N, K)] = (wq, ws, x, ref, bound)
    return _EXACT[(N, K)]


SMALL = [(128, 64), (1000, 704), (260, 2112)]         # one tile one step / ragged column tile, tiny-model K / 4-column tile
LARGE = [(4608, 3584), (132, 18944)]                  # 7B qkv / down-projection K, many slots per tile
EXACT_CASES = [(N, K, B) for N, K in SMALL for B in (5, 16, 17, 32, 33, 64)] + \
              [(N, K, B) for N, K in LARGE for B in (5, 33, 64)]


@pytest.mark.parametrize("N,K,B", EXACT_CASES)
def test_exact_sums(hip, device, N, K, B):
    """Integer x in [-8, 8], codes times 2^-2..2^2: the slots of ``part`` summed on the host in f64 equal the f64 reference
    exactly, whatever the MFMA's internal order and the stream-K cut.  With ksplit = 16 every slot from the geometry's
    count up is all zero.  Rows >= B of a slab are not read back."""
    wq, ws, x64, ref, bound = _exact_case(hip, device, N, K)
    assert bound < 2 ** 21
    x = x64[:B]
    R = hip.part_rows(B)
    need = hip.decode_gemm_mxfp4_ksplit(N, K)
    part = _part(hip, B, N, device)
    assert hip.decode_gemm_mxfp4(x, wq, ws, part=part, ksplit=SLOTS) == SLOTS
    slabs = part.view(SLOTS, R, N)[:, :B]
    assert bool(torch.isfinite(slabs).all()), "a slot was left unwritten"
    got = slabs.double().sum(0)
    assert torch.equal(got, ref[:B]), f"max err {float((got - ref[:B]).abs().max())}"
    assert bool((slabs[need:] == 0).all()), "slots past the geometry's count must be zero-filled"
    if N <= 1000:       # a padded code / scale layout (ldq > K/2, lds > K/32, 0xFF fill) reads the same elements
        wide = torch.full((N, K // 2 + 16), 0xFF, dtype=torch.uint8, device=device)
        wide[:, :K // 2] = wq
        swide = torch.full((N, K // 32 + 3), 0xFF, dtype=torch.uint8, device=device)
        swide[:, :K // 32] = ws
        part2 = _part(hip, B, N, device)
        assert hip.decode_gemm_mxfp4(x, wide[:, :K // 2], swide[:, :K // 32], part=part2) == need
        assert torch.equal(part2.view(SLOTS, R, N)[:need, :B], slabs[:need])


# ----------------------------------------------------------------------------- 3. direct output
@pytest.mark.parametrize("N,K,B,dt", [(512, 256, 7, torch.float32), (1000, 704, 20, torch.float32),
                                      (1024, 704, 40, torch.bfloat16)])
def test_direct_output(hip, device, N, K, B, dt):
    """part=None: C written directly, exact on the integer inputs (bf16: the exact f32 sum rounded once); columns >= N of
    a wider ldc keep the sentinel."""
    wq, ws, x64, ref, bound = _exact_case(hip, device, N, K)
    assert bound < 2 ** 21
    wide = torch.full((B, N + 8), -777.0, dtype=dt, device=device)
    hip.decode_gemm_mxfp4(x64[:B], wq, ws, out=wide[:, :N])
    want = ref[:B].float()
    assert torch.equal(wide[:, :N].float(), want.to(dt).float())
    assert bool((wide[:, N:] == -777.0).all()), "columns past N were written"
    tight = torch.full((B, N), -777.0, dtype=dt, device=device)
    hip.decode_gemm_mxfp4(x64[:B], wq, ws, out=tight)
    assert torch.equal(tight, wide[:, :N])


# ----------------------------------------------------------------------------- 4. invariance inside the family
@pytest.mark.parametrize("N,K", [(1408, 256), (256, 704)])
@pytest.mark.parametrize("mode", ["plain", "bias", "residual+norm", "swiglu"])
def test_row_bits_do_not_depend_on_batch_or_position(hip, device, N, K, mode):
    """Random bf16 x: one row computed in a batch of 5, of 17 at another position, of 33 and of 64 gives bit-identical
    skinny_finalize output (K order and stream-K cut depend on (N, K) alone; MB changes the slab height only)."""
    from vision_inspection_system_amd.weights import interleave_gate_up
    w = _randn((N, K), device, 720, 1.0 / math.sqrt(K))
    if mode == "swiglu":
        w = interleave_gate_up(w[:N // 2].contiguous(), w[N // 2:].contiguous())
    wq, ws = hip.quantize_mxfp4_rows(w)
    xs = _randn((64, K), device, 721, 2.0)
    n_out = N // 2 if mode == "swiglu" else N
    bias = _randn((N,), device, 722) if mode == "bias" else None
    res_row = _randn((1, n_out), device, 723)
    nw = _randn((N,), device, 724)
    row = xs[3:4]
    outs = []
    for B, pos in ((5, 3), (17, 11), (33, 30), (64, 63)):
        x = xs[:B].clone()
        x[pos] = row[0]
        if pos != 3:
            x[3] = xs[40]
        part = _part(hip, B, N, device)
        ks = hip.decode_gemm_mxfp4(x, wq, ws, part=part)
        y = torch.empty((B, n_out), dtype=torch.bfloat16, device=device)
        if mode == "residual+norm":
            res = _randn((B, n_out), device, 725 + B)
            res[pos] = res_row[0]
            yn = torch.empty_like(y)
            hip.skinny_finalize(part, ks, y, N, residual=res, norm_w=nw, yn=yn)
            outs.append(torch.cat([y[pos], yn[pos]]))
        else:
            hip.skinny_finalize(part, ks, y, N, bias=bias, swiglu=(mode == "swiglu"))
            outs.append(y[pos].clone())
    assert float(outs[0].float().abs().max()) > 0
    for o, B in zip(outs[1:], (17, 33, 64)):
        assert torch.equal(o, outs[0]), f"row differs between a batch of 5 and a batch of {B}"


# ----------------------------------------------------------------------------- 5. against the bf16 kernel
def test_against_bf16_projection_on_dequantised_weights(hip, device):
    """Same bf16 numbers on both sides (the de-quantised weights are exact bf16), only the summation order differs: within
    the tolerance tests/test_kernels_gpu.py applies to decode_gemm against fp32 (atol 4e-2, rtol 1e-2)."""
    B, N, K = 64, 4608, 3584
    x = _randn((B, K), device, 730, 2.0)
    w = _randn((N, K), device, 731, 1.0 / math.sqrt(K))
    b = _randn((N,), device, 732)
    r = _randn((B, N), device, 733)
    wq, ws = hip.quantize_mxfp4_rows(w)
    deq = hip.dequantize_mxfp4(wq, ws)
    wb = deq.bfloat16()
    assert torch.equal(wb.float(), deq)
    y4 = _finalized(hip, x, wq, ws, bias=b, residual=r)
    part = _part(hip, B, N, device)
    ks = hip.decode_gemm(x, wb, part=part)
    yb = torch.empty((B, N), dtype=torch.bfloat16, device=device)
    hip.skinny_finalize(part, ks, yb, N, bias=b, residual=r)
    _assert_close(y4, yb, atol=4e-2, rtol=1e-2, what="decode gemm mxfp4 vs bf16 on de-quantised weights")
    _assert_close(y4, x.float() @ deq.t() + b.float() + r.float(), atol=4e-2, rtol=1e-2, what="decode gemm mxfp4 vs fp32")


# ----------------------------------------------------------------------------- 6. engine
OTHERS = [([256, 72, 105, 33, 90, 41], []), None, ([256, 80, 81, 82], []), None, ([256, 99, 98, 97, 96], []),
          ([256, 70, 71], []), ([256, 60, 61, 62, 63, 64, 65], [])]


def _others(ids, fa):
    o = list(OTHERS)
    o[1], o[3] = (ids[:-1] + [77, 10], fa), (ids[:-2] + [65, 66], fa)
    return o


@pytest.fixture(scope="module")
def setup(device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    w = pack_device_weights(cfg, sd, device)
    kw = dict(max_ctx=256, decode_splits=4, max_batch=8, decode_weights="mxfp4")
    eng = Qwen2VLEngine(cfg, w, device, mxfp4_gemm_from=5, **kw)
    plain = Qwen2VLEngine(cfg, w, device, **kw)
    for e in (eng, plain):
        e.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    assert eng.mxfp4_gemm_from == 5 and plain.mxfp4_gemm_from is None
    assert hasattr(eng, "b_part") and not hasattr(plain, "b_part"), "without the switch nothing more is allocated"
    return cfg, sd, eng, plain


def test_engine_batch_of_six_matches_oracle(setup, device):
    """The oracle runs the per-token steps on the de-quantised MXFP4 weights: logits of the first MFMA step within LOGIT_TOL,
    tokens equal to the oracle's where its top-2 margin exceeds the tolerance."""
    from oracle import qwen2vl_ref as R
    cfg, sd, eng, _ = setup
    g = load_golden()
    ids, fr = g["ids_a"].tolist(), [g["frame_a"]]
    fa = [torch.from_numpy(f).to(device) for f in fr]
    pv, grids = oracle_inputs(fr)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, 12, decode_sd=_dequantised_sd(cfg, sd))
    reqs = _others(ids, fa)[:5]
    reqs.insert(2, (ids, fa))
    got = eng.generate_batch(reqs, max_new_tokens=2, ignore_eos=True, use_graph=False)
    assert _check_tokens(got[2], ref_toks[:2], ref_logits) >= 1
    err = float(np.abs(eng.logits_b[2].float().cpu().numpy() - ref_logits[1].numpy()).max())
    print(f"first MFMA mxfp4 step, batch of 6: max |logit - oracle| = {err:.5f}")
    assert err < LOGIT_TOL
    toks = eng.generate_batch(reqs, max_new_tokens=12, ignore_eos=True)[2]
    same = _check_tokens(toks, ref_toks, ref_logits)
    print(f"tokens equal to the oracle's up to {same} of 12")
    assert same >= 4


def test_engine_in_family_batches_are_bit_identical(setup, device):
    """The same request in batches of 5, 6 and 8 at different positions: identical tokens and logits rows."""
    cfg, sd, eng, _ = setup
    ids, fa = _requests(device)
    first = None
    for n, pos in ((5, 0), (6, 4), (8, 7), (8, 2)):
        reqs = _others(ids, fa)[:n - 1]
        reqs.insert(pos, (ids, fa))
        got = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
        cur = (got[pos], eng.logits_b[pos].clone())
        assert len(got[pos]) == 8 and len({tuple(t) for t in got}) > 1
        if first is None:
            first = cur
        assert cur[0] == first[0], f"batch of {n}, row {pos}: tokens differ"
        assert torch.equal(cur[1], first[1]), f"batch of {n}, row {pos}: final logits differ"


def test_engine_below_threshold_is_untouched(setup, device):
    """Alone and in a batch of 3 the engine with the switch equals the engine without it, bit for bit (GEMV family)."""
    cfg, sd, eng, plain = setup
    ids, fa = _requests(device)
    a = eng.generate(ids, fa, max_new_tokens=8, ignore_eos=True)
    la = eng.logits.clone()
    b = plain.generate(ids, fa, max_new_tokens=8, ignore_eos=True)
    assert a == b and torch.equal(la, plain.logits)
    reqs = [_others(ids, fa)[0], (ids, fa), _others(ids, fa)[1]]
    a3 = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
    l3 = eng.logits_b[:3].clone()
    b3 = plain.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
    assert a3 == b3 and torch.equal(l3, plain.logits_b[:3])
    assert a3[1] == a


def test_engine_graph_replay_equals_eager_and_fold_equals_two_launches(setup, device):
    cfg, sd, eng, _ = setup
    ids, fa = _requests(device)
    reqs = _others(ids, fa)[:5] + [(ids, fa)]
    replayed = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
    eager = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True, use_graph=False)
    assert replayed == eager
    logits = eng.logits_b[:6].clone()
    keep = eng.fold_qkv
    try:
        for fold in (False, True):       # VIS_QKV_FOLD=0 / =1
            eng.fold_qkv = fold
            assert eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True, use_graph=False) == eager
            assert torch.equal(eng.logits_b[:6], logits), f"fold_qkv={fold}"
    finally:
        eng.fold_qkv = keep


def test_engine_request_switches_travel_with_the_request(setup, device):
    """top_p + seeds + per-request repetition penalties + stop + logprobs=2 in a batch of 6, against batches of 6 in which
    every request, with its own seed and penalty, sits in another row (rotated by 1 and by 3, and reversed; not one at a
    time - that is the GEMV family): same tokens and the same last_finish for every request."""
    cfg, sd, eng, _ = setup
    ids, fa = _requests(device)
    reqs = [(ids, fa)] + _others(ids, fa)[:5]
    seeds = [11, 12, 13, 14, 15, 16]
    rps = [1.3, 1.0, 1.2, 1.1, 1.3, 1.05]
    kw = dict(max_new_tokens=16, ignore_eos=True, temperature=0.8, top_p=0.9, logprobs=2)
    free = eng.generate_batch(reqs, seeds=seeds, repetition_penalty=rps, **kw)
    tb = [eng.tokenizer.token_bytes(t) for t in free[0]]
    have = [i for i in range(4, 12) if tb[i] and free[0][i] not in cfg.eos_ids]
    assert have, "no token with bytes to stop on"
    stops = [tb[have[0]], b"\x00\x00never\x00"]
    base = eng.generate_batch(reqs, seeds=seeds, repetition_penalty=rps, stop=stops, **kw)
    fin, lps = list(eng.last_finish), list(eng.last_logprobs)
    assert fin[0][0] == "stop" and len(base[0]) < 16
    for order in ([1, 2, 3, 4, 5, 0], [3, 4, 5, 0, 1, 2], [5, 4, 3, 2, 1, 0]):
        got = eng.generate_batch([reqs[i] for i in order], seeds=[seeds[i] for i in order],
                                 repetition_penalty=[rps[i] for i in order], stop=stops, **kw)
        for row, i in enumerate(order):
            assert got[row] == base[i], f"request {i} in row {row}"
            assert eng.last_finish[row] == fin[i], f"request {i} in row {row}: finish"
            lp = eng.last_logprobs[row]
            assert np.array_equal(lp.token_logprobs, lps[i].token_logprobs) and np.array_equal(lp.top_ids, lps[i].top_ids)


def test_engine_without_the_switch_launches_what_it_did(setup, device, monkeypatch):
    """decode_weights="mxfp4" without mxfp4_gemm_from: a step of 6 sequences never calls the MFMA projection and issues
    2 * (4 * layers + 1) multi-row GEMVs (two groups of rows per projection), as before."""
    from vision_inspection_system_amd import hip as H
    cfg, sd, eng, plain = setup
    ids, fa = _requests(device)
    reqs = [(ids, fa)] + _others(ids, fa)[:5]
    n = {"gemm": 0, "rows": 0}
    real_gemm, real_rows = H.decode_gemm_mxfp4, H.gemv_mxfp4_rows

    def gemm(*a, **k):
        n["gemm"] += 1
        return real_gemm(*a, **k)

    def rows(*a, **k):
        n["rows"] += 1
        return real_rows(*a, **k)

    monkeypatch.setattr(H, "decode_gemm_mxfp4", gemm)
    monkeypatch.setattr(H, "gemv_mxfp4_rows", rows)
    plain.generate_batch(reqs, max_new_tokens=2, ignore_eos=True, use_graph=False)      # exactly one decode step
    assert n == {"gemm": 0, "rows": 2 * (4 * cfg.layers + 1)}
    n["rows"] = 0
    eng.generate_batch(reqs, max_new_tokens=2, ignore_eos=True, use_graph=False)
    assert n == {"gemm": 4 * cfg.layers + 1, "rows": 0}
