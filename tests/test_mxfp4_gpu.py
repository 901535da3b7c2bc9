"""MXFP4 decode weights on the GPU: vis_gemv_mxfp4w / vis_gemv_mxfp4w_rows against hip.dequantize_mxfp4 (exactly where the
arithmetic is exact, within the fp8 GEMV tests' tolerances where bf16 / f32 rounding enters), and the Qwen2-VL engine with
decode_weights="mxfp4" against the oracle run on the de-quantised weights, alone, batched, graph-replayed and with the
request switches on."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden, oracle_inputs, ref_config

pytestmark = pytest.mark.gpu
LOGIT_TOL = 6e-2          # the engine tests' value: the oracle sees the same de-quantised weights, so only the kernel differs


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _randn(shape, device, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(device)


def _assert_close(got, ref, atol, rtol, what):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, max err {err.max().item():.6f}"


def _random_codes(N, K, device, seed):
    """Random E2M1 codes (all sixteen, -0 included) and scale bytes 125..129 (X = 1/4 .. 4)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    wq = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8).to(device)
    ws = torch.randint(125, 130, (N, K // 32), generator=g, dtype=torch.uint8).to(device)
    return wq, ws


# ----------------------------------------------------------------------------- kernel: exact
def test_element_order_one_hot(hip, device):
    """x = e_k picks column k of the de-quantised matrix: catches nibble, byte_sel and scale-index mistakes, bit for bit."""
    N, K = 16, 64
    wq, ws = _random_codes(N, K, device, 300)
    deq = hip.dequantize_mxfp4(wq, ws)
    assert len(torch.unique(wq & 15)) == 16 and len(torch.unique(ws)) > 1
    got = torch.empty((K, N), dtype=torch.float32, device=device)
    eye = torch.eye(K, dtype=torch.bfloat16, device=device)
    for k in range(K):
        hip.gemv_mxfp4(eye[k], wq, ws, got[k])
    # (value equality: code 8, -0, decodes to 0 and the f32 sum 0 + (-0) is +0)
    assert torch.equal(got.t(), deq), "y(e_k) must be column k of dequantize_mxfp4"


@pytest.mark.parametrize("N,K", [(8, 32), (1002, 704), (260, 2080), (96, 8192), (130, 18944), (8200, 96)])
def test_exact_sums(hip, device, N, K):
    """Integer x in [-8, 8], E2M1 codes times 2^-2..2^2: every product is a multiple of 2^-3, and so is every partial sum;
    below 2^21 (24 significand bits) a sum is exact in f32 in ANY order, so y must equal the f64 reference bit for bit.
    The bound on every partial sum in any order is sum_k |w x| <= 6 * 4 * 8 * K; asserted on the actual inputs.
    (8, 32): one block, fewer rows than a task.  (1002, 704): row tail, 22 blocks on 64 lanes.  (260, 2080): 65 blocks -
    lane wrap plus a clamped block.  (96, 8192): the long-row task shape.  (130, 18944): down-projection K.
    (8200, 96): the eight-row task shape (more than 8192 rows) with a row tail."""
    wq, ws = _random_codes(N, K, device, 310 + N)
    g = torch.Generator(device="cpu").manual_seed(311 + K)
    x = torch.randint(-8, 9, (K,), generator=g).to(torch.bfloat16).to(device)
    deq = hip.dequantize_mxfp4(wq, ws).double()
    ref = deq @ x.double()
    assert float((deq.abs() @ x.double().abs()).max()) < 2 ** 21
    assert float(ref.abs().max()) < 2 ** 21
    y = torch.full((N,), 7.0, dtype=torch.float32, device=device)
    hip.gemv_mxfp4(x, wq, ws, y)
    assert torch.equal(y.double(), ref), f"max err {float((y.double() - ref).abs().max())}"
    # a padded weight / scale layout (ldq > K/2, lds > K/32) reads the same elements
    if N <= 260:
        wide = torch.full((N, K // 2 + 16), 0xFF, dtype=torch.uint8, device=device)
        wide[:, :K // 2] = wq
        swide = torch.full((N, K // 32 + 3), 0xFF, dtype=torch.uint8, device=device)
        swide[:, :K // 32] = ws
        y2 = torch.empty_like(y)
        hip.gemv_mxfp4(x, wide[:, :K // 2], swide[:, :K // 32], y2)
        assert torch.equal(y2, y)


# ----------------------------------------------------------------------------- kernel: options (test_gemv_fp8_weights' form)
@pytest.mark.parametrize("N,K", [(1002, 704), (4608, 3584)])
def test_gemv_mxfp4_weights_bias_residual(hip, device, N, K):
    """Against the SAME quantised weights de-quantised in fp32: the kernel's only rounding is bf16 x, f32 sums, bf16 y."""
    x = _randn((K,), device, 320)
    w = _randn((N, K), device, 321, 1.0 / math.sqrt(K))
    b = _randn((N,), device, 322)
    r = _randn((N,), device, 323)
    wq, ws = hip.quantize_mxfp4_rows(w)
    assert wq.dtype == torch.uint8 and wq.shape == (N, K // 2) and ws.shape == (N, K // 32)
    cq, cs = hip.quantize_mxfp4_rows(w.cpu())
    assert torch.equal(cq, wq.cpu()) and torch.equal(cs, ws.cpu()), "CPU and GPU quantiser bytes differ"
    out = torch.empty((N,), dtype=torch.bfloat16, device=device)
    hip.gemv_mxfp4(x, wq, ws, out, bias=b, residual=r)
    deq = hip.dequantize_mxfp4(wq, ws)
    _assert_close(out, deq @ x.float() + b.float() + r.float(), atol=3e-2, rtol=1e-2, what="gemv mxfp4")
    X = torch.ldexp(torch.ones_like(ws, dtype=torch.float32), ws.int() - 127).repeat_interleave(32, dim=1)
    assert ((deq - w.float()).abs() <= X).all()


def test_gemv_mxfp4_fused_rmsnorm_swiglu_f32(hip, device):
    from vision_inspection_system_amd.weights import interleave_gate_up
    K, I = 256, 704
    x = _randn((K,), device, 324, 2.0)
    nw = _randn((K,), device, 325)
    wg = _randn((I, K), device, 326, 1.0 / math.sqrt(K))
    wu = _randn((I, K), device, 327, 1.0 / math.sqrt(K))
    wq, ws = hip.quantize_mxfp4_rows(interleave_gate_up(wg, wu))
    out = torch.empty((I,), dtype=torch.bfloat16, device=device)
    hip.gemv_mxfp4(x, wq, ws, out, norm_w=nw, act=hip.ACT_SWIGLU, eps=1e-6)
    xf = x.float()
    xn = ((xf * torch.rsqrt(xf.pow(2).mean() + 1e-6)).to(torch.bfloat16).float() * nw.float()).to(torch.bfloat16).float()
    d = hip.dequantize_mxfp4(wq, ws).view(I // 16, 2, 16, K)
    g, u = d[:, 0].reshape(I, K) @ xn, d[:, 1].reshape(I, K) @ xn
    _assert_close(out, torch.nn.functional.silu(g) * u, atol=2e-2, rtol=1e-2, what="gemv mxfp4 swiglu")
    N = 1536
    w = _randn((N, K), device, 328, 1.0 / math.sqrt(K))
    wq, ws = hip.quantize_mxfp4_rows(w)
    o32 = torch.empty((N,), dtype=torch.float32, device=device)
    hip.gemv_mxfp4(x, wq, ws, o32, norm_w=nw, eps=1e-6)
    _assert_close(o32, hip.dequantize_mxfp4(wq, ws) @ xn, atol=2e-2, rtol=1e-2, what="gemv mxfp4 f32 out")


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("N,K,act,fused", [(1024, 704, 0, "norm+bias"), (256, 8192, 0, "residual"),
                                           (16448, 256, 3, "norm"), (1000, 704, 0, "f32"), (3584, 18944, 0, "residual")])
def test_rows_bit_identical_to_single_row(hip, device, B, N, K, act, fused):
    """vis_gemv_mxfp4w_rows: every row equals vis_gemv_mxfp4w on it bit for bit - each of the three task shapes (few short
    rows, long rows, more than 8192 SwiGLU outputs), a ragged f32 case, and the 7B down projection (4 x 37 KiB of LDS)."""
    g = torch.Generator(device="cpu").manual_seed(N + K + B)
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(device)
    x = torch.randn((B, K), generator=g).to(torch.bfloat16).to(device)
    n_out = N // 2 if act == 3 else N
    bias = torch.randn((N,), generator=g).to(torch.bfloat16).to(device) if "bias" in fused else None
    nw = (1 + 0.1 * torch.randn((K,), generator=g)).to(torch.bfloat16).to(device) if "norm" in fused else None
    res = torch.randn((B, n_out), generator=g).to(torch.bfloat16).to(device) if "residual" in fused else None
    odt = torch.float32 if fused == "f32" else torch.bfloat16
    wq, ws = hip.quantize_mxfp4_rows(w)
    many = torch.full((B, n_out), 9.0, dtype=odt, device=device)
    hip.gemv_mxfp4_rows(x, wq, ws, many, bias=bias, residual=res, norm_w=nw, act=act)
    for b in range(B):
        one = torch.empty((n_out,), dtype=odt, device=device)
        hip.gemv_mxfp4(x[b], wq, ws, one, bias=bias, residual=res[b] if res is not None else None, norm_w=nw, act=act)
        assert torch.equal(many[b], one), f"row {b} of {B} differs from the single-row kernel"
    assert float(many.float().abs().max()) > 0


def test_argument_errors_launch_nothing(hip, device):
    """K = 48, a null Ws, ldq = K/2 + 8 and lds < K/32: VIS_ERR_ARG (status 1) from the host checks, y untouched."""
    lib = hip.load()
    N, K = 16, 64
    wq = torch.zeros((N, 64), dtype=torch.uint8, device=device)
    ws = torch.full((N, 4), 127, dtype=torch.uint8, device=device)
    x = torch.ones((4, 64), dtype=torch.bfloat16, device=device)
    y = torch.full((4, N), 5.0, dtype=torch.float32, device=device)
    p, st = hip._ptr, hip._stream()

    def one(k, ldq, lds, s=ws):
        return lib.vis_gemv_mxfp4w(p(x), p(wq), p(s), None, None, None, p(y), N, k, ldq, lds, 0, 1, 1e-6, st)

    def rows(k, ldq, lds, s=ws):
        return lib.vis_gemv_mxfp4w_rows(p(x), p(wq), p(s), None, None, None, p(y), 2, N, k, ldq, lds, 64, N, 0, 0, 1, 1e-6, st)

    for f in (one, rows):
        assert f(48, 32, 2) == 1, "K % 32 != 0"
        assert f(K, 32, 2, s=None) == 1, "null Ws"
        assert f(K, K // 2 + 8, 2) == 1, "ldq % 16 != 0"
        assert f(K, 32, 1) == 1, "lds < K/32"
        assert f(K, 16, 2) == 1, "ldq < K/2"
    assert lib.vis_gemv_mxfp4w_rows(p(x), p(wq), p(ws), None, None, None, p(y), 5, N, K, 32, 2, 64, N, 0, 0, 1, 1e-6, st) == 1
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())
    assert one(K, 64, 4) == 0 and rows(K, 64, 4) == 0          # and the same call with sound strides runs
    torch.cuda.synchronize()
    assert bool((y[:2] == 0.0).all()) and bool((y[2:] == 5.0).all())


# ----------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def setup(device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    w = pack_device_weights(cfg, sd, device)
    eng4 = Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_splits=4, max_batch=6, decode_weights="mxfp4")
    eng4.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    eng16 = Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_splits=4)
    return cfg, sd, eng4, eng16


def _dequantised_sd(cfg, sd):
    """State dict whose LLM projections / lm_head are the engine's MXFP4 weights, de-quantised (CPU, same quantiser);
    gate/up is quantised in the engine's 16-row interleaved layout, as helpers.dequantised_sd does for e4m3."""
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.weights import interleave_gate_up

    def dq(w):
        return hip.dequantize_mxfp4(*hip.quantize_mxfp4_rows(w.to(torch.bfloat16)))

    dsd = dict(sd)
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        qkv = dq(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in ("q", "k", "v")], dim=0))
        nq, nk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        dsd[p + "self_attn.q_proj.weight"], dsd[p + "self_attn.k_proj.weight"], dsd[p + "self_attn.v_proj.weight"] = \
            qkv[:nq], qkv[nq:nq + nk], qkv[nq + nk:]
        dsd[p + "self_attn.o_proj.weight"] = dq(sd[p + "self_attn.o_proj.weight"])
        gu = dq(interleave_gate_up(sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]))
        gu = gu.view(cfg.intermediate // 16, 2, 16, cfg.hidden)
        dsd[p + "mlp.gate_proj.weight"] = gu[:, 0].reshape(cfg.intermediate, cfg.hidden)
        dsd[p + "mlp.up_proj.weight"] = gu[:, 1].reshape(cfg.intermediate, cfg.hidden)
        dsd[p + "mlp.down_proj.weight"] = dq(sd[p + "mlp.down_proj.weight"])
    dsd["lm_head.weight"] = dq(sd["lm_head.weight"])
    return dsd


def _check_tokens(toks, ref_toks, ref_logits):
    for i, (a, b) in enumerate(zip(toks, ref_toks)):
        if a != b:
            top2 = torch.topk(ref_logits[i], 2).values
            margin = float(top2[0] - top2[1])
            assert margin < 2 * LOGIT_TOL, f"token {i}: got {a}, oracle {b}, oracle margin {margin:.4f} is not a near-tie"
            return i
    return len(ref_toks)


def _requests(device):
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    ids = g["ids_a"].tolist()
    return ids, fa


def test_mxfp4_decode_weights_match_oracle_with_dequantised_weights(setup, device):
    """The oracle runs the prompt on the original weights and the per-token steps on the DE-QUANTISED MXFP4 weights (same
    quantiser, CPU), so the comparison isolates the kernel: logits of the first mxfp4 step within LOGIT_TOL, tokens equal
    up to a near-tie; and MXFP4 really changes the arithmetic."""
    from oracle import qwen2vl_ref as R
    cfg, sd, eng, eng16 = setup
    assert len(eng.q4) == cfg.layers and eng.q4[0]["gateup_w"][0].dtype == torch.uint8
    g = load_golden()
    ids, fr = g["ids_a"].tolist(), [g["frame_a"]]
    dev_fr = [torch.from_numpy(f).to(device) for f in fr]
    dsd = _dequantised_sd(cfg, sd)
    pv, grids = oracle_inputs(fr)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, 12, decode_sd=dsd)
    eng.prefill(ids, dev_fr)
    eng.decode(1, use_graph=False)
    err = float(np.abs(eng.logits.float().cpu().numpy() - ref_logits[1].numpy()).max())
    print(f"first mxfp4 step: max |logit - oracle| = {err:.5f}")
    assert err < LOGIT_TOL
    toks = eng.generate(ids, dev_fr, max_new_tokens=12, ignore_eos=True)
    same = _check_tokens(toks, ref_toks, ref_logits)
    print(f"tokens equal to the oracle's up to {same} of 12")
    assert same >= 4
    eng.prefill(ids, dev_fr)
    eng.decode(1, use_graph=False)
    eng16.prefill(ids, dev_fr)
    eng16.decode(1, use_graph=False)
    assert (eng16.logits - eng.logits).abs().max() > 1e-3


def test_batch_invariance_alone_three_six(setup, device):
    """The same request alone, in a batch of 3 and in a batch of 6 (one group of 4 rows + a 2-row remainder): tokens and
    final logits bit-equal."""
    cfg, sd, eng, _ = setup
    ids, fa = _requests(device)
    others = [([256, 72, 105, 33, 90, 41], []), (ids[:-1] + [77, 10], fa), ([256, 80, 81, 82], []),
              (ids[:-2] + [65, 66], fa), ([256, 99, 98, 97, 96], [])]
    alone = eng.generate(ids, fa, max_new_tokens=8, ignore_eos=True)
    logits_alone = eng.logits.clone()
    assert len(alone) == 8
    for n in (3, 6):
        for pos in (0, n - 1):      # first row of the first group / last row of the remainder group
            reqs = list(others[:n - 1])
            reqs.insert(pos, (ids, fa))
            got = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
            assert got[pos] == alone, f"batch of {n}, row {pos}"
            assert torch.equal(eng.logits_b[pos], logits_alone), f"batch of {n}, row {pos}: final logits differ"
            assert len({tuple(t) for t in got}) > 1


def test_graph_replay_equals_eager(setup, device):
    cfg, sd, eng, _ = setup
    ids, fa = _requests(device)
    replayed = eng.generate(ids, fa, max_new_tokens=12, ignore_eos=True)
    eager = eng.generate(ids, fa, max_new_tokens=12, ignore_eos=True, use_graph=False)
    assert replayed == eager and len(eager) == 12
    reqs = [(ids, fa), ([256, 72, 105, 33, 90, 41], []), (ids[:-1] + [77, 10], fa), ([256, 80, 81, 82], []),
            (ids[:-2] + [65, 66], fa)]
    assert eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True) == \
        eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True, use_graph=False)


def test_request_switches_batched_equal_one_at_a_time(setup, device):
    """top_p + seeds + repetition_penalty + stop + logprobs=2 in one generate_batch on MXFP4 weights: every request's
    tokens, finish reason and log-probabilities equal the same request run alone."""
    cfg, sd, eng, _ = setup
    ids, fa = _requests(device)
    reqs = [(ids, fa), ([256, 72, 105, 33, 90, 41], []), (ids[:-1] + [77, 10], fa)]
    seeds = [11, 12, 13]
    kw = dict(max_new_tokens=16, ignore_eos=True, temperature=0.8, top_p=0.9, repetition_penalty=1.3, logprobs=2)
    free = eng.generate_batch(reqs, seeds=seeds, **kw)
    tb = [eng.tokenizer.token_bytes(t) for t in free[0]]
    have = [i for i in range(4, 12) if tb[i] and free[0][i] not in cfg.eos_ids]
    assert have, "no token with bytes to stop on"
    stops = [tb[have[0]], b"\x00\x00never\x00"]
    batch = eng.generate_batch(reqs, seeds=seeds, stop=stops, **kw)
    fin, lps = list(eng.last_finish), list(eng.last_logprobs)
    assert fin[0][0] == "stop" and len(batch[0]) < 16
    for i, (rid, rfr) in enumerate(reqs):
        one = eng.generate(rid, rfr, seed=seeds[i], stop=stops, **kw)
        assert one == batch[i], f"request {i}"
        assert eng.last_finish == [fin[i]]
        lp = eng.last_logprobs[0]
        assert np.array_equal(lp.token_logprobs, lps[i].token_logprobs) and np.array_equal(lp.top_ids, lps[i].top_ids)
        assert np.array_equal(lp.top_logprobs, lps[i].top_logprobs)
