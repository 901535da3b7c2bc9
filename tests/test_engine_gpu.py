"""End-to-end parity on MI355X: HIP engine (bf16 kernels through the C ABI) vs the fp32 oracle and
vs the transformers-recorded golden vectors, tiny kernel-compatible config.

Stated tolerance (north_star: "within a stated float tolerance on the logits"): first-step logits
within 6e-2 absolute (logit scale here is ~3, i.e. 2 % of range: bf16 activations through ~10
GEMM stages), image embeddings within 5e-2.  Token criterion: ALL 16 generated steps are checked with the
oracle's tokens teacher-forced (helpers.teacher_forced_parity): every step's logits within the tolerance and
every greedy pick equal to the oracle's unless the oracle's top-2 margin at that step is below 2x the tolerance
(a genuine near-tie); the free-running tokens must equal the oracle's up to the first such near-tie."""
import numpy as np
import pytest
import torch

from helpers import load_golden, oracle_inputs, ref_config, teacher_forced_parity, dequantised_sd as _dequantised_sd

pytestmark = pytest.mark.gpu
LOGIT_TOL = 6e-2


@pytest.fixture(scope="module")
def setup(device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, decode_splits=4)
    return cfg, sd, eng


def _check_tokens(toks, ref_toks, ref_logits):
    for i, (a, b) in enumerate(zip(toks, ref_toks)):
        if a != b:
            top2 = torch.topk(ref_logits[i], 2).values
            margin = float(top2[0] - top2[1])
            assert margin < 2 * LOGIT_TOL, f"token {i}: got {a}, oracle {b}, oracle margin {margin:.4f} is not a near-tie"
            return i
    return len(ref_toks)


@pytest.mark.parametrize("case,frames", [("a", ["frame_a"]), ("b", ["frame_b1", "frame_b2"])])
def test_engine_matches_oracle_and_golden(setup, device, case, frames):
    from oracle import qwen2vl_ref as R
    cfg, sd, eng = setup
    g = load_golden()
    fr = [g[n] for n in frames]
    ids = g[f"ids_{case}"].tolist()
    dev_frames = [torch.from_numpy(f).to(device) for f in fr]
    taps = {}
    eng.prefill(ids, dev_frames, taps=taps)
    eng.decode(15, use_graph=False)
    toks = eng.generated(16)
    img = taps["image_embeds"].float().cpu().numpy()
    logits = taps["first_logits"].float().cpu().numpy()
    # vs transformers-recorded vectors
    assert np.abs(img - g[f"{case}_image_embeds"]).max() < 5e-2
    assert np.abs(logits - g[f"{case}_first_logits"]).max() < LOGIT_TOL
    # vs the oracle run here on the same inputs
    pv, grids = oracle_inputs(fr)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, 16)
    assert np.abs(logits - ref_logits[0].numpy()).max() < LOGIT_TOL
    _check_tokens(toks, ref_toks, ref_logits)          # free-running: equal up to the first near-tie (asserted inside)
    # all 16 steps, teacher-forced: logits within tolerance and picks equal off near-ties at EVERY step
    eng.prefill(ids, dev_frames, taps=taps)
    ties = teacher_forced_parity(eng, taps["first_logits"], ref_toks, ref_logits, LOGIT_TOL)
    assert ties <= 2, f"{ties} near-tie steps in 16 is implausible for seeded weights"


def _outlier_state_dict(cfg, sd, compensated: bool):
    """Massive-activation channels, as real checkpoints have them: 4 hidden channels carry values x100 in the token
    embeddings and in the image features (merger output).  ``compensated``: the norm weights of those channels are
    small (what trained models do); otherwise the projections see the outliers at full size."""
    sd = {k: v.clone() for k, v in sd.items()}
    ch = [3, 77, 130, 201]
    sd["model.embed_tokens.weight"][:, ch] *= 100.0
    sd["visual.merger.mlp.2.weight"][ch, :] *= 100.0
    sd["visual.merger.mlp.2.bias"][ch] *= 100.0
    if compensated:
        for k in sd:
            if k.endswith("input_layernorm.weight") or k.endswith("post_attention_layernorm.weight") or k == "model.norm.weight":
                sd[k][ch] *= 0.02
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


@pytest.mark.parametrize("compensated", [True, False])
def test_outlier_channels_bf16(setup, device, compensated):
    """bf16 residual stream with 4 channels at ~+-170 next to O(1) channels (logit range grows to ~+-10..40): the
    tolerance is stated RELATIVE to the logit range - 2 % of max|oracle logit| - and all 12 steps are teacher-forced."""
    from oracle import qwen2vl_ref as R
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights
    cfg, sd0, _ = setup
    sd = _outlier_state_dict(cfg, sd0, compensated)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, decode_splits=4)
    g = load_golden()
    ids, fr = g["ids_a"].tolist(), [g["frame_a"]]
    pv, grids = oracle_inputs(fr)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, 12)
    rng_ = max(float(l.abs().max()) for l in ref_logits)
    taps = {}
    eng.prefill(ids, [torch.from_numpy(f).to(device) for f in fr], taps=taps)
    x = taps["layer0"].float().abs()
    assert float(x.max()) > 50.0                              # the outliers really are in the residual stream
    teacher_forced_parity(eng, taps["first_logits"], ref_toks, ref_logits, 0.02 * rng_)


@pytest.mark.parametrize("compensated", [True, False])
def test_outlier_channels_fp8(setup, device, compensated):
    """The same outlier model through the fp8 configuration (e4m3 weights with per-row scales, per-token e4m3
    activations): per-row amax scaling keeps the O(1) channels representable next to a 100x outlier (e4m3 is a
    floating-point format: 3 mantissa bits down to 2^-9 of the row maximum).  Statistical tolerance as for the plain
    fp8 test, relative to the logit range: mean |dlogit| < 2 %, max < 12 % of max|oracle logit| against the fake-quant
    oracle."""
    from oracle import qwen2vl_ref as R
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights
    cfg, sd0, _ = setup
    sd = _outlier_state_dict(cfg, sd0, compensated)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, decode_splits=4,
                        prefill_dtype="fp8", decode_weights="fp8")
    g = load_golden()
    ids, fr = g["ids_a"].tolist(), [g["frame_a"]]
    pv, grids = oracle_inputs(fr)
    dsd = _dequantised_sd(cfg, sd)
    psd = dict(dsd)
    psd["lm_head.weight"] = sd["lm_head.weight"]            # first token: bf16 lm_head
    _, l8 = R.generate(ref_config(cfg), sd, ids, pv, grids, 1, prefill_fp8_sd=psd)
    taps = {}
    eng.prefill(ids, [torch.from_numpy(f).to(device) for f in fr], taps=taps)
    got = taps["first_logits"].float().cpu()
    assert torch.isfinite(got).all()
    rng_ = float(l8[0].abs().max())
    e8 = (got - l8[0]).abs()
    print(f"[outlier fp8 compensated={compensated}] range {rng_:.2f} mean {float(e8.mean()) / rng_:.4f} max {float(e8.max()) / rng_:.4f}")
    assert e8.mean() < 0.02 * rng_ and e8.max() < 0.12 * rng_, (float(e8.mean()), float(e8.max()), rng_)
    toks = eng.generate(ids, [torch.from_numpy(f).to(device) for f in fr], max_new_tokens=6, ignore_eos=True)
    assert len(toks) == 6 and all(0 <= t < cfg.vocab for t in toks)


def test_graph_replay_equals_eager(setup, device):
    cfg, sd, eng = setup
    g = load_golden()
    ids = g["ids_a"].tolist()
    fr = [torch.from_numpy(g["frame_a"]).to(device)]
    eager = eng.generate(ids, fr, max_new_tokens=12, ignore_eos=True, use_graph=False)
    graph = eng.generate(ids, fr, max_new_tokens=12, ignore_eos=True, use_graph=True)
    again = eng.generate(ids, fr, max_new_tokens=12, ignore_eos=True, use_graph=True)
    assert eager == graph == again and len(graph) == 12


def test_text_only_prompt_and_eos(setup, device):
    from oracle import qwen2vl_ref as R
    cfg, sd, eng = setup
    ids = [256, 72, 105, 33]
    toks = eng.generate(ids, [], max_new_tokens=8, ignore_eos=True)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, None, [], 8)
    _check_tokens(toks, ref_toks, ref_logits)
    taps = {}
    eng.prefill(ids, [], taps=taps)
    teacher_forced_parity(eng, taps["first_logits"], ref_toks, ref_logits, LOGIT_TOL, use_graph=True)
    # EOS truncation: declare the 3rd generated token to be EOS
    import dataclasses
    eng.cfg = dataclasses.replace(cfg, eos_ids=(toks[2],))
    try:
        out = eng.generate(ids, [], max_new_tokens=8, check_every=2)
        assert out == toks[:2]
    finally:
        eng.cfg = cfg


def test_prompt_validation(setup):
    cfg, sd, eng = setup
    with pytest.raises(ValueError):
        eng.prefill([cfg.vocab + 5], [])
    with pytest.raises(ValueError):
        eng.prefill([256, cfg.image_token_id, 10], [])  # image token without an image


@pytest.mark.parametrize("fused", ["0", "1"])
def test_batched_generation_matches_single(device, monkeypatch, fused):
    """Batched decode (skinny MFMA GEMM, one weight pass for all sequences) vs the single-sequence GEMV path:
    same prompts -> same greedy tokens up to genuine near-ties (different summation order), and the
    first token (prefill path, identical code) must agree exactly.  fused = 1: the opt-in r05 step, every projection one
    launch (vis_decode_proj_*: in-kernel reduction or column slabs, RMSNorm split into column and row factors)."""
    monkeypatch.setenv("VIS_DECODE_FUSED", fused)
    from oracle import qwen2vl_ref as R
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=4)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    fb = [torch.from_numpy(g["frame_b1"]).to(device), torch.from_numpy(g["frame_b2"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fa), (g["ids_b"].tolist(), fb), ([256, 72, 105, 33], []), (g["ids_a"].tolist(), fa)]
    singles = [eng.generate(ids, fr, max_new_tokens=12, ignore_eos=True) for ids, fr in reqs]
    for use_graph in (False, True):
        batch = eng.generate_batch(reqs, max_new_tokens=12, ignore_eos=True, use_graph=use_graph)
        assert [len(t) for t in batch] == [12] * 4
        assert batch[0] == batch[3]                      # identical requests in different slots
        for b, (ids, fr) in enumerate(reqs):
            assert batch[b][0] == singles[b][0]
            frames_np = [f.cpu().numpy() for f in fr]
            pv, grids = oracle_inputs(frames_np) if frames_np else (None, [])
            ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, 12)
            assert _check_tokens(batch[b], ref_toks, ref_logits) >= 3, (b, batch[b], ref_toks)
    # a second batch after the first reuses the captured graph and the slots
    again = eng.generate_batch(reqs[:2], max_new_tokens=6, ignore_eos=True)
    assert again[0] == batch[0][:6] and again[1] == batch[1][:6]


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_rows_gemv_decode_equals_single_sequence_decode(device, monkeypatch, weights):
    """VIS_ROWS_GEMV=2 (opt-in): two in-flight sequences decode on vis_gemv_*_rows - per-row arithmetic of the
    single-sequence step, so tokens AND logits are exactly the single-sequence ones."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    monkeypatch.setenv("VIS_ROWS_GEMV", "2")
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=4,
                        decode_weights=weights)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fa), ([256, 72, 105, 33, 90, 41], [])]
    singles, logits = [], []
    for ids, fr in reqs:
        singles.append(eng.generate(ids, fr, max_new_tokens=10, ignore_eos=True))
        logits.append(eng.logits.clone())
    for use_graph in (False, True):
        pair = eng.generate_batch(reqs, max_new_tokens=10, ignore_eos=True, use_graph=use_graph)
        assert pair == singles
        for b in range(2):
            assert torch.equal(eng.logits_b[b], logits[b].view(-1)), f"sequence {b}: logits differ from the single-sequence step"


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_batched_generation_more_than_16_sequences(device, weights, monkeypatch, fused):
    """17..32 (33..64) in-flight sequences use two (four) 16-row MFMA blocks in the batched projection: the tokens of a
    request are the same as in a batch of <= 16 (rows are independent; the stream-K slot order depends on (N, K) only)."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    monkeypatch.setenv("VIS_DECODE_FUSED", fused)
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=64, decode_weights=weights)
    assert eng.fused_proj == (fused == "1")
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    fb = [torch.from_numpy(g["frame_b1"]).to(device), torch.from_numpy(g["frame_b2"]).to(device)]
    base = [(g["ids_a"].tolist(), fa), (g["ids_b"].tolist(), fb), ([256, 72, 105, 33], [])]
    small = eng.generate_batch(base, max_new_tokens=10, ignore_eos=True)
    for B in (17, 32, 40, 64):
        reqs = [base[i % 3] for i in range(B)]
        out = eng.generate_batch(reqs, max_new_tokens=10, ignore_eos=True)
        assert len(out) == B
        for i in range(B):
            assert out[i] == small[i % 3], f"B={B}: sequence {i} differs from the same request in a batch of 3"


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_shared_text_prefix_is_bit_identical(device, monkeypatch, dtype):
    """Batch inspection sends the same text in front of every image: prefill_many computes that prefix once and copies
    its K / V / V^T into every slot.  The tokens and the first-step logits must be exactly those of the unshared pass."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=512, max_batch=4,
                        prefill_dtype=dtype, decode_weights=dtype)
    eng.min_shared_prefix = 64
    g = load_golden()
    frames = [torch.from_numpy(g["frame_a"]).to(device), torch.from_numpy(g["frame_b1"]).to(device)]
    rng = np.random.default_rng(5)
    text = rng.integers(3, 200, 150).tolist()                      # 150 common text tokens -> shared prefix of 128

    def ids_for(f, tail):
        n = (f.shape[0] // cfg.patch) * (f.shape[1] // cfg.patch) // cfg.merge ** 2
        return text + [cfg.vision_start_id] + [cfg.image_token_id] * n + [cfg.vision_end_id] + tail

    reqs = [(ids_for(frames[0], [7, 8, 9]), [frames[0]]), (ids_for(frames[1], [11]), [frames[1]]),
            (ids_for(frames[0], [7, 8, 9]), [frames[0]])]
    assert eng.shared_prefix_len([r[0] for r in reqs]) == 128
    shared = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
    logits_shared = eng.logits_b[:3].clone()
    monkeypatch.setenv("VIS_SHARE_PREFIX", "0")
    assert eng.shared_prefix_len([r[0] for r in reqs]) == 0
    plain = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
    assert shared == plain
    assert torch.equal(logits_shared, eng.logits_b[:3])
    assert shared[0] == shared[2]
    # requests 0 and 2 have one prompt structure: their suffix rows ran as ONE stacked pass
    # (_prefill_group); forced apart (VIS_MERGE_PREFILL=0) the result is the same bit for bit - and so is a group of four
    monkeypatch.setenv("VIS_SHARE_PREFIX", "1")
    four = [(ids_for(frames[0], [7, 8, 9]), [frames[0]]), (ids_for(frames[0], [9, 9, 9]), [frames[0]]),
            (ids_for(frames[0], [1, 2, 3]), [frames[0]]), (ids_for(frames[0], [7, 8, 9]), [frames[0]])]
    calls = []
    real = eng._prefill_group
    monkeypatch.setattr(eng, "_prefill_group", lambda items, *a, **k: (calls.append(len(items)), real(items, *a, **k))[1])
    stacked = eng.generate_batch(four, max_new_tokens=8, ignore_eos=True)
    logits_stacked = eng.logits_b[:4].clone()
    assert calls == [4]
    monkeypatch.setenv("VIS_MERGE_PREFILL", "0")
    apart = eng.generate_batch(four, max_new_tokens=8, ignore_eos=True)
    # (every text pass is a group now: forced apart, the four ran as four groups of one - and the prefix came from the cache)
    assert calls == [4, 1, 1, 1, 1] and stacked == apart and torch.equal(logits_stacked, eng.logits_b[:4])
    assert stacked[0] == stacked[3] == shared[0]
    monkeypatch.delenv("VIS_MERGE_PREFILL")
    # prompts without a common text prefix, or with the image first, fall back to the plain pass
    assert eng.shared_prefix_len([[1, 2, 3] * 100, [4, 5, 6] * 100]) == 0
    assert eng.shared_prefix_len([[cfg.vision_start_id] + text, [cfg.vision_start_id] + text]) == 0


def test_fp8_decode_weights_match_oracle_with_dequantised_weights(setup, device):
    """BASELINE configs[4] slice: decode GEMVs on e4m3 weights.  The oracle runs the prompt on the original weights
    and the per-token steps on the DE-QUANTISED weights (same quantiser, CPU), so the comparison isolates the kernel:
    logits of the first fp8 step within LOGIT_TOL, tokens equal up to a near-tie."""
    from oracle import qwen2vl_ref as R
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import interleave_gate_up, pack_device_weights
    cfg, sd, _ = setup
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, decode_splits=4,
                        decode_weights="fp8")
    g = load_golden()
    ids = g["ids_a"].tolist()
    fr = [g["frame_a"]]

    dsd = _dequantised_sd(cfg, sd)
    pv, grids = oracle_inputs(fr)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, 12, decode_sd=dsd)
    eng.prefill(ids, [torch.from_numpy(f).to(device) for f in fr])
    eng.decode(1, use_graph=False)
    assert np.abs(eng.logits.float().cpu().numpy() - ref_logits[1].numpy()).max() < LOGIT_TOL
    toks = eng.generate(ids, [torch.from_numpy(f).to(device) for f in fr], max_new_tokens=12, ignore_eos=True)
    assert _check_tokens(toks, ref_toks, ref_logits) >= 4
    # and fp8 really changes the arithmetic: the bf16 engine's second-step logits differ measurably
    _, _, eng16 = setup
    eng16.prefill(ids, [torch.from_numpy(f).to(device) for f in fr])
    eng16.decode(1, use_graph=False)
    assert (eng16.logits - eng.logits).abs().max() > 1e-3


def test_vit_features_do_not_depend_on_batch_position(setup, device):
    """An image's features are bit-identical alone, second in a request, or batched behind other images: every image
    starts on a 64-row boundary, so the attention kernel's absolute 64-key tiles group its keys the same way."""
    cfg, sd, eng = setup
    rng = np.random.default_rng(5)
    fa = torch.from_numpy(rng.integers(0, 256, (28 * 5, 28 * 7, 3), dtype=np.uint8)).to(device)    # 140 patches
    fb = torch.from_numpy(rng.integers(0, 256, (28 * 3, 28 * 3, 3), dtype=np.uint8)).to(device)    # 36 patches
    na, nb = (10 * 14) // 4, (6 * 6) // 4
    a = eng.vision_forward([fa])
    b = eng.vision_forward([fb])
    assert a.shape[0] == na and b.shape[0] == nb
    mixed = eng.vision_forward([fb, fa, fb, fa])
    assert mixed.shape[0] == 2 * (na + nb)
    o = 0
    for ref in (b, a, b, a):
        assert torch.equal(mixed[o:o + ref.shape[0]], ref)
        o += ref.shape[0]


def test_fp8_prefill_matches_oracle_with_fake_quant(setup, device, monkeypatch):
    """configs[4]: LLM projections of the prompt pass on the fp8 MFMA (e4m3 weights, per-token e4m3 activations).
    The oracle fake-quantises the same tensors (de-quantised weights, per-row activation quantise/de-quantise).
    A quantiser is discontinuous: the bf16-level differences between the GPU pipeline and the fp32 oracle move some
    activations across e4m3 rounding boundaries (one step = 6 %), so the two fp8 results agree statistically, not
    element-wise - the element-wise checks are the kernel tests (test_gemm_fp8 / test_quant_rows_fp8, exact operands).
    Stated tolerance here: mean |dlogit| < 0.05, max < 0.35 (logit range +-3), and - on a text-only prompt, where both
    start from identical embeddings - closer to the fp8 oracle than to the bf16 oracle."""
    from oracle import qwen2vl_ref as R
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights
    cfg, sd, eng16 = setup
    monkeypatch.setenv("VIS_VIT_FP8", "1")      # exercise the (opt-in) fp8 ViT projections too
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, decode_splits=4,
                        prefill_dtype="fp8")
    assert eng.vq8
    g = load_golden()
    dsd = _dequantised_sd(cfg, sd)
    psd = dict(dsd)
    psd["lm_head.weight"] = sd["lm_head.weight"]            # first token: bf16 lm_head
    cases = [(g["ids_a"].tolist(), [g["frame_a"]]), ([256, 10, 20, 30] + list(range(40, 90)) + [257], [])]
    for ids, fr in cases:
        pv, grids = oracle_inputs(fr) if fr else (None, [])
        _, l8 = R.generate(ref_config(cfg), sd, ids, pv, grids, 1, prefill_fp8_sd=psd)
        _, l16 = R.generate(ref_config(cfg), sd, ids, pv, grids, 1)
        taps = {}
        eng.prefill(ids, [torch.from_numpy(f).to(device) for f in fr], taps=taps)
        got = taps["first_logits"].float().cpu()
        e8, e16 = (got - l8[0]).abs(), (got - l16[0]).abs()
        assert e8.mean() < 0.06 and e8.max() < 0.4, (float(e8.mean()), float(e8.max()))
        if not fr:
            assert e8.mean() < e16.mean()
        assert e16.max() > 1e-3                                 # really a different arithmetic from bf16
    toks = eng.generate(cases[0][0], [torch.from_numpy(f).to(device) for f in cases[0][1]], max_new_tokens=6,
                        ignore_eos=True)
    assert len(toks) == 6


@pytest.mark.parametrize("fused", ["0", "1"])
def test_fp8_batched_decode(device, monkeypatch, fused):
    """configs[4], batched decode on e4m3 weights + activations (fused = 1: the opt-in r05 step on MX activation blocks).  Invariants (the element-wise checks are the kernel
    tests): identical requests in different slots give identical tokens, graph replay == eager, the first token (bf16
    prefill + bf16-activation lm_head path of prefill) equals the single-sequence engine's, and the first batched step's
    logits stay within fp8 noise of the W8A16 single-sequence step (mean < 0.06, max < 0.4 on a +-3 logit range)."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    monkeypatch.setenv("VIS_DECODE_FUSED", fused)
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=4, decode_weights="fp8")
    assert eng.fp8_batched and eng.fused_proj == (fused == "1")
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fa), ([256, 72, 105, 33], []), (g["ids_a"].tolist(), fa)]
    eager = eng.generate_batch(reqs, max_new_tokens=10, ignore_eos=True, use_graph=False)
    graph = eng.generate_batch(reqs, max_new_tokens=10, ignore_eos=True, use_graph=True)
    assert eager == graph and eager[0] == eager[2] and [len(t) for t in eager] == [10] * 3
    single = eng.generate(reqs[0][0], fa, max_new_tokens=10, ignore_eos=True)
    assert single[0] == eager[0][0]
    # first decode step: batched (W8A8) vs single-sequence (W8A16) logits
    eng.prefill(reqs[0][0], fa)
    eng.decode(1, use_graph=False)
    l_single = eng.logits.float().clone()
    eng.prefill_many(reqs[:2])
    eng._decode_step_batched(2)
    d = (eng.logits_b[0].float() - l_single).abs()
    assert d.mean() < 0.06 and d.max() < 0.4, (float(d.mean()), float(d.max()))


def test_lazy_requests_stream_into_the_batch_and_failures_stay_per_request(device):
    """The batch seam hands generate_batch callables (each waits for its image's host decode): they are resolved in
    order, a ViT group at a time; the tokens are those of the eager call, a callable that raises leaves its exception in
    its place and takes no slot, and nothing is resolved before the request in front of it."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=8)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    fb = [torch.from_numpy(g["frame_b1"]).to(device), torch.from_numpy(g["frame_b2"]).to(device)]
    base = [(g["ids_a"].tolist(), fa), (g["ids_b"].tolist(), fb), ([256, 72, 105, 33], []), (g["ids_a"].tolist(), fa),
            (g["ids_b"].tolist(), fb), (g["ids_a"].tolist(), fa)]
    eager = eng.generate_batch(base, max_new_tokens=9, ignore_eos=True)
    order = []

    def lazy(i, fail=False):
        def resolve():
            order.append(i)
            if fail:
                raise ValueError(f"image {i} is corrupt")
            return base[i]
        return resolve

    out = eng.generate_batch([lazy(i) for i in range(6)], max_new_tokens=9, ignore_eos=True)
    assert out == eager and order == list(range(6))
    order.clear()
    out = eng.generate_batch([lazy(0), lazy(1, fail=True), lazy(2), lazy(3), lazy(4, fail=True), lazy(5)], max_new_tokens=9,
                             ignore_eos=True)
    assert isinstance(out[1], ValueError) and isinstance(out[4], ValueError) and "image 4" in str(out[4])
    survivors = eng.generate_batch([base[0], base[2], base[3], base[5]], max_new_tokens=9, ignore_eos=True)
    assert [out[0], out[2], out[3], out[5]] == survivors
    # everything fails / a single survivor / a single lazy request
    out = eng.generate_batch([lazy(0, fail=True), lazy(1, fail=True)], max_new_tokens=4, ignore_eos=True)
    assert all(isinstance(o, ValueError) for o in out)
    out = eng.generate_batch([lazy(0, fail=True), lazy(1)], max_new_tokens=6, ignore_eos=True)
    assert isinstance(out[0], ValueError) and out[1][0] == eager[1][0] and len(out[1]) == 6
    assert eng.generate_batch([lazy(3)], max_new_tokens=5, ignore_eos=True) == [eng.generate(*base[3], max_new_tokens=5, ignore_eos=True)]


def test_prefix_cache_across_requests_is_bit_identical(device, monkeypatch):
    """Prompt caching: the text in front of the image (the agents' fixed inspection prompt) is computed once and its K / V /
    V^T kept across requests (LRU).  A later single request computes only the rows from the image on - same tokens and
    bit-identical logits as the full pass; a batch takes its shared prefix from the same cache."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=1024, max_batch=4)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    n_img = int((g["ids_a"] == cfg.image_token_id).sum())
    rng = np.random.default_rng(3)

    def prompt(seed, n_text=330, tail=(5, 6, 7)):
        text = np.random.default_rng(seed).integers(0, 200, n_text).tolist()
        return text + [cfg.vision_start_id] + [cfg.image_token_id] * n_img + [cfg.vision_end_id] + list(tail)

    pa, pb = prompt(1), prompt(2)
    assert eng.text_prefix_len(pa) == 320 and eng.text_prefix_len([cfg.vision_start_id] + pa) == 0
    monkeypatch.setenv("VIS_SHARE_PREFIX", "0")
    full_a = eng.generate(pa, fa, max_new_tokens=8, ignore_eos=True)
    logits_full = eng.logits.clone()
    monkeypatch.setenv("VIS_SHARE_PREFIX", "1")
    first = eng.generate(pa, fa, max_new_tokens=8, ignore_eos=True)           # miss: prefix pass + suffix pass, kept
    assert eng.prefix_cache_hits == 0 and len(eng._prefix_cache) == 1
    again = eng.generate(pa, fa, max_new_tokens=8, ignore_eos=True)           # hit: suffix rows only
    assert eng.prefix_cache_hits == 1
    assert first == full_a and again == full_a and torch.equal(eng.logits, logits_full)
    # same text, another tail / another request in a batch: still the cached prefix
    other = eng.generate(prompt(1, tail=(9,)), fa, max_new_tokens=4, ignore_eos=True)
    assert eng.prefix_cache_hits == 2 and len(other) == 4
    out = eng.generate_batch([(pa, fa), (prompt(1, tail=(9,)), fa)], max_new_tokens=8, ignore_eos=True)
    assert eng.prefix_cache_hits == 3 and out[0][0] == full_a[0]
    # LRU bound and switch
    monkeypatch.setenv("VIS_PREFIX_CACHE", "2")
    for s in (2, 3, 4):
        eng.generate(prompt(s), fa, max_new_tokens=2, ignore_eos=True)
    assert len(eng._prefix_cache) == 2
    monkeypatch.setenv("VIS_PREFIX_CACHE", "0")
    eng._prefix_cache.clear()
    assert eng.generate(pa, fa, max_new_tokens=8, ignore_eos=True) == full_a and len(eng._prefix_cache) == 0


def test_chain_context_limit_is_crossed_mid_request(device):
    """The chained layer head runs while the context fits what the device holds resident for the head shape
    (hip.decode_chain_ctx_limit - waiting workgroups only, independent of VIS_MAX_CTX) and the four launches take over beyond:
    a request that crosses the limit in the middle of its decode loop gives the same tokens and logits as one that never
    chains and one that always does."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    w = pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)
    g = load_golden()
    ids, frames = g["ids_a"].tolist(), [torch.from_numpy(g["frame_a"]).to(device)]
    eng = Qwen2VLEngine(cfg, w, device, max_ctx=256)
    assert eng.chain_sync is not None and eng.chain_ctx_limit >= 256
    ref = eng.generate(ids, frames, max_new_tokens=14, ignore_eos=True)
    ref_logits = eng.logits.clone()
    for limit in (0, len(ids) + 1, len(ids) + 5):
        eng.chain_ctx_limit = limit
        for use_graph in (False, True):
            assert eng.generate(ids, frames, max_new_tokens=14, ignore_eos=True, use_graph=use_graph) == ref, (limit, use_graph)
            assert torch.equal(eng.logits, ref_logits)


def test_stalled_chained_launch_is_re_served_on_the_unchained_step(device, monkeypatch):
    """A chained layer-head launch whose in-grid wait gave up (another process running chained launches on the same GPU) raises
    the status word; the engine must notice it at the end of the request, serve the request again on the four-launch step -
    identical tokens - stay there for VIS_CHAIN_RETRY_AFTER clean requests and then go back to the chained launch (one
    transient stall must not cost the engine its faster step for good).  Simulated by raising the status word by hand."""
    monkeypatch.setenv("VIS_CHAIN_RETRY_AFTER", "2")
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    w = pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)
    g = load_golden()
    ids, frames = g["ids_a"].tolist(), [torch.from_numpy(g["frame_a"]).to(device)]
    ref = Qwen2VLEngine(cfg, w, device, max_ctx=256).generate(ids, frames, max_new_tokens=12, ignore_eos=True)
    eng = Qwen2VLEngine(cfg, w, device, max_ctx=256)
    assert eng.chain_sync is not None
    assert eng.generate(ids, frames, max_new_tokens=12, ignore_eos=True) == ref          # chained, graph captured
    eng.chain_sync[hip.CHAIN_STATUS_WORD] = 1                                            # "a wait timed out"
    assert eng.generate(ids, frames, max_new_tokens=12, ignore_eos=True) == ref          # noticed, re-served unchained
    assert eng.chain_sync is None
    assert eng.generate(ids, frames, max_new_tokens=12, ignore_eos=True) == ref          # stays on the four launches ...
    assert eng.chain_sync is None
    assert eng.generate(ids, frames, max_new_tokens=12, ignore_eos=True) == ref          # ... for two clean requests,
    assert eng.chain_sync is not None                                                    # then the chained launch is back
    assert eng.generate(ids, frames, max_new_tokens=12, ignore_eos=True) == ref
    assert eng.chain_sync is not None and int(eng.chain_sync[hip.CHAIN_STATUS_WORD]) == 0
    with pytest.raises(hip.ChainStalled):                                                # the low-level path reports it
        e2 = Qwen2VLEngine(cfg, w, device, max_ctx=256)
        e2.prefill(ids, frames, max_new_tokens=4)
        e2.decode(2)
        e2.chain_sync[hip.CHAIN_STATUS_WORD] = 1
        e2.generated(3)


@pytest.mark.gpu
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_folded_qkv_finalisation_changes_nothing(device, monkeypatch, weights):
    """VIS_QKV_FOLD (default 1): the batched decode step's self-attention launch finalises the qkv projection's partial slabs
    itself (vis_decode_attn_parts) instead of reading the row a skinny_finalize launch wrote.  Same arithmetic, so tokens AND the
    last step's logits must be equal bit for bit to the two-launch step, for the split and the streaming attention form."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    fb = [torch.from_numpy(g["frame_b1"]).to(device), torch.from_numpy(g["frame_b2"]).to(device)]
    base = [(g["ids_a"].tolist(), fa), (g["ids_b"].tolist(), fb), ([256, 72, 105, 33], [])]
    res = {}
    for fold in ("0", "1"):
        monkeypatch.setenv("VIS_QKV_FOLD", fold)
        eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=64, decode_weights=weights)
        assert eng.fold_qkv == (fold == "1")
        out = {}
        for B in (3, 64):
            reqs = [base[i % 3] for i in range(B)]
            toks = eng.generate_batch(reqs, max_new_tokens=8, ignore_eos=True)
            out[B] = (toks, eng.logits_b[:B].clone())
        res[fold] = out
        del eng
    for B in (3, 64):
        assert res["0"][B][0] == res["1"][B][0], f"B={B}: tokens differ"
        assert torch.equal(res["0"][B][1], res["1"][B][1]), f"B={B}: logits differ"
