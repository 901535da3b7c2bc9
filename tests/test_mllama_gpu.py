"""Row f2 end-to-end parity on MI355X: the mllama HIP engine (bf16 kernels through the C ABI) vs the fp32 oracle
and vs the transformers-recorded golden vectors, tiny kernel-compatible config.

Stated tolerance: cross-attention states within 6e-2 absolute (values are O(1); bf16 activations through the
6-layer tiny tower), logits within 8e-2 absolute (logit scale ~3) at EVERY one of the 12 generated steps with the
oracle's tokens teacher-forced (helpers.teacher_forced_parity), greedy picks equal to the oracle's unless its top-2
margin at that step is below 2x the tolerance; free-running tokens equal up to the first such near-tie."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LOGIT_TOL = 8e-2
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def setup(device):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from test_oracle_mllama import ref_cfg
    cfg = MllamaConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = MllamaEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256)
    return cfg, ref_cfg(cfg), sd, eng, np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))


def test_preprocess_tiles_match_oracle(setup, device):
    """GPU bilinear resample + tile patchify == oracle preprocessing (PIL + numpy), patch by patch."""
    from oracle import mllama_ref as R
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.image_processing import CLIP_MEAN, CLIP_STD
    cfg, rc, sd, eng, g = setup
    for case in "abc":
        img = g[f"{case}_image"]
        tiles, n, (th, tw), ar = R.preprocess_u8(img, rc.image_size, rc.max_tiles)
        frame, gth, gtw, gar = eng.prepare_image(torch.from_numpy(img).to(device))
        assert (gth, gtw, gar) == (th, tw, ar)
        P = cfg.tile_tokens
        out = torch.zeros((cfg.max_tiles * P, 640), dtype=torch.bfloat16, device=device)
        hip.patchify_tiles(frame, out, th, tw, cfg.image_size, CLIP_MEAN, CLIP_STD)
        got = out.float().cpu().numpy()
        G = cfg.image_size // cfg.patch
        ref = tiles.reshape(cfg.max_tiles, 3, G, 14, G, 14).transpose(0, 2, 4, 1, 3, 5).reshape(cfg.max_tiles, G * G, 588)
        for t in range(cfg.max_tiles):
            rows = got[t * P + 1:(t + 1) * P, :588]
            if t < n:
                assert np.abs(rows - ref[t]).max() < 2e-2          # bf16 rounding of O(2) values
            else:
                assert not rows.any()
            assert not got[t * P].any() and not got[:, 588:].any()


def _check_tokens(toks, ref_toks, ref_logits):
    for i, (a, b) in enumerate(zip(toks, ref_toks)):
        if a != b:
            top2 = torch.topk(ref_logits[i], 2).values
            margin = float(top2[0] - top2[1])
            assert margin < 2 * LOGIT_TOL, f"token {i}: got {a}, oracle {b}, oracle margin {margin:.4f} is not a near-tie"
            return i
    return len(ref_toks)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_engine_matches_oracle_and_golden(setup, device, case):
    from oracle import mllama_ref as R
    cfg, rc, sd, eng, g = setup
    ids = g[f"{case}_ids"].tolist()
    frame = torch.from_numpy(g[f"{case}_image"]).to(device)
    taps = {}
    eng.prefill(ids, frame, taps=taps)
    eng.decode(11, use_graph=False)
    toks = eng.generated(12)
    cross = taps["cross_states"].float().cpu().numpy()
    logits = taps["first_logits"].float().cpu().numpy()
    assert np.abs(cross - g[f"{case}_cross_states"]).max() < 6e-2
    assert np.abs(logits - g[f"{case}_logits"][0]).max() < LOGIT_TOL
    rtaps = {}
    ref_toks, ref_logits = R.generate(rc, sd, ids, g[f"{case}_image"], 12, taps=rtaps)
    assert np.abs(logits - ref_logits[0].numpy()).max() < LOGIT_TOL
    for li in range(cfg.layers):                       # per-layer hidden states of the prompt
        a = taps[f"layer{li}"].float().cpu().numpy()
        b = rtaps[f"layer{li}"].numpy()
        assert np.abs(a - b).max() < 0.15, f"layer {li}: {np.abs(a - b).max()}"
    _check_tokens(toks, ref_toks, ref_logits)
    from helpers import teacher_forced_parity
    eng.prefill(ids, frame, taps=taps)
    ties = teacher_forced_parity(eng, taps["first_logits"], ref_toks, ref_logits, LOGIT_TOL)
    assert ties <= 2


def test_graph_replay_equals_eager_and_text_only(setup, device):
    cfg, rc, sd, eng, g = setup
    from oracle import mllama_ref as R
    ids = g["a_ids"].tolist()
    frame = torch.from_numpy(g["a_image"]).to(device)
    eager = eng.generate(ids, frame, max_new_tokens=10, stop_on_eos=False, use_graph=False)
    graph = eng.generate(ids, frame, max_new_tokens=10, stop_on_eos=False, use_graph=True)
    assert eager == graph and len(graph) == 10
    # text-only prompt: cross-attention layers are skipped entirely
    tids = [1, 5, 6, 40, 41, 42, 7, 8]
    toks = eng.generate(tids, None, max_new_tokens=8, stop_on_eos=False, use_graph=True)
    ref_toks, ref_logits = R.generate(rc, sd, tids, None, 8)
    assert _check_tokens(toks, ref_toks, ref_logits) >= 4
    with pytest.raises(ValueError):
        eng.prefill(ids, None)                        # image token without a frame


def test_chained_self_layers_equal_separate_launches(setup, device, monkeypatch):
    """The Auditor's single-sequence decode with the head of every SELF-attention layer as one chained launch + the lm_head with
    the pick in its epilogue (vis_decode_chain, vis_gemv_bf16_argmax) against the separate launches
    (VIS_DECODE_CHAIN=0): tokens and last-step logits bit for bit, eager and from the graph; and a context limit that is crossed
    in the middle of a request - the engine switches to the separate launches there - changes nothing."""
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    cfg, rc, sd, eng, g = setup
    assert eng.chain_sync is not None and eng.chain_ctx_limit > 0, "the chained layer head must be the default for the Auditor"
    monkeypatch.setenv("VIS_DECODE_CHAIN", "0")
    plain = MllamaEngine(cfg, eng.w, device, max_ctx=256)
    assert plain.chain_sync is None
    for case in "ab":
        ids = g[f"{case}_ids"].tolist()
        frame = torch.from_numpy(g[f"{case}_image"]).to(device)
        ref = plain.generate(ids, frame, max_new_tokens=14, stop_on_eos=False, use_graph=False)
        ref_logits = plain.logits.clone()
        before = int(eng.chain_sync[0])
        for use_graph in (False, True):
            assert eng.generate(ids, frame, max_new_tokens=14, stop_on_eos=False, use_graph=use_graph) == ref
            assert torch.equal(eng.logits, ref_logits)
            assert int(eng.chain_sync[hip.CHAIN_STATUS_WORD]) == 0
        assert int(eng.chain_sync[0]) > before, "no chained launch ran"
        saved = eng.chain_ctx_limit
        eng.chain_ctx_limit = len(ids) + 6            # steps 1..6 chained, 7..13 on the separate launches
        try:
            assert eng.generate(ids, frame, max_new_tokens=14, stop_on_eos=False, use_graph=True) == ref
            assert torch.equal(eng.logits, ref_logits)
        finally:
            eng.chain_ctx_limit = saved
    # text-only prompts skip the cross layers; the chained self layers serve them as well
    tids = [1, 5, 6, 40, 41, 42, 7, 8]
    assert eng.generate(tids, None, max_new_tokens=8, stop_on_eos=False) == plain.generate(tids, None, max_new_tokens=8, stop_on_eos=False)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_batched_decode_matches_single_and_is_batch_invariant(device, monkeypatch, fused):
    """verify_many path: several images share ONE decode loop (stream-K batched projections, batched
    self- and cross-attention).  A request's tokens do not depend on its slot, on the batch size or on what shares the
    batch (exact); graph replay == eager; against the single-sequence GEMV path the first token (same prompt pass) is
    exact and the rest agree up to genuine near-ties of the oracle (different f32 summation order)."""
    monkeypatch.setenv("VIS_DECODE_FUSED", fused)      # 1: the opt-in r05 step (every projection one launch)
    from oracle import mllama_ref as R
    from test_oracle_mllama import ref_cfg
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    cfg = MllamaConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = MllamaEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=5)
    g = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    reqs = [(g[f"{c}_ids"].tolist(), torch.from_numpy(g[f"{c}_image"]).to(device)) for c in "abc"]
    singles = [eng.generate(ids, fr, max_new_tokens=10, stop_on_eos=False) for ids, fr in reqs]
    eager = eng.generate_batch(reqs + [reqs[0], reqs[2]], max_new_tokens=10, stop_on_eos=False, use_graph=False)
    graph = eng.generate_batch(reqs + [reqs[0], reqs[2]], max_new_tokens=10, stop_on_eos=False, use_graph=True)
    assert eager == graph and [len(t) for t in graph] == [10] * 5
    assert graph[0] == graph[3] and graph[2] == graph[4]                     # same request, different slots
    other = eng.generate_batch([reqs[2], reqs[0]], max_new_tokens=10, stop_on_eos=False)
    assert other == [graph[2], graph[0]]                                     # other batch size / order / neighbours
    for b, (ids, fr) in enumerate(reqs):
        assert graph[b][0] == singles[b][0]
        ref_toks, ref_logits = R.generate(ref_cfg(cfg), sd, ids, fr.cpu().numpy(), 10)
        _check_tokens(graph[b], ref_toks, ref_logits)
        _check_tokens(singles[b], ref_toks, ref_logits)
    # a text-only request cannot join a batch (the batched step always runs the cross layers)
    with pytest.raises(ValueError):
        eng.generate_batch([reqs[0], ([1, 5, 6, 7], None)], max_new_tokens=4)


def test_stacked_prompt_passes_equal_one_pass_per_request(device, monkeypatch):
    """verify_many sends the same Auditor prompt with every image: the requests of a group run the tower once over their
    stacked images and the text decoder once over their stacked rows (MllamaEngine.vision_forward_many / _prefill_group).
    Tokens and first-step logits must be exactly those of one pass per request - also against the single-sequence path's
    first token - for images of different tile counts."""
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    cfg = MllamaConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    eng = MllamaEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=6)
    g = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    ids = g["b_ids"].tolist()                                            # text first, image token last (the reference's order)
    frames = [torch.from_numpy(g[f"{c}_image"]).to(device) for c in "abc"]           # 2, 4 and 1 tiles
    reqs = [(ids, frames[0]), (ids, frames[1]), (ids, frames[2]), (ids, frames[0]), (ids, frames[1])]
    calls = []
    real = eng._prefill_group
    monkeypatch.setattr(eng, "_prefill_group", lambda items, *a, **k: (calls.append(len(items)), real(items, *a, **k))[1])
    stacked = eng.generate_batch(reqs, max_new_tokens=10, stop_on_eos=False)
    logits = eng.logits_b[:5].clone()
    assert calls == [4, 1]                                               # groups of four: [4 stacked] + [1 alone, a group of one]
    monkeypatch.setenv("VIS_MERGE_PREFILL", "0")
    monkeypatch.setenv("VIS_VIT_BATCH", "1")
    apart = eng.generate_batch(reqs, max_new_tokens=10, stop_on_eos=False)
    assert calls == [4, 1] + [1] * 5 and apart == stacked and torch.equal(logits, eng.logits_b[:5])      # no stack now
    assert stacked[0] == stacked[3] and stacked[1] == stacked[4]
    for b in range(3):
        assert eng.generate(ids, frames[b], max_new_tokens=10, stop_on_eos=False)[0] == stacked[b][0]


def test_max_batch_one_engine_serves_callable_requests(device):
    """with VIS_MAX_BATCH = 1 the batched buffers do not exist, yet the batch seam still hands every verify_many
    group over as callables (Futures).  A one-request lazy batch must take the single-sequence path - same tokens as
    generate() - and a callable that raises must come back as that exception in its slot, not as an AttributeError."""
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=1)
    assert not hasattr(eng, "b_x")                       # no batched-decode buffers at max_batch == 1
    g = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    ids, fr = g["a_ids"].tolist(), torch.from_numpy(g["a_image"]).to(device)
    direct = eng.generate(ids, fr, max_new_tokens=8, stop_on_eos=False)
    assert eng.generate_batch([lambda: (ids, fr)], max_new_tokens=8, stop_on_eos=False) == [direct]
    assert eng.generate_batch([(ids, fr)], max_new_tokens=8, stop_on_eos=False) == [direct]

    def broken():
        raise OSError("image file is truncated")
    out = eng.generate_batch([broken], max_new_tokens=8, stop_on_eos=False)
    assert len(out) == 1 and isinstance(out[0], OSError)
    with pytest.raises(ValueError):
        eng.generate_batch([(ids, fr), (ids, fr)], max_new_tokens=4)      # two requests do not fit max_batch = 1


def test_mllama_folded_qkv_finalisation_changes_nothing(device, monkeypatch):
    """VIS_QKV_FOLD on the Auditor: in the batched step its self-attention layers read the qkv projection's partial slabs directly
    (vis_decode_attn_parts: no bias, the rope table shared by the batch = stride 0).  Tokens and last-step logits equal to the
    two-launch step bit for bit."""
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    cfg = MllamaConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    g = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    reqs = [(g[f"{c}_ids"].tolist(), torch.from_numpy(g[f"{c}_image"]).to(device)) for c in "abc"]
    res = {}
    for fold in ("0", "1"):
        monkeypatch.setenv("VIS_QKV_FOLD", fold)
        eng = MllamaEngine(cfg, pack_device_weights(cfg, sd, device), device, max_ctx=256, max_batch=5)
        assert eng.fold_qkv == (fold == "1")
        toks = eng.generate_batch(reqs + [reqs[0], reqs[2]], max_new_tokens=10, stop_on_eos=False)
        res[fold] = (toks, eng.logits_b[:5].clone())
        del eng
    assert res["0"][0] == res["1"][0]
    assert torch.equal(res["0"][1], res["1"][1])
