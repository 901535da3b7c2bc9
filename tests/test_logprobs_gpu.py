"""Token log-probabilities on MI355X: the vis_logprobs_f32 kernel against a float64 reference at the real vocabulary sizes,
and the engines' / client's logprobs against the logits they pick from.

Tolerances: the kernel's values within 1e-4 absolute of float64 log_softmax (f32 sums over up to 152064 entries), ids
exact with ties in index order; engine values within 1e-4 of log_softmax of the engine's own logits at every step and within
2 x the logit tolerance of the parity tests against the recorded / oracle logits (log_softmax shifts every logit by the same
lse, whose error is at most the largest logit error)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import load_golden, oracle_inputs, ref_config

pytestmark = pytest.mark.gpu
LOGIT_TOL = 6e-2
MLLAMA_LOGIT_TOL = 8e-2
HERE = os.path.dirname(os.path.abspath(__file__))
K = 20


def _ref(x: torch.Tensor, k: int):
    """float64 log_softmax and the top-k ids of f32 rows, ties to the lower index."""
    lsm = torch.log_softmax(x.double(), dim=-1)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
    return lsm, order


def _rows(V: int, B: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((B, V), generator=g, device="cuda") * 4.0
    for r in range(0, B, 3):           # planted exact ties: at the top and just below it
        idx = torch.randperm(V, generator=g, device="cuda")[:6]
        top = x[r].max()
        x[r, idx[:3]] = top + 1.0
        x[r, idx[3:]] = top + 0.5
    if B > 1:
        x[1, :] = 0.25                  # a constant row: every entry ties
    return x


def _run(x, tokens, step, k, lp, ids):
    from vision_inspection_system_amd import hip
    ws = hip.logprobs_ws(x.shape[1], x.shape[0], x.device)
    hip.logprobs(x, tokens, step, k, lp, ids, ws)


@pytest.mark.parametrize("V", [152064, 128256, 512, 513])
def test_kernel_against_float64_reference(device, V):
    from vision_inspection_system_amd import hip
    T = 8
    x = _rows(V, 64, seed=V)
    lsm, order = _ref(x, K)
    for B in (1, 3, 64):
        for k in (0, 1, 20):
            xb = x[:B].contiguous()
            # the pick first (greedy): tokens[b][pos] = argmax, step[b] = pos + 1; the last row of a batch sits at
            # pos = T (past max_tokens): the pick stores nothing there and neither may the logprobs kernel
            pos = torch.tensor([b % T for b in range(B)], dtype=torch.int32, device=device)
            if B > 1:
                pos[-1] = T
            step = pos.clone()
            tokens = torch.full((B, T), -1, dtype=torch.int32, device=device)
            cur = torch.zeros(B, dtype=torch.int32, device=device)
            wv = torch.empty(256 * B, dtype=torch.float32, device=device)
            wi = torch.empty(256 * B, dtype=torch.int32, device=device)
            hip.argmax(xb, wv, wi, tokens, cur, step)
            lp = torch.full((B, T, K + 1), 7.0, dtype=torch.float32, device=device)
            ids = torch.full((B, T, K), -7, dtype=torch.int32, device=device)
            _run(xb, tokens, step, k, lp, ids)
            lp_c, ids_c, tok_c, pos_c = lp.cpu(), ids.cpu(), tokens.cpu(), pos.cpu()
            for b in range(B):
                p = int(pos_c[b])
                if p >= T:
                    assert (lp_c[b] == 7.0).all() and (ids_c[b] == -7).all(), "wrote past max_tokens"
                    continue
                others = [q for q in range(T) if q != p]
                assert (lp_c[b, others] == 7.0).all() and (ids_c[b, others] == -7).all()
                t = int(tok_c[b, p])
                ref = lsm[b].cpu()
                assert abs(float(lp_c[b, p, 0]) - float(ref[t])) < 1e-4, (V, B, k, b)
                assert (lp_c[b, p, 1 + k:] == 7.0).all() and (ids_c[b, p, k:] == -7).all()
                if k:
                    want = order[b, :k].cpu()
                    assert torch.equal(ids_c[b, p, :k].long(), want), (V, B, k, b, ids_c[b, p, :k], want)
                    assert (lp_c[b, p, 1:1 + k].double() - ref[want]).abs().max() < 1e-4
                    # greedy: the top id is the argmax kernel's pick, and its value is the chosen token's, bit for bit
                    assert int(ids_c[b, p, 0]) == t
                    assert lp_c[b, p, 1].view(torch.int32) == lp_c[b, p, 0].view(torch.int32)


@pytest.mark.parametrize("V", [152064, 513])
def test_kernel_row_results_do_not_depend_on_the_batch(device, V):
    T = 4
    x = _rows(V, 64, seed=7)
    step = torch.full((64,), 2, dtype=torch.int32, device=device)
    tokens = torch.randint(0, V, (64, T), dtype=torch.int32, device=device)
    lp = torch.zeros((64, T, K + 1), dtype=torch.float32, device=device)
    ids = torch.zeros((64, T, K), dtype=torch.int32, device=device)
    _run(x, tokens, step, K, lp, ids)
    for r in (0, 1, 17, 63):
        lp1 = torch.zeros((1, T, K + 1), dtype=torch.float32, device=device)
        ids1 = torch.zeros((1, T, K), dtype=torch.int32, device=device)
        _run(x[r:r + 1], tokens[r:r + 1], step[r:r + 1], K, lp1, ids1)
        assert torch.equal(lp1[0, 1].view(torch.int32), lp[r, 1].view(torch.int32)), r
        assert torch.equal(ids1[0, 1], ids[r, 1]), r


# ----------------------------------------------------------------------------- engines
def _lsm(logits: torch.Tensor) -> torch.Tensor:
    return torch.log_softmax(logits.double().cpu().view(-1), dim=-1)


def _check_own(eng, slot: int, pos: int, k: int, logits: torch.Tensor, tol: float = 1e-4):
    """Record at (slot, pos) against log_softmax of the logits the pick read."""
    ref = _lsm(logits)
    lp = eng._lp.lp[slot, pos].double().cpu()
    ids = eng._lp.top_ids[slot, pos, :k].long().cpu()
    tok = int(eng.tokens_b[slot, pos])
    assert abs(float(lp[0]) - float(ref[tok])) < tol
    assert torch.equal(ids, torch.sort(logits.float().cpu().view(-1), descending=True, stable=True).indices[:k])
    assert (lp[1:1 + k] - ref[ids]).abs().max() < tol
    return lp, ref


def _step_by_step(eng, prefill, n_steps: int, k: int = K):
    """Prefill + eager single steps with logprobs on; every step's record against the engine's own logits."""
    eng._begin_logprobs(k)
    try:
        prefill()
        S = eng.prompt_len
        first = eng.logits.clone()
        out = [_check_own(eng, 0, S - 1, k, first)[0]]
        for t in range(1, n_steps):
            eng.decode(1, use_graph=False)
            out.append(_check_own(eng, 0, S - 1 + t, k, eng.logits)[0])
        return first, out, eng.tokens[S - 1:S - 1 + n_steps].cpu().tolist()
    finally:
        eng.lp_k = None


@pytest.fixture(scope="module")
def qwen(device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    sd = synth_state_dict(cfg, seed=0)
    w = pack_device_weights(cfg, sd, device)
    return cfg, sd, w, Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_splits=4)


def test_qwen_logprobs_against_golden_oracle_and_own_logits(qwen, device):
    from oracle import qwen2vl_ref as R
    cfg, sd, w, eng = qwen
    g = load_golden()
    ids, fr = g["ids_a"].tolist(), [g["frame_a"]]
    dev_fr = [torch.from_numpy(f).to(device) for f in fr]
    n = 8
    first, lps, toks = _step_by_step(eng, lambda: eng.prefill(ids, dev_fr), n)
    gold = torch.log_softmax(torch.from_numpy(g["a_first_logits"]).double().view(-1), dim=-1)
    t0 = toks[0]
    assert abs(float(lps[0][0]) - float(gold[t0])) < 2 * LOGIT_TOL
    top = torch.sort(first.float().cpu(), descending=True, stable=True).indices[:K]
    assert (lps[0][1:].double() - gold[top]).abs().max() < 2 * LOGIT_TOL
    # free-running greedy steps against the oracle's logits, up to the oracle's first near-tie
    pv, grids = oracle_inputs(fr)
    ref_toks, ref_logits = R.generate(ref_config(cfg), sd, ids, pv, grids, n)
    for t in range(n):
        rl = ref_logits[t].double().view(-1)
        top2 = torch.topk(rl, 2).values
        if float(top2[0] - top2[1]) < 2 * LOGIT_TOL or toks[t] != ref_toks[t]:
            break
        ref = torch.log_softmax(rl, dim=-1)
        assert abs(float(lps[t][0]) - float(ref[toks[t]])) < 2 * LOGIT_TOL, t


def test_qwen_paths_agree(qwen, device, monkeypatch):
    """Tokens do not change with logprobs on; logprobs are the same bits eager vs graph and chained vs unchained; the values
    do not depend on the temperature (same prompt -> same first-position record)."""
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg, sd, w, eng = qwen
    g = load_golden()
    ids = g["ids_a"].tolist()
    fr = [torch.from_numpy(g["frame_a"]).to(device)]
    for temp, seed in ((0.0, 0), (0.8, 3)):
        off = eng.generate(ids, fr, max_new_tokens=10, ignore_eos=True, temperature=temp, seed=seed)
        assert eng.last_logprobs is None
        recs = {}
        for k in (0, K):
            for use_graph in (False, True):
                toks = eng.generate(ids, fr, max_new_tokens=10, ignore_eos=True, temperature=temp, seed=seed,
                                    use_graph=use_graph, logprobs=k)
                assert toks == off
                (rec,) = eng.last_logprobs
                assert rec.token_logprobs.shape == (10,) and rec.top_ids.shape == (10, k) == rec.top_logprobs.shape
                recs[(k, use_graph)] = rec
        for key, rec in recs.items():
            assert np.array_equal(rec.token_logprobs, recs[(K, True)].token_logprobs), key
        assert np.array_equal(recs[(K, False)].top_ids, recs[(K, True)].top_ids)
        assert np.array_equal(recs[(K, False)].top_logprobs, recs[(K, True)].top_logprobs)
        if temp == 0.0:
            greedy = recs[(K, True)]
            assert (greedy.top_ids[:, 0] == np.array(off)).all()
            assert np.array_equal(greedy.top_logprobs[:, 0], greedy.token_logprobs)
        else:
            assert np.array_equal(recs[(K, True)].top_logprobs[0], greedy.top_logprobs[0])   # raw logits: no temperature
    assert eng.chain_sync is not None
    monkeypatch.setenv("VIS_DECODE_CHAIN", "0")
    plain = Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_splits=4)
    assert plain.chain_sync is None
    ref = eng.generate(ids, fr, max_new_tokens=10, ignore_eos=True, logprobs=K)
    b = eng.last_logprobs[0]
    assert plain.generate(ids, fr, max_new_tokens=10, ignore_eos=True, logprobs=K) == ref
    a = plain.last_logprobs[0]
    assert np.array_equal(a.token_logprobs, b.token_logprobs) and np.array_equal(a.top_ids, b.top_ids)
    assert np.array_equal(a.top_logprobs, b.top_logprobs)
    # EOS cut: the record is cut like the tokens
    import dataclasses
    eng.cfg = dataclasses.replace(cfg, eos_ids=(ref[3],))
    try:
        cut = eng.generate(ids, fr, max_new_tokens=10, check_every=2, logprobs=2)
        assert cut == ref[:3] and eng.last_logprobs[0].token_logprobs.shape == (3,)
    finally:
        eng.cfg = cfg


@pytest.mark.parametrize("form,weights", [("plain", "bf16"), ("plain", "fp8"), ("fused", "bf16"), ("rows", "bf16")])
def test_qwen_batched_forms(device, monkeypatch, form, weights):
    """Every batched decode form with logprobs: tokens unchanged, one record per request with n == len(tokens), the last
    step's records against the batch's own logits, the first position (prompt pass) equal to the single-sequence record;
    VIS_ROWS_GEMV's rows are the single-sequence arithmetic, so there every record equals the single one."""
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    monkeypatch.setenv("VIS_DECODE_FUSED", "1" if form == "fused" else "0")
    monkeypatch.setenv("VIS_ROWS_GEMV", "2" if form == "rows" else "0")
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256,
                        max_batch=4, decode_weights=weights)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fa), ([256, 72, 105, 33, 90, 41], [])]
    if form != "rows":
        reqs.append((g["ids_a"].tolist(), fa))
    n = 10
    off = eng.generate_batch(reqs, max_new_tokens=n, ignore_eos=True)
    for use_graph in (False, True):
        on = eng.generate_batch(reqs, max_new_tokens=n, ignore_eos=True, use_graph=use_graph, logprobs=5)
        assert on == off
        recs = eng.last_logprobs
        assert len(recs) == len(reqs) and all(r.token_logprobs.shape == (len(t),) for r, t in zip(recs, on))
        for b in range(len(reqs)):
            start = eng.slot_prompt_len[b] - 1
            _check_own(eng, b, start + n - 1, 5, eng.logits_b[b])
    singles = []
    for ids, fr in reqs:
        assert eng.generate(ids, fr, max_new_tokens=n, ignore_eos=True, logprobs=5) is not None
        singles.append(eng.last_logprobs[0])
    for r, s in zip(recs, singles):
        assert r.token_logprobs[0] == s.token_logprobs[0] and np.array_equal(r.top_logprobs[0], s.top_logprobs[0])
        if form == "rows":
            assert np.array_equal(r.token_logprobs, s.token_logprobs) and np.array_equal(r.top_ids, s.top_ids)


def test_qwen_fp8_single_sequence_against_own_logits(qwen, device):
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg, sd, w, _ = qwen
    eng = Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_splits=4, decode_weights="fp8")
    g = load_golden()
    ids = g["ids_a"].tolist()
    fr = [torch.from_numpy(g["frame_a"]).to(device)]
    _, _, toks = _step_by_step(eng, lambda: eng.prefill(ids, fr), 6)
    off = eng.generate(ids, fr, max_new_tokens=6, ignore_eos=True)
    assert eng.generate(ids, fr, max_new_tokens=6, ignore_eos=True, logprobs=3) == off == toks


@pytest.fixture(scope="module")
def mllama(device):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    cfg = MllamaConfig.tiny()
    w = pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)
    return cfg, w, MllamaEngine(cfg, w, device, max_ctx=256, max_batch=3), np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))


def test_mllama_logprobs(mllama, device):
    cfg, w, eng, g = mllama
    ids = g["a_ids"].tolist()
    frame = torch.from_numpy(g["a_image"]).to(device)
    first, lps, toks = _step_by_step(eng, lambda: eng.prefill(ids, frame), 6)
    gold = torch.log_softmax(torch.from_numpy(g["a_logits"][0]).double().view(-1), dim=-1)
    assert abs(float(lps[0][0]) - float(gold[toks[0]])) < 2 * MLLAMA_LOGIT_TOL
    off = eng.generate(ids, frame, max_new_tokens=8, stop_on_eos=False)
    recs = {}
    for use_graph in (False, True):
        assert eng.generate(ids, frame, max_new_tokens=8, stop_on_eos=False, use_graph=use_graph, logprobs=K) == off
        recs[use_graph] = eng.last_logprobs[0]
    assert np.array_equal(recs[False].token_logprobs, recs[True].token_logprobs)
    assert np.array_equal(recs[False].top_ids, recs[True].top_ids) and recs[True].token_logprobs.shape == (8,)
    assert (recs[True].top_ids[:, 0] == np.array(off)).all()
    # batched: tokens unchanged, a record per request, the last step against the batch's own logits
    reqs = [(g["a_ids"].tolist(), frame), (g["b_ids"].tolist(), torch.from_numpy(g["b_image"]).to(device)),
            (g["a_ids"].tolist(), frame)]
    boff = eng.generate_batch(reqs, max_new_tokens=6, stop_on_eos=False)
    bon = eng.generate_batch(reqs, max_new_tokens=6, stop_on_eos=False, logprobs=4)
    assert bon == boff and [r.token_logprobs.shape[0] for r in eng.last_logprobs] == [len(t) for t in bon]
    for b in range(3):
        _check_own(eng, b, eng.slot_prompt_len[b] - 1 + 5, 4, eng.logits_b[b])
    assert eng.last_logprobs[0].token_logprobs[0] == recs[True].token_logprobs[0]


# ----------------------------------------------------------------------------- client
@pytest.fixture
def image_url(tmp_path):
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    p = tmp_path / "img.png"
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    return encode_image_optimized(str(p), 256)


@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_logprobs(device, image_url, model):
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": [{"type": "text", "text": "Inspect."},
                                         {"type": "image_url", "image_url": {"url": image_url}}]}]
    plain = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=12)
    assert plain.choices[0].logprobs is None
    r = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=12, logprobs=True, top_logprobs=5)
    ch = r.choices[0]
    assert ch.message.content == plain.choices[0].message.content
    content = ch.logprobs.content
    assert len(content) == r.usage["completion_tokens"]
    for e in content:
        assert len(e.top_logprobs) == 5 and e.logprob <= 0
        assert sum(np.exp(t.logprob) for t in e.top_logprobs) <= 1 + 1e-5
        assert e.logprob == e.top_logprobs[0].logprob
    assert bytes(b for e in content for b in e.bytes).decode("utf-8", errors="replace") == ch.message.content
    r0 = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=12, logprobs=True)
    assert all(e.top_logprobs == [] for e in r0.choices[0].logprobs.content)
    assert [e.logprob for e in r0.choices[0].logprobs.content] == [e.logprob for e in content]
    # three requests in one call: per-request logprobs as in single calls (same prompt pass; the first token's record is
    # the prompt pass's, the later ones may come from the batched step's different summation order)
    many = c.complete_many(model, [msgs, msgs, [{"role": "user", "content": "OK?"}]], temperature=0.0, max_tokens=12,
                           logprobs=True, top_logprobs=5)
    for m in many[:2]:
        mc = m.choices[0].logprobs.content
        assert len(mc) == m.usage["completion_tokens"]
        assert mc[0].logprob == content[0].logprob and mc[0].token == content[0].token
        assert [t.logprob for t in mc[0].top_logprobs] == [t.logprob for t in content[0].top_logprobs]
    single3 = c.chat.completions.create(model=model, messages=[{"role": "user", "content": "OK?"}], temperature=0.0,
                                        max_tokens=12, logprobs=True, top_logprobs=5)
    m3 = many[2].choices[0].logprobs.content
    assert len(m3) == many[2].usage["completion_tokens"] and m3[0].logprob == single3.choices[0].logprobs.content[0].logprob
