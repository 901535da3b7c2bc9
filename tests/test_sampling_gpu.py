"""Nucleus sampling and per-request seeds on MI355X: vis_sample_f32 against the float64 reference (sampling.nucleus_ref),
its agreement with vis_argmax_f32 at top_p = 1, the sampled distribution, batch invariance, masks and graph replay; then
the engines' and the client's top_p / seed(s) keywords."""
import os

import numpy as np
import pytest
import torch

from helpers import load_golden
from vision_inspection_system_amd import hip
from vision_inspection_system_amd.sampling import SLOT_SEED_STRIDE, nucleus_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


def _masks(V: int, B: int, kind: str, seed: int) -> torch.Tensor:
    """int64 allow rows [B, ceil(V / 64)]: every id ("ones") or a random 10 %."""
    nw = (V + 63) // 64
    if kind == "ones":
        bits = np.zeros((B, nw * 64), dtype=bool)
        bits[:, :V] = True
    else:
        bits = np.random.default_rng(seed).random((B, nw * 64)) < 0.1
        bits[:, V:] = False
    return torch.from_numpy(np.packbits(bits.reshape(B, -1, 8), axis=2, bitorder="little").reshape(B, -1)
                            .view("<u8").view(np.int64).copy()).cuda()


def _allowed_bits(m: torch.Tensor, V: int) -> np.ndarray:
    a = m.cpu().numpy().view(np.uint8)
    return np.unpackbits(a.reshape(a.shape[0], -1), axis=1, bitorder="little")[:, :V].astype(bool)


def _seeds(vals):
    return torch.from_numpy(np.array([v & 0xFFFFFFFF for v in vals], dtype=np.uint32).view(np.int32)).cuda()


def _sample(x, T, p, seeds, allow=None, step=None, T_tok=8):
    """One vis_sample_f32 launch over the rows of x [B, V]; returns (picks, nkeep, tokens, step after)."""
    B, V = x.shape
    tokens = torch.full((B, T_tok), -1, dtype=torch.int32, device="cuda")
    st = (torch.arange(B, dtype=torch.int32, device="cuda") % 5) if step is None else step.clone()
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    nkeep = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ws = hip.sample_ws(V, B, "cuda")
    hip.sample(x, tokens if B > 1 else tokens[0], cur, st, _seeds(seeds), ws, T, p, allow=allow, nkeep=nkeep)
    return cur.cpu().numpy(), nkeep.cpu().numpy(), tokens.cpu(), st.cpu()


def _argmax(x, T, seed, step, allow=None):
    B, V = x.shape
    tokens = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = step.clone()
    wv = torch.empty(256 * B, dtype=torch.float32, device="cuda")
    wi = torch.empty(256 * B, dtype=torch.int32, device="cuda")
    if allow is None:
        hip.argmax(x, wv, wi, tokens if B > 1 else tokens[0], cur, st, T, seed)
    else:
        hip.argmax_masked(x, wv, wi, tokens if B > 1 else tokens[0], cur, st, allow, T, seed)
    return cur.cpu().numpy()


def _rows(V, seed):
    """Rows with planted structure: plain, a tie at the top, a constant row, a big tie group near the top, a peaked row,
    logits on a 0.1 grid (ties everywhere)."""
    rng = np.random.default_rng(seed)
    r0 = rng.normal(0, 3, V)
    r1 = rng.normal(0, 3, V)
    r1[rng.choice(V, 5, replace=False)] = r1.max() + 1.0
    r2 = np.zeros(V)
    r3 = rng.normal(0, 1, V)
    r3[rng.choice(V, 3000, replace=False)] = 3.0
    r3[7] = 4.0
    r4 = rng.normal(0, 8, V)
    r5 = np.round(rng.normal(0, 2, V), 1)
    return np.stack([r0, r1, r2, r3, r4, r5]).astype(np.float32)


def _check_nkeep(got, ref, p, what):
    # a loose check (+-1 near the boundary); the exact ones - the cut record (v*, i*), nkeep inside the interval the kernel's
    # fixed-point weights allow, the pick over exactly that prefix - are tests/test_pick_exact_gpu.py::test_sample
    if got == ref.nkeep:
        return
    # the kernel sums in fixed point: a boundary within 1e-5 Z of p Z may land on the neighbouring count
    near = [n for n in (ref.nkeep - 1, ref.nkeep + 1) if 1 <= n <= ref.order.size]
    ok = [n for n in near if abs(ref.cum[min(n, ref.nkeep) - 1] - p) < 1e-5]
    assert got in ok, (what, got, ref.nkeep)


@pytest.mark.parametrize("V", [152064, 128256])
def test_kernel_matches_reference(V):
    x = _rows(V, V)
    xd = torch.from_numpy(x).cuda()
    for T in (0.1, 0.7, 1.0, 2.0):
        for p in (0.0, 0.1, 0.5, 0.9, 0.999, 1.0):
            picks, nk, tokens, st = _sample(xd, T, p, [11 + r for r in range(x.shape[0])])
            for r in range(x.shape[0]):
                ref = nucleus_ref(x[r], T, p)
                _check_nkeep(int(nk[r]), ref, p, (V, T, p, r))
                assert ref.keep[picks[r]], (V, T, p, r)
                assert tokens[r, r % 5] == picks[r] and st[r] == r % 5 + 1
    # 64 rows in one launch: every row checked against the reference
    rng = np.random.default_rng(1)
    x64 = (rng.normal(0, 1, (64, V)) * rng.uniform(0.5, 6, (64, 1))).astype(np.float32)
    picks, nk, _, _ = _sample(torch.from_numpy(x64).cuda(), 0.7, 0.9, list(range(64)))
    for r in range(64):
        ref = nucleus_ref(x64[r], 0.7, 0.9)
        _check_nkeep(int(nk[r]), ref, 0.9, ("B64", r))
        assert ref.keep[picks[r]]


@pytest.mark.parametrize("masked", [False, True])
def test_top_p_one_is_argmax_bit_for_bit(masked):
    V, B = 152064, 16
    g = torch.Generator(device="cuda").manual_seed(3)
    x = (torch.randn((B, V), generator=g, device="cuda") * 4).contiguous()
    allow = _masks(V, B, "random", 5) if masked else None
    step = torch.arange(B, dtype=torch.int32, device="cuda") % 5
    for T in (0.5, 1.0, 1.7):
        s = 1234
        # the old derived seeds: vis_argmax_f32 at batch B
        picks, _, _, _ = _sample(x, T, 1.0, [s + SLOT_SEED_STRIDE * r for r in range(B)], allow=allow, step=step)
        assert (picks == _argmax(x, T, s, step, allow)).all()
        # one seed for every row: vis_argmax_f32 at batch 1 with that seed, row by row
        picks, _, _, _ = _sample(x, T, 1.0, [s] * B, allow=allow, step=step)
        for r in range(0, B, 5):
            a = allow[r:r + 1] if masked else None
            assert picks[r] == _argmax(x[r:r + 1], T, s, step[r:r + 1], a)[0]


def test_zero_temperature_is_greedy():
    V, B = 128256, 8
    g = torch.Generator(device="cuda").manual_seed(4)
    x = (torch.randn((B, V), generator=g, device="cuda") * 3).contiguous()
    x[2, 100] = x[2, 200] = x[2].max() + 1        # a tie: the lower index
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    greedy = _argmax(x, 0.0, 0, step)
    assert greedy[2] == 100
    for p in (0.0, 0.3, 0.9, 1.0):
        picks, nk, _, _ = _sample(x, 0.0, p, [9] * B, step=step)
        assert (picks == greedy).all() and (nk == 1).all()


def test_distribution_chi_square():
    V, B, rounds = 40, 64, 64
    logits = np.log(np.linspace(1.0, 0.05, V)) * 1.5
    logits = np.random.default_rng(2).permutation(logits).astype(np.float32)
    T, p = 1.0, 0.8
    ref = nucleus_ref(logits, T, p)
    x = torch.from_numpy(np.tile(logits, (B, 1))).cuda()
    counts = np.zeros(V)
    for k in range(rounds):
        step = torch.arange(B, dtype=torch.int32, device="cuda") + k * B
        picks, nk, _, _ = _sample(x, T, p, [77] * B, step=step)
        assert (nk == ref.nkeep).all()
        np.add.at(counts, picks, 1)
    assert counts[~ref.keep].sum() == 0                 # no draw outside K
    w = np.exp((logits.astype(np.float64) - logits.max()) / T) * ref.keep
    expect = w / w.sum() * counts.sum()
    k = ref.keep
    chi2 = (((counts[k] - expect[k]) ** 2) / expect[k]).sum()
    dof = int(k.sum()) - 1
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)


def test_batch_invariance():
    V = 152064
    rng = np.random.default_rng(9)
    x = rng.normal(0, 2.5, (64, V)).astype(np.float32)
    x[37] = x[0]
    step = torch.zeros(64, dtype=torch.int32, device="cuda")
    step[0] = step[37] = 3
    seeds = list(range(100, 164))
    seeds[37] = seeds[0]
    for T, p in ((1.0, 0.9), (0.7, 0.5), (2.0, 0.999)):
        picks, nk, _, _ = _sample(torch.from_numpy(x).cuda(), T, p, seeds, step=step)
        assert picks[0] == picks[37] and nk[0] == nk[37]
        one, nk1, _, _ = _sample(torch.from_numpy(x[:1]).cuda(), T, p, seeds[:1], step=step[:1])
        assert one[0] == picks[0] and nk1[0] == nk[0]


def test_mask():
    V, B = 152064, 8
    g = torch.Generator(device="cuda").manual_seed(6)
    x = (torch.randn((B, V), generator=g, device="cuda") * 3).contiguous()
    allow = _masks(V, B, "random", 8)
    bits = _allowed_bits(allow, V)
    xn = x.cpu().numpy()
    for T, p in ((1.0, 0.9), (0.5, 0.5), (2.0, 0.1)):
        picks, nk, _, _ = _sample(x, T, p, list(range(B)), allow=allow)
        for r in range(B):
            assert bits[r, picks[r]]
            ref = nucleus_ref(xn[r], T, p, bits[r])
            _check_nkeep(int(nk[r]), ref, p, ("mask", T, p, r))
            assert ref.keep[picks[r]]
        ones = _masks(V, B, "ones", 0)
        a = _sample(x, T, p, list(range(B)), allow=ones)
        u = _sample(x, T, p, list(range(B)))
        assert (a[0] == u[0]).all() and (a[1] == u[1]).all()
    # an empty row stores id 0
    empty = torch.zeros_like(allow)
    picks, nk, _, _ = _sample(x, 1.0, 0.9, list(range(B)), allow=empty)
    assert (picks == 0).all() and (nk == 0).all()


def test_graph_replay_equals_eager():
    V, B = 152064, 4
    g = torch.Generator(device="cuda").manual_seed(12)
    x = (torch.randn((B, V), generator=g, device="cuda") * 2).contiguous()
    tokens = torch.zeros((B, 16), dtype=torch.int32, device="cuda")
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    seeds = _seeds([1, 2, 3, 4])
    ws = hip.sample_ws(V, B, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.sample(x, tokens, cur, step, seeds, ws, 1.0, 0.9)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.sample(x, tokens, cur, step, seeds, ws, 1.0, 0.9)
    for vals in ([1, 2, 3, 4], [9, 8, 7, 6]):
        seeds.copy_(_seeds(vals))
        step.zero_()
        for _ in range(6):
            graph.replay()
        got = tokens[:, :6].clone()
        step.zero_()
        tokens.zero_()
        for _ in range(6):
            hip.sample(x, tokens, cur, step, seeds, ws, 1.0, 0.9)
        assert torch.equal(got, tokens[:, :6]), vals


# ----------------------------------------------------------------------------- engines
def _qwen_engine(device, **kw):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, **kw)
    eng.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    return cfg, eng


def _qwen_reqs(device):
    g = load_golden()
    a = (g["ids_a"].tolist(), [torch.from_numpy(g["frame_a"]).to(device)])
    b = ([256, 72, 105, 33, 90, 41], [])
    return a, b


def test_qwen_single_sequence_top_p_zero_is_greedy(device, monkeypatch):
    a, _ = _qwen_reqs(device)
    for chain, weights in (("1", "bf16"), ("0", "bf16"), ("1", "fp8")):
        monkeypatch.setenv("VIS_DECODE_CHAIN", chain)
        cfg, eng = _qwen_engine(device, decode_splits=4, decode_weights=weights)
        if chain == "1" and weights == "bf16":
            assert eng.chain_sync is not None
        greedy = eng.generate(*a, max_new_tokens=40, ignore_eos=True)
        for use_graph in (False, True):
            assert eng.generate(*a, max_new_tokens=40, ignore_eos=True, temperature=1.0, seed=3, top_p=0.0,
                                use_graph=use_graph) == greedy, (chain, weights, use_graph)
        jgreedy = eng.generate(*a, max_new_tokens=30, json_mode=True)
        assert eng.generate(*a, max_new_tokens=30, json_mode=True, temperature=1.0, top_p=0.0) == jgreedy
        # sampling with a nucleus: eager and graph agree, and the engine is back to the plain kernels afterwards
        s1 = eng.generate(*a, max_new_tokens=30, ignore_eos=True, temperature=1.0, seed=5, top_p=0.9, use_graph=False)
        s2 = eng.generate(*a, max_new_tokens=30, ignore_eos=True, temperature=1.0, seed=5, top_p=0.9)
        assert s1 == s2
        assert eng.smp_on is False
        assert eng.generate(*a, max_new_tokens=40, ignore_eos=True) == greedy


@pytest.mark.parametrize("form,weights", [("plain", "bf16"), ("plain", "fp8"), ("fused", "bf16"), ("rows", "bf16")])
def test_qwen_batched_forms_top_p_zero_is_greedy(device, monkeypatch, form, weights):
    monkeypatch.setenv("VIS_DECODE_FUSED", "1" if form == "fused" else "0")
    monkeypatch.setenv("VIS_ROWS_GEMV", "2" if form == "rows" else "0")
    cfg, eng = _qwen_engine(device, max_batch=17, decode_weights=weights)
    a, b = _qwen_reqs(device)
    reqs = [a, b]
    for jm in (False, True):
        greedy = eng.generate_batch(reqs, max_new_tokens=30, ignore_eos=not jm, json_mode=jm)
        for use_graph in (False, True):
            out = eng.generate_batch(reqs, max_new_tokens=30, ignore_eos=not jm, temperature=1.0, top_p=0.0,
                                     use_graph=use_graph, json_mode=jm)
            assert out == greedy, (form, weights, jm, use_graph)
            out = eng.generate_batch(reqs, max_new_tokens=30, ignore_eos=not jm, temperature=1.0, top_p=0.0,
                                     seeds=[1, 2], use_graph=use_graph, json_mode=jm)
            assert out == greedy, (form, weights, jm, use_graph, "seeds")


def test_qwen_seeds_make_replies_batch_independent(device):
    cfg, eng = _qwen_engine(device, max_batch=8)
    a, b = _qwen_reqs(device)
    kw = dict(max_new_tokens=40, ignore_eos=True, temperature=1.0, top_p=0.9)
    out = eng.generate_batch([a, b, a], seeds=[5, 9, 5], **kw)
    assert out[0] == out[2]
    assert eng.generate_batch([a, b, a], seeds=[5, 9, 5], **kw) == out           # repeatable
    re = eng.generate_batch([b, a, a], seeds=[9, 5, 5], **kw)                    # reordered
    assert re[0] == out[1] and re[1] == out[0] and re[2] == out[0]
    big = eng.generate_batch([a, b, a, b], seeds=[5, 9, 5, 9], **kw)             # another batch size
    assert big[:3] == out and big[3] == out[1]
    other = eng.generate_batch([a, b, a], seeds=[6, 9, 7], **kw)
    assert other[0] != out[0] and other[2] != out[0] and other[1] == out[1]
    single = eng.generate(*a, seed=5, **kw)
    assert single[:1] == out[0][:1]
    # seeds alone (top_p off): still per request
    s = eng.generate_batch([a, b, a], seeds=[5, 9, 5], max_new_tokens=40, ignore_eos=True, temperature=1.0)
    assert s[0] == s[2]


def test_qwen_off_means_unchanged(device, monkeypatch):
    cfg, eng = _qwen_engine(device, max_batch=4)
    a, b = _qwen_reqs(device)
    ref1 = eng.generate(*a, max_new_tokens=30, ignore_eos=True, temperature=0.8, seed=2)
    refb = eng.generate_batch([a, b], max_new_tokens=30, ignore_eos=True, temperature=0.8, seed=2)

    def boom(*args, **kw):
        raise AssertionError("vis_sample_f32 launched with sampling off")
    monkeypatch.setattr(hip, "sample", boom)
    for tp in (None, 1.0, 1):
        assert eng.generate(*a, max_new_tokens=30, ignore_eos=True, temperature=0.8, seed=2, top_p=tp) == ref1
        assert eng.generate_batch([a, b], max_new_tokens=30, ignore_eos=True, temperature=0.8, seed=2, top_p=tp) == refb


def _mllama(device):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=8)
    eng.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
    gm = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    a = (gm["a_ids"].tolist(), torch.from_numpy(gm["a_image"]).to(device))
    b = (gm["b_ids"].tolist(), torch.from_numpy(gm["b_image"]).to(device))
    return eng, a, b


def test_mllama_engine(device, monkeypatch):
    eng, a, b = _mllama(device)
    kw = dict(max_new_tokens=30, stop_on_eos=False)
    greedy = eng.generate(*a, **kw)
    for use_graph in (False, True):
        assert eng.generate(*a, temperature=1.0, top_p=0.0, use_graph=use_graph, **kw) == greedy
    assert eng.generate(*a, temperature=1.0, top_p=0.0, json_mode=True, max_new_tokens=30) == \
        eng.generate(*a, json_mode=True, max_new_tokens=30)
    gb = eng.generate_batch([a, b], **kw)
    for use_graph in (False, True):
        assert eng.generate_batch([a, b], temperature=1.0, top_p=0.0, seeds=[1, 2], use_graph=use_graph, **kw) == gb
    skw = dict(kw, temperature=1.0, top_p=0.9)
    out = eng.generate_batch([a, b, a], seeds=[5, 9, 5], **skw)
    assert out[0] == out[2]
    assert eng.generate_batch([a, b, a], seeds=[5, 9, 5], **skw) == out
    re = eng.generate_batch([b, a, a], seeds=[9, 5, 5], **skw)
    assert re == [out[1], out[0], out[0]]
    assert eng.generate_batch([a, b, a, b], seeds=[5, 9, 5, 9], **skw)[:3] == out
    other = eng.generate_batch([a, b, a], seeds=[6, 9, 7], **skw)
    assert other[0] != out[0] and other[1] == out[1]
    assert eng.generate(*a, seed=5, **skw)[:1] == out[0][:1]
    ref1 = eng.generate(*a, temperature=0.8, seed=2, **kw)
    refb = eng.generate_batch([a, b], temperature=0.8, seed=2, **kw)

    def boom(*args, **k):
        raise AssertionError("vis_sample_f32 launched with sampling off")
    monkeypatch.setattr(hip, "sample", boom)
    for tp in (None, 1.0):
        assert eng.generate(*a, temperature=0.8, seed=2, top_p=tp, **kw) == ref1
        assert eng.generate_batch([a, b], temperature=0.8, seed=2, top_p=tp, **kw) == refb


# ----------------------------------------------------------------------------- client
def _msgs(tmp_path, seed):
    from PIL import Image
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    p = tmp_path / f"img{seed}.png"
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    url = encode_image_optimized(str(p), 256)
    return [{"role": "user", "content": [{"type": "text", "text": "Inspect."},
                                         {"type": "image_url", "image_url": {"url": url}}]}]


@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_top_p_and_seed(device, tmp_path, model):
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    ma, mb = _msgs(tmp_path, 1), _msgs(tmp_path, 2)
    greedy = c.chat.completions.create(model=model, messages=ma, temperature=0.0, max_tokens=24, logprobs=True,
                                       top_logprobs=3)
    g1 = c.chat.completions.create(model=model, messages=ma, temperature=1.0, top_p=0.0, max_tokens=24, logprobs=True,
                                   top_logprobs=3)
    assert g1.choices[0].message.content == greedy.choices[0].message.content
    # logprobs keep their raw-logit meaning: the same tokens give the same numbers with or without the nucleus
    for e1, e0 in zip(g1.choices[0].logprobs.content, greedy.choices[0].logprobs.content):
        assert e1.token == e0.token and e1.logprob == pytest.approx(e0.logprob, abs=1e-6)
        assert [t.token for t in e1.top_logprobs] == [t.token for t in e0.top_logprobs]
    s1 = c.chat.completions.create(model=model, messages=ma, temperature=1.0, top_p=0.9, seed=7, max_tokens=24)
    s2 = c.chat.completions.create(model=model, messages=ma, temperature=1.0, top_p=0.9, seed=7, max_tokens=24)
    assert s1.choices[0].message.content == s2.choices[0].message.content
    many = c.complete_many(model, [ma, mb, ma], temperature=1.0, max_tokens=24, top_p=0.9, seed=7)
    assert many[0].choices[0].message.content == many[2].choices[0].message.content
