"""``n`` choices per request on MI355X: the forked decode attention (vis_decode_attn_forked / vis_decode_attn_parts_forked)
bit for bit against its unforked sibling, the engines' generate_batch(.., n=) against the same request sent n times, the
request switches per choice, the client, and the launches with ``n`` off."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden
from vision_inspection_system_amd import hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HD, T = 128, 256


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


def _randn(shape, device, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(device)


def _bits(t):
    return t.view(torch.int16)


# ----------------------------------------------------------------------------- 1. the kernel
def _fork_case(B, parents):
    """parent / fork_len of a batch of B: the two parents are roots, every other sequence forks from one of them with a fork
    length of 0, 64 or 128 (mixed inside the batch)."""
    parent, flen = list(range(B)), [0] * B
    kids = [b for b in range(B) if b not in parents]
    for i, b in enumerate(kids):
        parent[b], flen[b] = parents[i % 2], (64, 128, 0)[i % 3]
    return parent, flen


def _attn_inputs(device, Hq, Hkv, B):
    nq = (Hq + 2 * Hkv) * HD
    kc, vc = _randn((B, Hkv, T, HD), device, 31), _randn((B, Hkv, T, HD), device, 32)
    ang = torch.rand((B, T, HD // 2), generator=torch.Generator().manual_seed(33)) * 6.28
    emb = torch.cat((ang, ang), -1)
    qkv = _randn((B, nq), device, 34)
    ns = -(-T // hip.DECODE_KEYS_PER_SPLIT)                 # as the engines choose it
    po = torch.empty(B * Hq * ns * HD, dtype=torch.float32, device=device)
    pml = torch.empty(B * Hq * ns * 2, dtype=torch.float32, device=device)
    return kc, vc, emb.cos().to(device), emb.sin().to(device), qkv, ns, po, pml


def _launch(sibling, qkv, cos, sin, kc, vc, step, po, pml, Hq, Hkv, ns, **share):
    B = kc.shape[0]
    out = torch.full((B, Hq * HD), 7.0, dtype=torch.bfloat16, device=kc.device)
    if sibling == "attn":
        hip.decode_attn(qkv, cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, HD ** -0.5, **share)
    else:       # one slab that holds the projection row as f32: the finalised row is qkv itself
        rows, nq = hip.part_rows(B), qkv.shape[1]
        part = torch.full((rows * nq,), float("nan"), dtype=torch.float32, device=kc.device)
        part.view(rows, nq)[:B] = qkv.float()
        hip.decode_attn_parts(part, 1, cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, HD ** -0.5, **share)
    return out


# batch 4 cannot hold a parent 5: the 28/4 grouping runs at batch 4 with parents {0, 2} and at batch 8 with {0, 5}
SHAPES = [(28, 4, 4, (0, 2)), (28, 4, 8, (0, 5)), (32, 8, 16, (0, 5))]


@pytest.mark.parametrize("sibling", ["attn", "parts"])
@pytest.mark.parametrize("mode", ["1", "0", "2"])          # the engines' choice, the split form, the streaming form
@pytest.mark.parametrize("Hq,Hkv,B,parents", SHAPES)
def test_forked_attention_is_bit_identical(device, monkeypatch, Hq, Hkv, B, parents, mode, sibling):
    """Reference: the unforked sibling on caches in which every child holds a copy of its parent's rows.  Forked run: the
    children's rows below their fork length are NaN.  Steps at fork_len, fork_len + 1 and 255.  Outputs equal bit for bit, the
    appended row in the child's own cache, no row of any cache touched besides the appended ones, the parents' caches
    included.  (28/4 at batch 4 and 8: Hkv * B < 128, the split form by default; 32/8 at batch 16: the streaming form.)"""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    parent, flen = _fork_case(B, parents)
    assert set(parent[b] for b in range(B) if flen[b]) == set(parents) and {0, 64, 128} <= set(flen)
    kc, vc, cos, sin, qkv, ns, po, pml = _attn_inputs(device, Hq, Hkv, B)
    for b in range(B):
        kc[b, :, :flen[b]] = kc[parent[b], :, :flen[b]]
        vc[b, :, :flen[b]] = vc[parent[b], :, :flen[b]]
    par_d = torch.tensor(parent, dtype=torch.int32, device=device)
    fl_d = torch.tensor(flen, dtype=torch.int32, device=device)
    for kind in range(3):
        steps = [(flen[b], flen[b] + 1, 255)[kind] for b in range(B)]
        step = torch.tensor(steps, dtype=torch.int32, device=device)
        k_ref, v_ref = kc.clone(), vc.clone()
        want = _launch(sibling, qkv, cos, sin, k_ref, v_ref, step, po, pml, Hq, Hkv, ns)
        k_f, v_f = kc.clone(), vc.clone()
        for b in range(B):
            k_f[b, :, :flen[b]] = float("nan")
            v_f[b, :, :flen[b]] = float("nan")
        k_in, v_in = k_f.clone(), v_f.clone()
        got = _launch(sibling, qkv, cos, sin, k_f, v_f, step, po, pml, Hq, Hkv, ns, fork=(par_d, fl_d))
        assert torch.isfinite(want.float()).all()
        assert torch.equal(_bits(got), _bits(want)), f"step kind {kind}: outputs differ in sequences " \
            f"{sorted(set((_bits(got) != _bits(want)).nonzero()[:, 0].tolist()))}"
        for b in range(B):
            s = steps[b]
            assert torch.equal(_bits(k_f[b, :, s]), _bits(k_ref[b, :, s])) and torch.equal(_bits(v_f[b, :, s]), _bits(v_ref[b, :, s])), \
                f"sequence {b}: appended row {s} is not in its own cache"
            keep = torch.ones(T, dtype=torch.bool, device=device)
            keep[s] = False
            assert torch.equal(_bits(k_f[b][:, keep]), _bits(k_in[b][:, keep])) and \
                torch.equal(_bits(v_f[b][:, keep]), _bits(v_in[b][:, keep])), f"sequence {b}: a row besides {s} was written"
        for p in parents:       # the parent's cache: what the unforked run leaves, byte for byte
            assert torch.equal(_bits(k_f[p]), _bits(k_ref[p])) and torch.equal(_bits(v_f[p]), _bits(v_ref[p]))


@pytest.mark.parametrize("sibling", ["attn", "parts"])
@pytest.mark.parametrize("mode", ["0", "2"])
def test_forked_attention_clamps_its_tables(device, monkeypatch, mode, sibling):
    """A table holding parent 99 and fork_len 70 (and a negative parent, a fork length past the cache) runs to completion
    and equals the run on the clamped and rounded table: the kernel forms no address from what the table says."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv, B = 28, 4, 4
    kc, vc, cos, sin, qkv, ns, po, pml = _attn_inputs(device, Hq, Hkv, B)
    step = torch.tensor([200, 201, 255, 202], dtype=torch.int32, device=device)
    raw = ([0, 99, -3, 0], [0, 70, 130, 100000])
    clamped = ([0, 3, 0, 0], [0, 64, 128, 192])
    res = []
    for parent, flen in (raw, clamped):
        k1, v1 = kc.clone(), vc.clone()
        out = _launch(sibling, qkv, cos, sin, k1, v1, step, po, pml, Hq, Hkv, ns,
                      fork=(torch.tensor(parent, dtype=torch.int32, device=device),
                            torch.tensor(flen, dtype=torch.int32, device=device)))
        res.append((out, k1, v1))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.isfinite(res[0][0].float()).all()


def test_forked_entry_points_refuse_bad_arguments(device):
    Hq, Hkv, B = 28, 4, 4
    kc, vc, cos, sin, qkv, ns, po, pml = _attn_inputs(device, Hq, Hkv, B)
    step = torch.full((B,), 200, dtype=torch.int32, device=device)
    tab = torch.zeros(B, dtype=torch.int32, device=device)
    out = torch.empty((B, Hq * HD), dtype=torch.bfloat16, device=device)
    lib = hip.load()
    P = lambda t: t.data_ptr()      # noqa: E731
    args = lambda batch, par, fl: (P(qkv), P(cos), P(sin), P(kc), P(vc), P(step), P(po), P(pml), P(out), Hq, Hkv, HD, T, ns,   # noqa: E731
                                   0.088, batch, qkv.stride(0), kc.stride(0), cos.stride(0), par, fl, None)
    assert lib.vis_decode_attn_forked(*args(B, None, P(tab))) == 1
    assert lib.vis_decode_attn_forked(*args(B, P(tab), None)) == 1
    assert lib.vis_decode_attn_forked(*args(0, P(tab), P(tab))) == 1
    assert lib.vis_decode_attn_forked(*args(65, P(tab), P(tab))) == 1
    with pytest.raises(hip.HipLibraryError):      # tables and shared_len exclude each other; tables have one entry per sequence
        hip.decode_attn(qkv, cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, 0.088, shared_len=64, fork=(tab, tab))
    with pytest.raises(hip.HipLibraryError):
        hip.decode_attn(qkv, cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, 0.088, fork=(tab[:3], tab[:3]))


# ----------------------------------------------------------------------------- 2. - 3. the Qwen2-VL engine
def _qwen_engine(device, **kw):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=8, **kw)
    eng.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    eng.min_shared_prefix = 64        # the 128-token text prefix of a and b is shared: the fork tables carry it too
    return cfg, eng


def _qwen_reqs(cfg, device):
    """a, b: one image each behind the same 150 tokens of text (S = 161 and 157: fork_len 128, 33 and 29 rows copied);
    c: text only, S = 6 (fork_len 0)."""
    g = load_golden()
    fa, fb = torch.from_numpy(g["frame_a"]).to(device), torch.from_numpy(g["frame_b1"]).to(device)
    text = np.random.default_rng(5).integers(3, 200, 150).tolist()

    def ids_for(f, tail):
        n_img = (f.shape[0] // cfg.patch) * (f.shape[1] // cfg.patch) // cfg.merge ** 2
        return text + [cfg.vision_start_id] + [cfg.image_token_id] * n_img + [cfg.vision_end_id] + tail
    a, b = (ids_for(fa, [7, 8, 9]), [fa]), (ids_for(fb, [11]), [fb])
    assert len(a[0]) % 64 and len(a[0]) >= 128 and len(b[0]) % 64
    return a, b, ([256, 72, 105, 33, 90, 41], [])


KW = dict(max_new_tokens=24, ignore_eos=True, temperature=1.0, top_p=0.9)


def _poison(eng):
    """Every KV cache row NaN: a child's rows below its fork length are never written afterwards, a read of them shows."""
    eng.kcache_b.fill_(float("nan"))
    eng.vcache_b.fill_(float("nan"))


def _check_qwen_n(eng, a, b, c, **kw):
    kw = dict(KW, **kw)
    for use_graph in (False, True):
        want = eng.generate_batch([a, a, a], seeds=[5, 6, 7], use_graph=use_graph, **kw)
        _poison(eng)
        got = eng.generate_batch([a], n=3, seeds=[5], use_graph=use_graph, **kw)
        assert got[0] == want, f"use_graph={use_graph}"
        assert len({tuple(t) for t in want}) == 3          # three different replies: the seeds matter
        want = eng.generate_batch([a, a, b], seeds=[5, 6, 9], use_graph=use_graph, **kw)
        _poison(eng)
        got = eng.generate_batch([a, b], n=[2, 1], seeds=[5, 9], use_graph=use_graph, **kw)
        assert got == [want[:2], want[2:]], f"mixed, use_graph={use_graph}"
        want = eng.generate_batch([c, c, c], seeds=[5, 6, 7], use_graph=use_graph, **kw)
        _poison(eng)
        assert eng.generate_batch([c], n=3, seeds=[5], use_graph=use_graph, **kw)[0] == want, "text only, fork_len 0"
    assert eng.fork_on is False


def test_qwen_n_equals_the_request_sent_n_times(device):
    cfg, eng = _qwen_engine(device)
    a, b, c = _qwen_reqs(cfg, device)
    _check_qwen_n(eng, a, b, c)
    assert len(eng.last_finish) == 1 and len(eng.last_finish[0]) == 3 and all(f[0] == "length" for f in eng.last_finish[0])
    # n is off unless asked for; 1 nests today's result; the total must fit the slots
    one = eng.generate_batch([a], seeds=[5], **KW)
    assert eng.generate_batch([a], n=1, seeds=[5], **KW) == [one] and len(eng.last_finish[0]) == 1
    assert eng.generate_batch([a, b], n=1, seeds=[5, 9], **KW) == [[t] for t in eng.generate_batch([a, b], seeds=[5, 9], **KW)]
    for reqs, bad in (([a], 9), ([a, b], [5, 4]), ([a, b], 5), ([a], 0), ([a], True), ([a], 2.0), ([a], "2"), ([a], [2, 1])):
        with pytest.raises(ValueError):
            eng.generate_batch(reqs, n=bad, **KW)
    # without seeds every choice takes the seed of the slot it lands in, as three requests do
    assert eng.generate_batch([a], n=3, seed=4, **KW)[0] == eng.generate_batch([a, a, a], seed=4, **KW)
    # temperature 0: all choices equal (and still decoded)
    g = eng.generate_batch([a], n=3, max_new_tokens=12, ignore_eos=True)[0]
    assert g[0] == g[1] == g[2] and len(g[0]) == 12


@pytest.mark.parametrize("env,weights", [({"VIS_DECODE_SHARED": "0"}, "bf16"), ({"VIS_QKV_FOLD": "0"}, "bf16"), ({}, "fp8")])
def test_qwen_n_under_the_decode_switches(device, monkeypatch, env, weights):
    """Equality against the same configuration's three-request run."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, eng = _qwen_engine(device, decode_weights=weights)
    _check_qwen_n(eng, *_qwen_reqs(cfg, device))


def _check_switch(eng, a, **kw):
    kw = dict(KW, **kw)
    want = eng.generate_batch([a, a, a], seeds=[5, 6, 7], **kw)
    assert not any(isinstance(t, Exception) for t in want)
    want_lp, want_fin = eng.last_logprobs, eng.last_finish
    _poison(eng)
    got = eng.generate_batch([a], n=3, seeds=[5], **kw)
    assert got[0] == want
    assert eng.last_finish == [want_fin]
    if want_lp is None:
        assert eng.last_logprobs is None
    else:
        assert len(eng.last_logprobs) == 1 and len(eng.last_logprobs[0]) == 3
        for r, w in zip(eng.last_logprobs[0], want_lp):
            for f in ("token_logprobs", "top_ids", "top_logprobs"):
                assert np.array_equal(np.asarray(getattr(r, f)), np.asarray(getattr(w, f))), f
    return want


@pytest.fixture(scope="module")
def qwen(device):
    cfg, eng = _qwen_engine(device)
    return (eng,) + _qwen_reqs(cfg, device)


def test_n_with_logprobs(qwen):
    _check_switch(qwen[0], qwen[1], logprobs=2)


def test_n_with_json_mode(qwen):
    _check_switch(qwen[0], qwen[1], json_mode=True, ignore_eos=False)


def test_n_with_repetition_penalty(qwen):
    """The prompt's flags must be in every choice's penalty row."""
    eng, a = qwen[0], qwen[1]
    want = _check_switch(eng, a, repetition_penalty=1.3)
    assert want != eng.generate_batch([a, a, a], seeds=[5, 6, 7], **KW)      # the penalty changes these replies


def test_n_with_a_stop_string(qwen):
    """One stop string that cuts at least one choice but not all."""
    eng, a = qwen[0], qwen[1]
    free = eng.generate_batch([a, a, a], seeds=[5, 6, 7], **KW)
    tok = eng.tokenizer
    texts = [b"".join(bytes(tok.token_bytes(t)) for t in toks) for toks in free]
    stop = None
    # a short piece of one reply, behind its start, that some other reply lacks
    for n_bytes, tx in ((k, tx) for k in (2, 1, 3) for tx in texts):
        for o in range(4, len(tx) - n_bytes):
            s = tx[o:o + n_bytes]
            if not all(s in other for other in texts):
                try:
                    stop = s.decode("utf-8")
                except UnicodeDecodeError:
                    continue
                break
        if stop:
            break
    assert stop, "no stop string separates these replies"
    _check_switch(eng, a, stop=stop)
    reasons = [f[0] for f in eng.last_finish[0]]
    assert "stop" in reasons and "length" in reasons


def test_n_with_logit_bias(qwen):
    eng, a = qwen[0], qwen[1]
    free = eng.generate_batch([a, a, a], seeds=[5, 6, 7], **KW)
    banned = {int(free[0][1]): -100, int(free[1][2]): -100}
    want = _check_switch(eng, a, logit_bias=banned)
    assert all(t not in banned for toks in want for t in toks)


# ----------------------------------------------------------------------------- 4. the Mllama engine
def test_mllama_n_equals_the_request_sent_n_times(device):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=8)
    eng.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
    gm = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    more = np.random.default_rng(6).integers(3, 200, 130).tolist()
    a = (gm["a_ids"].tolist() + more, torch.from_numpy(gm["a_image"]).to(device))          # S = 145: fork_len 128
    b = (gm["b_ids"].tolist() + more[:30], torch.from_numpy(gm["b_image"]).to(device))     # S = 45: fork_len 0
    assert len(a[0]) % 64 and len(a[0]) >= 128
    kw = dict(max_new_tokens=24, stop_on_eos=False, temperature=1.0, top_p=0.9)
    for use_graph in (False, True):
        want = eng.generate_batch([a, a, a], seeds=[5, 6, 7], use_graph=use_graph, **kw)
        _poison(eng)
        assert eng.generate_batch([a], n=3, seeds=[5], use_graph=use_graph, **kw)[0] == want, f"use_graph={use_graph}"
        assert len({tuple(t) for t in want}) == 3
        want = eng.generate_batch([a, a, b], seeds=[5, 6, 9], use_graph=use_graph, **kw)
        _poison(eng)
        assert eng.generate_batch([a, b], n=[2, 1], seeds=[5, 9], use_graph=use_graph, **kw) == [want[:2], want[2:]]
    assert eng.fork_on is False


# ----------------------------------------------------------------------------- 5. the client
def _msgs(tmp_path, seed):
    from PIL import Image
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    p = tmp_path / f"img{seed}.png"
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    url = encode_image_optimized(str(p), 256)
    return [{"role": "user", "content": [{"type": "text", "text": "Inspect this part and describe every defect you find. " * 3},
                                         {"type": "image_url", "image_url": {"url": url}}]}]


@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_n(device, tmp_path, model):
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    m = _msgs(tmp_path, 1)
    kw = dict(temperature=1.0, max_tokens=16, logprobs=True)
    r = c.chat.completions.create(model=model, messages=m, n=3, seed=11, **kw)
    assert [ch.index for ch in r.choices] == [0, 1, 2]
    done = 0
    for i, ch in enumerate(r.choices):
        one = c.complete_many(model, [m, m, m], seed=11 + i, **kw)[0]      # the same batch size: the same arithmetic family
        assert len(one.choices) == 1
        assert ch.message.content == one.choices[0].message.content and ch.finish_reason == one.choices[0].finish_reason
        assert [(e.token, e.logprob) for e in ch.logprobs.content] == [(e.token, e.logprob) for e in one.choices[0].logprobs.content]
        assert r.usage["prompt_tokens"] == one.usage["prompt_tokens"]      # counted once
        done += one.usage["completion_tokens"]
    assert r.usage["completion_tokens"] == done and r.usage["total_tokens"] == r.usage["prompt_tokens"] + done
    assert len({ch.message.content for ch in r.choices}) > 1
    base = c.chat.completions.create(model=model, messages=m, seed=11, **kw)
    for n in (None, 1):
        same = c.chat.completions.create(model=model, messages=m, seed=11, n=n, **kw)
        assert same.choices == base.choices and same.usage == base.usage and same.model == base.model
    with pytest.raises(ValueError):
        c.chat.completions.create(model=model, messages=m, n=0)


# ----------------------------------------------------------------------------- 6. off means unchanged
def test_off_means_unchanged_and_on_changes_the_attention_only(device):
    """The launch recorder of tests/test_decode_transcript_gpu.py: a batch without ``n`` names no forked entry point and makes
    the calls of the golden transcript; with n=[2, 1] the only names that differ are the attention's."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import json
    import gen_decode_transcript as G
    with open(os.path.join(HERE, "golden", "decode_transcript.json")) as f:
        golden = json.load(f)["configs"]
    got = G.record("qwen_b3_streamk_fold1", device)["calls"]
    assert not G.first_difference(got, golden["qwen_b3_streamk_fold1"]["calls"])

    def names(n, reqs_of):
        with G.vis_env({}), G.recording() as rec:
            cfg, eng = G._qwen(device, max_batch=8)
            reqs = reqs_of(G._qwen_requests(cfg, device, 2, False))
            rec.arm_method(eng, "_decode_step_batched")
            out = eng.generate_batch(reqs, max_new_tokens=4, use_graph=False, ignore_eos=True, **({"n": n} if n else {}))
            assert not any(isinstance(o, Exception) for o in out)
            torch.cuda.synchronize(device)
            return [c.split("(")[0] for c in rec.calls]
    two = names(None, lambda r: r)
    assert two and not any("_forked" in c for c in two)
    three = names(None, lambda r: [r[0], r[1], r[0]])          # the same three slots without n
    forked = names([2, 1], lambda r: r)
    assert any("_forked" in c for c in forked)
    diff = {(x, y) for x, y in zip(three, forked) if x != y}
    assert len(three) == len(forked) and diff == {("vis_decode_attn_parts", "vis_decode_attn_parts_forked")}
