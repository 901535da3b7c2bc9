"""Lossless n-gram speculative decoding on the GPU: the three kernels of csrc/spec.hip against their definitions - R successive
vis_decode_attn launches (torch.equal, outputs and cache), spec.accept_ref, spec.propose - and the engine's speculative step
against its plain decode: the same tokens with drafts planted right, planted wrong, and proposed by the drafter."""
import math

import numpy as np
import pytest
import torch

from spec_cases import PROPOSE_CASES

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ vis_decode_attn_draft
def _attn_inputs(device, Hq, Hkv, T, R, seed):
    g = torch.Generator().manual_seed(seed)
    nq = (Hq + 2 * Hkv) * 128
    qkv = torch.randn((R, nq), generator=g).to(torch.bfloat16).to(device)
    ang = torch.rand((T, 128), generator=g) * 6.283
    cos, sin = torch.cos(ang).to(device), torch.sin(ang).to(device)
    k = torch.randn((Hkv, T, 128), generator=g).to(torch.bfloat16)
    v = torch.randn((Hkv, T, 128), generator=g).to(torch.bfloat16)
    return qkv, cos, sin, k, v


def _ws(device, R, Hq, nsplit):
    return (torch.zeros(R * Hq * nsplit * 128, dtype=torch.float32, device=device),
            torch.zeros(R * Hq * nsplit * 2, dtype=torch.float32, device=device))


def _successive(hip, device, qkv, cos, sin, k, v, step, Hq, Hkv, nsplit):
    """R plain launches at advancing steps on a copy of the cache; rows past the cache are not run."""
    T, R = k.shape[1], qkv.shape[0]
    kc, vc = k.clone().to(device), v.clone().to(device)
    out = torch.zeros((R, Hq * 128), dtype=torch.bfloat16, device=device)
    po, pm = _ws(device, 1, Hq, nsplit)
    valid = [r for r in range(R) if step + r < T]
    for r in valid:
        st = torch.tensor([step + r], dtype=torch.int32, device=device)
        hip.decode_attn(qkv[r], cos, sin, kc, vc, st, po, pm, out[r], Hq, Hkv, 128, nsplit, 128 ** -0.5)
    return out, kc, vc, valid


@pytest.mark.parametrize("heads", [(28, 4), (2, 1)])
@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("step", [0, 62, 126])
def test_decode_attn_draft_equals_successive_launches(device, heads, R, step):
    from vision_inspection_system_amd import hip
    Hq, Hkv = heads
    T = 256
    nsplit = T // hip.DECODE_KEYS_PER_SPLIT
    qkv, cos, sin, k, v = _attn_inputs(device, Hq, Hkv, T, R, 100 * step + R)
    want, kw, vw, valid = _successive(hip, device, qkv, cos, sin, k, v, step, Hq, Hkv, nsplit)
    assert valid == list(range(R))
    kc, vc = k.clone().to(device), v.clone().to(device)
    st = torch.tensor([step], dtype=torch.int32, device=device)
    out = torch.zeros((R, Hq * 128), dtype=torch.bfloat16, device=device)
    po, pm = _ws(device, R, Hq, nsplit)
    hip.decode_attn_draft(qkv, cos, sin, kc, vc, st, po, pm, out, Hq, Hkv, 128, nsplit, 128 ** -0.5)
    assert int(st.item()) == step
    assert torch.equal(out, want)
    assert torch.equal(kc[:, :step + R], kw[:, :step + R]) and torch.equal(vc[:, :step + R], vw[:, :step + R])
    assert torch.equal(kc, kw) and torch.equal(vc, vw)          # and nothing else moved


@pytest.mark.parametrize("heads", [(28, 4), (2, 1)])
def test_decode_attn_draft_rows_past_the_cache_touch_nothing(device, heads):
    """cache_tokens = 256, step = 254, R = 4: rows 0 and 1 are exact, rows 2 and 3 read and write nothing - the caches sit
    inside larger poisoned buffers that stay byte-identical around them, and output rows 2 and 3 keep their poison."""
    from vision_inspection_system_amd import hip
    Hq, Hkv = heads
    T, R, step, guard = 256, 4, 254, 4096
    nsplit = T // hip.DECODE_KEYS_PER_SPLIT
    qkv, cos, sin, k, v = _attn_inputs(device, Hq, Hkv, T, R, 7)
    want, kw, vw, valid = _successive(hip, device, qkv, cos, sin, k, v, step, Hq, Hkv, nsplit)
    assert valid == [0, 1]
    n = Hkv * T * 128
    poison = torch.full((2, n + 2 * guard), 0x7F7F, dtype=torch.int16, device=device).view(torch.bfloat16)
    kc, vc = poison[0, guard:guard + n].view(Hkv, T, 128), poison[1, guard:guard + n].view(Hkv, T, 128)
    kc.copy_(k)
    vc.copy_(v)
    before = poison.clone()
    st = torch.tensor([step], dtype=torch.int32, device=device)
    out = torch.full((R, Hq * 128), 0x7F7F, dtype=torch.int16, device=device).view(torch.bfloat16)
    po, pm = _ws(device, R, Hq, nsplit)
    hip.decode_attn_draft(qkv, cos, sin, kc, vc, st, po, pm, out, Hq, Hkv, 128, nsplit, 128 ** -0.5)
    assert torch.equal(out[:2], want[:2])
    assert torch.equal(out[2:].view(torch.int16), torch.full_like(out[2:].view(torch.int16), 0x7F7F))
    assert torch.equal(kc, kw) and torch.equal(vc, vw)
    b, a = before.view(torch.int16), poison.view(torch.int16)
    assert torch.equal(a[:, :guard], b[:, :guard]) and torch.equal(a[:, guard + n:], b[:, guard + n:])


def test_spec_entries_refuse_bad_arguments(device):
    from vision_inspection_system_amd import hip
    lib = hip.load()
    P = 4096
    assert lib.vis_decode_attn_draft(P, P, P, P, P, P, P, P, P, 28, 4, 128, 256, 4, 0.1, 5, 4608, None) == 1      # rows
    assert lib.vis_decode_attn_draft(P, P, P, P, P, P, P, P, P, 28, 4, 128, 256, 3, 0.1, 4, 4608, None) == 1      # splits cover
    assert lib.vis_decode_attn_draft(P, P, P, P, P, P, P, P, P, 28, 4, 128, 256, 4, 0.1, 4, 4600, None) == 1      # row stride
    assert lib.vis_spec_accept(P, 1000, 999, 2, P, P, P, P, P, P, 64, P, P, P, None) == 1                        # ld < V
    assert lib.vis_spec_accept(P, 1000, 1000, 5, P, P, P, P, P, P, 64, P, P, P, None) == 1                       # rows
    assert lib.vis_spec_draft(P, 8, P, P, 64, P, P, 4, 4, 2, 512, P, P, None) == 1                               # k
    assert lib.vis_spec_draft(P, 8, P, P, 64, P, P, 3, 9, 2, 512, P, P, None) == 1                               # lookup_max
    assert lib.vis_spec_draft(P, 8, P, P, 64, P, P, 3, 2, 3, 512, P, P, None) == 1                               # min > max


# ------------------------------------------------------------------------------------------------------ vis_spec_accept
def _run_accept(device, logits, draft, d, step, limit, T=64):
    from vision_inspection_system_amd import hip, spec
    R = logits.shape[0]
    tokens0 = np.arange(1000, 1000 + T, dtype=np.int32)
    counters0 = [5, 7, 3]
    dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=device)      # noqa: E731
    lg = torch.from_numpy(logits).to(device)
    dr = dev(list(draft) + [0] * (max(1, R - 1) - len(draft)))
    nd, lim, tok, cur, st, cnt = dev([d]), dev([limit]), dev(tokens0), dev([-1]), dev([step]), dev(counters0)
    hip.spec_accept(lg, dr, nd, lim, torch.empty(256 * R, device=device), torch.empty(256 * R, dtype=torch.int32, device=device),
                    tok, cur, st, cnt)
    got = (tok.cpu().numpy(), int(cur.item()), int(st.item()), cnt.cpu().tolist())
    want = spec.accept_ref(logits, draft, d, step, limit, tokens0, counters0)
    assert np.array_equal(got[0], want[0])
    assert got[1] == (-1 if want[1] is None else want[1])
    assert got[2] == want[2] and got[3] == want[3]
    return got


def _rows(V, picks, seed=0):
    lg = np.random.default_rng(seed).standard_normal((len(picks), V)).astype(np.float32)
    for r, p in enumerate(picks):
        lg[r, p] = 50.0
    return lg


def test_spec_accept_cases(device):
    V = 1000
    lg = _rows(V, [11, 22, 33, 44])
    tok, cur, st, cnt = _run_accept(device, lg, [11, 22, 33], 3, 10, 60)            # all drafts accepted
    assert (cur, st, cnt) == (44, 14, [6, 10, 6]) and tok[10:14].tolist() == [11, 22, 33, 44]
    tok, cur, st, cnt = _run_accept(device, lg, [12, 22, 33], 3, 10, 60)            # first draft rejected
    assert (cur, st, cnt) == (11, 11, [6, 10, 3]) and tok[10] == 11 and tok[11] == 1011
    tok, cur, st, cnt = _run_accept(device, lg, [11, 22, 99], 3, 10, 60)            # partial
    assert (cur, st, cnt) == (33, 13, [6, 10, 5])
    tok, cur, st, cnt = _run_accept(device, lg, [11, 22, 33], 0, 10, 60)            # d = 0: the drafts are not looked at
    assert (cur, st, cnt) == (11, 11, [6, 7, 3])
    tok, cur, st, cnt = _run_accept(device, lg, [11, 22, 33], 3, 10, 11)            # the limit cuts an accepted run
    assert (cur, st, cnt) == (22, 12, [6, 10, 4]) and tok[12] == 1012
    tok, cur, st, cnt = _run_accept(device, lg, [11, 22, 33], 3, 12, 11)            # past the limit: nothing at all
    assert (cur, st, cnt) == (-1, 12, [5, 7, 3])
    # an exact tie: the pick is the LOWER id, so a draft equal to the higher one is rejected
    tie = _rows(V, [11, 22])
    tie[0, 700] = tie[0, 11]
    tok, cur, st, cnt = _run_accept(device, tie, [700], 1, 10, 60)
    assert (cur, st, cnt) == (11, 11, [6, 8, 3])
    tok, cur, st, cnt = _run_accept(device, tie, [11], 1, 10, 60)
    assert (cur, st, cnt) == (22, 12, [6, 8, 4])
    # an all-NaN row picks id 0
    nan = _rows(V, [11, 22, 33])
    nan[1, :] = np.nan
    tok, cur, st, cnt = _run_accept(device, nan, [11, 0], 2, 10, 60)
    assert (cur, st, cnt) == (33, 13, [6, 9, 5]) and tok[10:13].tolist() == [11, 0, 33]
    # R = 1, 2, 3 with a draft count larger than the rows allow
    for R in (1, 2, 3):
        _run_accept(device, _rows(V, [5, 6, 7][:R], seed=R), [5, 6][:R - 1], 3, 0, 60)


def test_spec_accept_full_vocabulary(device):
    V = 152064
    lg = _rows(V, [152063, 0, 77777, 4])
    lg[2, 151000] = lg[2, 77777]                                # a tie far apart: two different stage-1 workgroups
    tok, cur, st, cnt = _run_accept(device, lg, [152063, 0, 77777], 3, 3, 60)
    assert (cur, st) == (4, 7) and tok[3:7].tolist() == [152063, 0, 77777, 4]
    _run_accept(device, lg, [152063, 0, 151000], 3, 3, 60)


# ------------------------------------------------------------------------------------------------------- vis_spec_draft
def _run_draft(device, history, split, k, lookup_max, lookup_min, vocab=1 << 20):
    """History = a prompt part of ``split`` ids and a generated part that sits somewhere in a token row."""
    from vision_inspection_system_amd import hip
    dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=device)      # noqa: E731
    prompt, gen = list(history[:split]), list(history[split:])
    gen0 = 3
    row = [-7] * gen0 + gen + [-9] * 5
    draft, nd = dev([-1, -1, -1]), dev([-5])
    hip.spec_draft(dev(prompt + [-3] * 2), dev([len(prompt)]), dev(row), dev([gen0]), dev([gen0 + len(gen)]), k, lookup_max,
                   lookup_min, vocab, draft, nd)
    d = int(nd.item())
    got = draft.cpu().tolist()
    assert got[d:] == [-1] * (3 - d)                            # nothing past the count is written
    return got[:d]


def test_spec_draft_equals_propose_on_hand_made_cases(device):
    from vision_inspection_system_amd import spec
    for hist, split, k, hi, lo, want in PROPOSE_CASES:
        assert spec.propose(hist, k, hi, lo) == want
        assert _run_draft(device, hist, split, k, hi, lo) == want


@pytest.mark.parametrize("k", [1, 2, 3])
def test_spec_draft_equals_propose_on_random_histories(device, k):
    from vision_inspection_system_amd import spec
    rng = np.random.default_rng(k)
    matched = 0
    for i in range(200):
        L = int(rng.integers(1, 301)) if i else 300
        hist = rng.integers(0, 4, L).tolist()
        split = int(rng.integers(1, L + 1))
        hi = int(rng.integers(1, 9))
        lo = int(rng.integers(1, hi + 1))
        want = spec.propose(hist, k, hi, lo)
        matched += bool(want)
        assert _run_draft(device, hist, split, k, hi, lo) == want, (hist, split, k, hi, lo)
    assert matched > 100


# --------------------------------------------------------------------------------------------------------------- engine
N_NEW = 24
PHRASE = [72, 105, 33, 116, 104, 101, 114, 101, 32, 119]


def _prompts():
    rng = np.random.default_rng(11)
    return {"repeats": [256] + PHRASE * 5 + PHRASE[:4], "random": [256] + rng.integers(1, 490, 41).tolist()}


@pytest.fixture(scope="module", params=["tiny", "tiny25"])
def model(request, device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny() if request.param == "tiny" else Qwen2VLConfig.tiny_2_5()
    return cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)


@pytest.fixture(scope="module", params=["bf16", "fp8", "mxfp4"])
def eng(request, model, device):
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg, w = model
    return Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_weights=request.param)      # max_batch = 1: no batched buffers


@pytest.mark.parametrize("R", [2, 4])
def test_engine_planted_drafts(eng, R):
    """The true continuation planted as drafts: every draft is accepted, ceil(23 / R) steps.  Every draft wrong: none is,
    23 steps.  The tokens are the plain decode's either way."""
    from vision_inspection_system_amd.spec import SpecConfig
    ids = _prompts()["random"]
    eng.prefill(ids, [], max_new_tokens=N_NEW + R)
    eng.decode(N_NEW - 1, use_graph=False)
    ref = eng.generated(N_NEW)
    start = len(ids) - 1
    for wrong in (False, True):
        eng.prefill(ids, [], max_new_tokens=N_NEW + R)
        buf = eng._spec_begin(SpecConfig(R - 1, 4, 2), N_NEW)
        steps = 0
        while True:
            p = int(eng.step.item()) - start                    # tokens so far; ref[p] is the next one
            if p >= N_NEW:
                break
            drafts = [(t + 1) % 490 if wrong else t for t in ref[p:p + R - 1]]
            buf.ids[1:1 + len(drafts)].copy_(torch.tensor(drafts, dtype=torch.int32))
            buf.n_draft.fill_(len(drafts))
            eng._decode_step_spec(R, propose=False)
            steps += 1
            assert steps <= N_NEW
        assert eng.generated(N_NEW) == ref
        c = buf.read_counters()
        want_steps = N_NEW - 1 if wrong else math.ceil((N_NEW - 1) / R)
        assert steps == want_steps and c[0] == want_steps
        assert c[2] == (0 if wrong else N_NEW - 1 - want_steps)
        assert int(eng.step.item()) == start + N_NEW            # the limit: exactly N_NEW tokens


def test_engine_generate_speculative_equals_plain(eng):
    prompts = _prompts()
    plain, fin = {}, {}
    for name, ids in prompts.items():
        for n, ig in ((N_NEW, True), (N_NEW, False), (5, True), (6, True)):
            plain[name, n, ig] = eng.generate(ids, [], max_new_tokens=n, ignore_eos=ig)
            fin[name, n, ig] = eng.last_finish
    accepted = 0
    for name, ids in prompts.items():
        for k in (1, 3):
            for graph in (True, False):
                for ig in (True, False):
                    got = eng.generate(ids, [], max_new_tokens=N_NEW, ignore_eos=ig, use_graph=graph, speculative=k)
                    assert got == plain[name, N_NEW, ig], (name, k, graph, ig)
                    assert eng.last_finish == fin[name, N_NEW, ig]
                    t = eng.last_timing
                    assert t["spec_steps"] >= 1 and 0 <= t["spec_accepted"] <= t["spec_proposed"] <= k * t["spec_steps"]
                    accepted += t["spec_accepted"]
        for n in (5, 6):                                        # the last step's run is cut by the limit
            got = eng.generate(ids, [], max_new_tokens=n, ignore_eos=True, speculative=3)
            assert got == plain[name, n, True] and len(got) == n and eng.last_finish == fin[name, n, True]
        spec_dict = {"method": "ngram", "num_speculative_tokens": 2, "prompt_lookup_max": 3, "prompt_lookup_min": 1}
        assert eng.generate(ids, [], max_new_tokens=N_NEW, ignore_eos=True, speculative=spec_dict) == plain[name, N_NEW, True]
    # nothing is left behind: the plain request after all of them
    for name, ids in prompts.items():
        assert eng.generate(ids, [], max_new_tokens=N_NEW, ignore_eos=True) == plain[name, N_NEW, True]
        assert "spec_steps" not in eng.last_timing


def test_engine_speculative_at_the_end_of_the_context(device, model):
    """A prompt that leaves room for 6 tokens: the rows of the last steps lie past the cache and are skipped; the reply is the
    plain one."""
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg, w = model
    e = Qwen2VLEngine(cfg, w, device, max_ctx=64)
    ids = [256] + (PHRASE * 6)[:56]
    want = e.generate(ids, [], max_new_tokens=20, ignore_eos=True)
    assert len(want) == 64 - len(ids) - 1
    assert e.generate(ids, [], max_new_tokens=20, ignore_eos=True, speculative=3) == want


def test_mllama_engine_refuses(device):
    from vision_inspection_system_amd.client import get_model
    lm = get_model("synthetic:mllama-tiny")
    with pytest.raises(ValueError, match="Qwen2-VL"):
        lm.engine.generate([1, 2, 3], None, max_new_tokens=4, speculative=2)


# --------------------------------------------------------------------------------------------------------------- client
def test_client_create_speculative_same_text_and_usage(device):
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": "list: alpha beta gamma; list: alpha beta gamma; list: alpha beta"}]
    for model_id in ("synthetic:tiny", "synthetic:tiny25"):
        plain = c.chat.completions.create(model=model_id, messages=msgs, max_tokens=20)
        for k in (1, 3):
            sp = c.chat.completions.create(model=model_id, messages=msgs, max_tokens=20,
                                           speculative={"method": "ngram", "num_speculative_tokens": k})
            assert sp.choices[0].message.content == plain.choices[0].message.content
            assert sp.choices[0].finish_reason == plain.choices[0].finish_reason
            assert sp.usage == plain.usage
    with pytest.raises(ValueError, match="Qwen2-VL"):
        c.chat.completions.create(model="synthetic:mllama-tiny", messages=msgs, max_tokens=4,
                                  speculative={"method": "ngram", "num_speculative_tokens": 1})
