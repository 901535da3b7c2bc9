"""Speculative decoding and predicted outputs on the Auditor (MllamaEngine), on the GPU.  The two draft cross-attention
kernels (vis_decode_cross_attn_draft, vis_decode_cross_attn_fp8_draft) against R single-row launches on the same inputs; the
engine's speculative step through cross-attention layers against its plain decode; the client and the agents' switch behind
VIS_AUDITOR_SPECULATIVE.  Every comparison is torch.equal / ==: "lossless" means the plain reply, token for token."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, SCALE = 1e-5, 128 ** -0.5
T_KEYS = 192                                        # three splits of 64 keys
COUNTS = (1, 64, 65, 191, 192)
HEADS = [(8, 2), (2, 1), (1, 1)]
PATTERN = 0x3C3C                                    # what a buffer a refused call must not touch is filled with


# ------------------------------------------------------------------------------------------------ the two draft kernels
def _inputs(device, fmt, Hq, Hkv, count, seed=0):
    """Four distinct q rows in a packed [4, (Hq + 2 Hkv) * 128] buffer and the static keys / values in ``fmt``; rows at or past
    ``count`` hold the poison of tests/test_cross_kv_gpu.py (NaN codes and inf scales; bf16 keys / values: NaN rows)."""
    rng = np.random.default_rng(1000 * Hq + seed)
    nq = (Hq + 2 * Hkv) * 128
    qbuf = torch.from_numpy(rng.standard_normal((4, nq)).astype(np.float32)).to(torch.bfloat16).to(device)
    w = torch.from_numpy((1 + 0.1 * rng.standard_normal(128)).astype(np.float32)).to(torch.bfloat16).to(device)
    if fmt == "bf16":
        k = rng.standard_normal((Hkv, T_KEYS, 128)).astype(np.float32)
        v = rng.standard_normal((Hkv, T_KEYS, 128)).astype(np.float32)
        k[:, count:], v[:, count:] = np.nan, np.nan
        kv = (torch.from_numpy(k).to(torch.bfloat16).to(device), torch.from_numpy(v).to(torch.bfloat16).to(device))
    else:
        def codes():
            c = rng.integers(0, 256, size=(Hkv, T_KEYS, 128)).astype(np.uint8)
            c[(c & 0x7F) == 0x7F] = 0x38                          # no NaN code among the live rows
            c[:, count:] = 0x7F
            return c
        kq, vq = codes(), codes()
        ksc = (rng.uniform(0.5, 1.5, (Hkv, T_KEYS)) * 2.0 ** -9).astype(np.float32)
        vsc = (rng.uniform(0.5, 1.5, (Hkv, T_KEYS)) * 2.0 ** -7).astype(np.float32)
        ksc[:, count:], vsc[:, count:] = np.inf, np.inf
        kv = tuple(torch.from_numpy(a).to(device) for a in (kq, ksc, vq, vsc))
    return qbuf, w, kv, torch.tensor([count - 1], dtype=torch.int32, device=device)


def _ws(device, R, Hq, ns):
    return (torch.full((R * Hq * ns * 128,), float("nan"), dtype=torch.float32, device=device),
            torch.full((R * Hq * ns * 2,), float("nan"), dtype=torch.float32, device=device))


def _single(hip, fmt, q, w, kv, nk, Hq, Hkv):
    """R single-row launches, row by row -> [R, Hq * 128]."""
    ns = T_KEYS // hip.DECODE_KEYS_PER_SPLIT
    fn = hip.decode_cross_attn if fmt == "bf16" else hip.decode_cross_attn_fp8
    out = torch.zeros((q.shape[0], Hq * 128), dtype=torch.bfloat16, device=q.device)
    for r in range(q.shape[0]):
        po, pm = _ws(q.device, 1, Hq, ns)
        fn(q[r].contiguous(), w, *kv, nk, po, pm, out[r], Hq, Hkv, 128, ns, SCALE, EPS)
    return out


def _draft(hip, fmt, q, w, kv, nk, Hq, Hkv):
    ns = T_KEYS // hip.DECODE_KEYS_PER_SPLIT
    fn = hip.decode_cross_attn_draft if fmt == "bf16" else hip.decode_cross_attn_fp8_draft
    out = torch.full((q.shape[0], Hq * 128), float("nan"), dtype=torch.bfloat16, device=q.device)
    po, pm = _ws(q.device, q.shape[0], Hq, ns)
    fn(q, w, *kv, nk, po, pm, out, Hq, Hkv, 128, ns, SCALE, EPS)
    return out


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("heads", HEADS)
def test_draft_rows_equal_single_row_launches(device, fmt, heads):
    """R = 1..4 over every key count: output row r == the single-row launch on q row r (q = the leading columns of packed rows,
    q_ld = (Hq + 2 Hkv) * 128), the rows past the count poisoned.  Row 0 at R = 4 == the R = 1 launch, and permuting the q
    rows permutes the output rows: a row depends neither on ``rows`` nor on what the other rows hold."""
    from vision_inspection_system_amd import hip
    Hq, Hkv = heads
    perm = [2, 0, 3, 1]
    for count in COUNTS:
        qbuf, w, kv, nk = _inputs(device, fmt, Hq, Hkv, count)
        q = qbuf[:, :Hq * 128]
        assert q.stride(0) == (Hq + 2 * Hkv) * 128
        want = _single(hip, fmt, q, w, kv, nk, Hq, Hkv)
        assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0
        if count > 1:       # (one key: every row's output is that key's value) the rows really differ
            assert len({want[r].view(torch.int16).cpu().numpy().tobytes() for r in range(4)}) == 4
        by_rows = {}
        for R in (1, 2, 3, 4):
            by_rows[R] = _draft(hip, fmt, q[:R], w, kv, nk, Hq, Hkv)
            assert torch.equal(by_rows[R], want[:R]), (count, R)
        assert torch.equal(by_rows[4][0], by_rows[1][0])
        qp = qbuf[perm][:, :Hq * 128]
        assert torch.equal(_draft(hip, fmt, qp, w, kv, nk, Hq, Hkv), want[perm]), count


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_draft_refusals_touch_nothing(device, fmt):
    """rows * G > 16 (heads (16, 2) and (8, 1) with three rows), rows 0 and rows 5: refused, and the output and the partial
    buffers keep the pattern they were filled with."""
    from vision_inspection_system_amd import hip
    lib = hip.load()
    ns = T_KEYS // hip.DECODE_KEYS_PER_SPLIT
    name = "vis_decode_cross_attn_draft" if fmt == "bf16" else "vis_decode_cross_attn_fp8_draft"
    fn = hip.decode_cross_attn_draft if fmt == "bf16" else hip.decode_cross_attn_fp8_draft
    for Hq, Hkv in ((16, 2), (8, 1)):
        qbuf, w, kv, nk = _inputs(device, fmt, Hq, Hkv, 100)
        extra = torch.zeros((2, qbuf.shape[1]), dtype=torch.bfloat16, device=device)
        q6 = torch.cat([qbuf, extra])[:, :Hq * 128]                                  # six rows to slice from
        out = torch.full((6, Hq * 128), PATTERN, dtype=torch.int16, device=device)
        po = torch.full((6 * Hq * ns * 128,), PATTERN, dtype=torch.int32, device=device)
        pm = torch.full((6 * Hq * ns * 2,), PATTERN, dtype=torch.int32, device=device)
        outb, pof, pmf = out.view(torch.bfloat16), po.view(torch.float32), pm.view(torch.float32)
        with pytest.raises(hip.HipLibraryError):
            fn(q6[:3], w, *kv, nk, pof, pmf, outb[:3], Hq, Hkv, 128, ns, SCALE, EPS)
        for rows in (3, 0, 5):
            rc = getattr(lib, name)(q6.data_ptr(), w.data_ptr(), *(t.data_ptr() for t in kv), nk.data_ptr(), po.data_ptr(),
                                    pm.data_ptr(), out.data_ptr(), Hq, Hkv, 128, T_KEYS, ns, SCALE, EPS, rows, q6.stride(0),
                                    torch.cuda.current_stream().cuda_stream)
            assert rc == 1, (Hq, rows)
        with pytest.raises(hip.HipLibraryError):
            fn(q6[:5], w, *kv, nk, pof, pmf, outb[:5], Hq, Hkv, 128, ns, SCALE, EPS)
        with pytest.raises(hip.HipLibraryError):
            fn(q6[:0], w, *kv, nk, pof, pmf, outb[:0], Hq, Hkv, 128, ns, SCALE, EPS)
        torch.cuda.synchronize()
        for t in (out, po, pm):
            assert torch.equal(t, torch.full_like(t, PATTERN))
        # two rows fit a group of 8 and run
        got = _draft(hip, fmt, q6[:2], w, kv, nk, Hq, Hkv)
        assert torch.equal(got, _single(hip, fmt, q6[:2], w, kv, nk, Hq, Hkv))


# --------------------------------------------------------------------------------------------------------------- engine
N_NEW = 24
PHRASE = [72, 105, 33, 116, 104, 101, 114, 101, 32, 119]
FORMATS = [(dw, xkv) for dw in ("bf16", "fp8", "mxfp4") for xkv in ("bf16", "fp8")]


@pytest.fixture(scope="module")
def tiny(device):
    from vision_inspection_system_amd import mllama_weights as MW
    cfg = MW.MllamaConfig.tiny()
    return cfg, MW.pack_device_weights(cfg, MW.synth_state_dict(cfg, 0), device)


@pytest.fixture(scope="module")
def frame(device):
    return torch.from_numpy(np.random.default_rng(2).integers(0, 256, (40, 56, 3), dtype=np.uint8)).to(device)


def _engine(tiny, device, dw="bf16", xkv="bf16", max_ctx=256, **kw):
    """A private engine every time: the cached one of the client is never touched."""
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    cfg, w = tiny
    return MllamaEngine(cfg, w, device, max_ctx=max_ctx, decode_weights=dw, cross_kv=xkv, speculative=True, **kw)


def _prompt(cfg, image: bool, n_phrases: int = 4):
    body = PHRASE * n_phrases + PHRASE[:4]
    return ([cfg.image_token_id] if image else []) + [min(cfg.vocab - 1, 300)] + body


@pytest.fixture(scope="module", params=FORMATS, ids=lambda p: f"{p[0]}-x{p[1]}")
def eng(request, tiny, device):
    return _engine(tiny, device, *request.param)


@pytest.mark.parametrize("image", [True, False], ids=["image", "text"])
def test_generate_speculative_and_prediction_equal_plain(eng, frame, image):
    """generate(speculative=k) == generate() for k = 1, 3, eager and replayed; the same with a prediction - the plain reply, a
    copy with every 4th id replaced, unrelated ids - whose counters equal spec.simulate_prediction's; with the plain reply as
    the prediction drafts are accepted through the cross layers and the steps are fewer than the tokens."""
    from vision_inspection_system_amd import spec
    cfg = eng.cfg
    ids, fr = _prompt(cfg, image), (frame if image else None)
    plain = eng.generate(ids, fr, max_new_tokens=N_NEW, stop_on_eos=False)
    fin = eng.last_finish
    assert len(plain) == N_NEW and "spec_steps" not in eng.last_timing
    assert eng.has_image == image
    for k in (1, 3):
        for graph in (False, True):
            got = eng.generate(ids, fr, max_new_tokens=N_NEW, stop_on_eos=False, use_graph=graph, speculative=k)
            assert got == plain, (k, graph)
            assert eng.last_finish == fin
            t = eng.last_timing
            assert t["spec_steps"] >= 1 and 0 <= t["spec_accepted"] <= t["spec_proposed"] <= k * t["spec_steps"]
    for n in (5, 6):                                            # the limit cuts the last step's run
        assert eng.generate(ids, fr, max_new_tokens=n, stop_on_eos=False, speculative=3) == plain[:n]
    preds = {"same": list(plain), "every4th": [(t + 1) % 490 if i % 4 == 3 else t for i, t in enumerate(plain)],
             "unrelated": [(7 * i + 3) % 490 for i in range(N_NEW)]}
    for name, pred in preds.items():
        for k, graph in ((3, True), (1, False)):
            got = eng.generate(ids, fr, max_new_tokens=N_NEW, stop_on_eos=False, use_graph=graph, speculative=k,
                               prediction=pred)
            assert got == plain, (name, k)
            sim = spec.simulate_prediction(plain, ids, pred, k, 4, 2, N_NEW, cfg.vocab)
            t = eng.last_timing
            got_c = {n: t[n] for n in ("spec_steps", "spec_proposed", "spec_accepted", "pred_accepted", "pred_rejected")}
            want_c = {n: sim[n] for n in got_c}
            assert got_c == want_c, (name, k, graph)      # steps issued behind the limit change nothing and count nothing
            if name == "same":
                assert t["spec_accepted"] > 0 and t["spec_steps"] < N_NEW - 1
    got = eng.generate(ids, fr, max_new_tokens=N_NEW, stop_on_eos=False, prediction=preds["same"])      # alone: k = 3
    assert got == plain and eng.last_timing["spec_steps"] == math.ceil((N_NEW - 1) / 4)
    assert eng.generate(ids, fr, max_new_tokens=N_NEW, stop_on_eos=False) == plain      # nothing is left behind
    assert "spec_steps" not in eng.last_timing


@pytest.mark.parametrize("image", [True, False], ids=["image", "text"])
@pytest.mark.parametrize("R", [2, 4])
def test_planted_drafts(eng, frame, image, R):
    """The true continuation planted as drafts: every draft is accepted, ceil(23 / R) steps.  Every draft wrong: none is, 23
    steps.  The tokens are the plain decode's either way."""
    from vision_inspection_system_amd.spec import SpecConfig
    ids, fr = _prompt(eng.cfg, image), (frame if image else None)
    eng.prefill(ids, fr)
    eng.decode(N_NEW - 1, use_graph=False)
    ref = eng.generated(N_NEW)
    start = len(ids) - 1
    for wrong in (False, True):
        eng.prefill(ids, fr)
        buf = eng._spec_begin(SpecConfig(R - 1, 4, 2), N_NEW)
        steps = 0
        while True:
            p = int(eng.step.item()) - start
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
        assert int(eng.step.item()) == start + N_NEW


@pytest.mark.parametrize("xkv", ["bf16", "fp8"])
def test_prompt_six_tokens_short_of_the_context(tiny, device, frame, xkv):
    """max_ctx 64 and a prompt that leaves room for 6 tokens: the rows of the last steps lie past the cache; the reply is the
    plain one."""
    e = _engine(tiny, device, "bf16", xkv, max_ctx=64)
    ids = ([e.cfg.image_token_id] + [300] + PHRASE * 6)[:57]
    want = e.generate(ids, frame, max_new_tokens=20, stop_on_eos=False)
    assert len(want) == 64 - len(ids) - 1 == 6
    for k in (1, 3):
        assert e.generate(ids, frame, max_new_tokens=20, stop_on_eos=False, speculative=k) == want
    assert e.generate(ids, frame, max_new_tokens=20, stop_on_eos=False, prediction=list(want)) == want


def test_reply_keeps_its_eos(tiny, device, frame):
    """keep_eos: a reply that ends on EOS keeps the EOS token, speculative or not.  The EOS id is made the 6th token of the
    plain reply by naming that token an EOS id on a private config."""
    import dataclasses
    cfg, w = tiny
    probe = _engine(tiny, device)
    ids = _prompt(cfg, True)
    free = probe.generate(ids, frame, max_new_tokens=N_NEW, stop_on_eos=False)
    eos = next(t for i, t in enumerate(free) if i >= 3 and t not in free[:i])      # first fresh id from the 4th token on
    cut = free.index(eos) + 1
    e = _engine((dataclasses.replace(cfg, eos_ids=(eos,)), w), device)
    plain = e.generate(ids, frame, max_new_tokens=N_NEW)
    assert plain == free[:cut] and plain[-1] == eos and e.last_finish[0][0] == "eos"
    for kw in (dict(speculative=1), dict(speculative=3), dict(prediction=list(free))):
        assert e.generate(ids, frame, max_new_tokens=N_NEW, **kw) == plain, kw
        assert e.last_finish[0][0] == "eos"


def test_default_engine_still_refuses(tiny, device):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    cfg, w = tiny
    e = MllamaEngine(cfg, w, device, max_ctx=64)
    assert e.speculative_supported is False and MllamaEngine.speculative_supported is False
    for kw in (dict(speculative=2), dict(prediction=[1, 2, 3])):
        with pytest.raises(ValueError, match="Qwen2-VL"):
            e.generate([1, 2, 3], None, max_new_tokens=4, **kw)
    with pytest.raises(ValueError, match="speculative=True"):
        e.generate([1, 2, 3], None, max_new_tokens=4, speculative=2)
    s = _engine(tiny, device, max_ctx=64)
    with pytest.raises(ValueError, match="temperature"):
        s.generate([1, 2, 3], None, max_new_tokens=4, speculative=2, temperature=0.5)
    with pytest.raises(ValueError, match="one request"):
        s.generate_batch([([1, 2, 3], None)], max_new_tokens=4, prediction=[1, 2])


# ------------------------------------------------------------------------------------------------------ client and agents
MSGS = [{"role": "user", "content": "list: alpha beta gamma; list: alpha beta gamma; list: alpha beta"}]
MODEL = "synthetic:mllama-tiny"


def test_client_behind_the_switch(device, monkeypatch):
    from vision_inspection_system_amd import agents
    from vision_inspection_system_amd.client import LocalVLMClient, drop_models, get_model
    c = LocalVLMClient()
    monkeypatch.delenv("VIS_AUDITOR_SPECULATIVE", raising=False)
    drop_models()
    try:
        plain = c.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=20)
        with pytest.raises(ValueError, match="Qwen2-VL"):
            c.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, speculative={"method": "ngram", "num_speculative_tokens": 1})
        with pytest.raises(ValueError, match="Qwen2-VL"):
            c.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, prediction={"type": "content", "content": "x"})
        assert agents.speculative_kwargs(c, MODEL, 0.0, {}) == {}
        drop_models()
        monkeypatch.setenv("VIS_AUDITOR_SPECULATIVE", "2")
        for k in (1, 3):
            sp = c.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=20,
                                           speculative={"method": "ngram", "num_speculative_tokens": k})
            assert sp.choices[0].message.content == plain.choices[0].message.content
            assert sp.choices[0].finish_reason == plain.choices[0].finish_reason
            assert sp.usage == plain.usage
        pr = c.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=20,
                                       prediction={"type": "content", "content": plain.choices[0].message.content})
        assert pr.choices[0].message.content == plain.choices[0].message.content
        t = get_model(MODEL).engine.last_timing      # (the reply of random weights need not survive text -> ids: no count is pinned;
        assert pr.usage["completion_tokens_details"] == {"accepted_prediction_tokens": t["pred_accepted"],      # the engine tests do)
                                                         "rejected_prediction_tokens": t["pred_rejected"]}
        assert get_model(MODEL).engine.speculative_supported is True
        assert {n: v for n, v in pr.usage.items() if n != "completion_tokens_details"} == plain.usage
        assert agents.speculative_kwargs(c, MODEL, 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 2}}
        assert agents.speculative_kwargs(c, MODEL, 0.7, {}) == {}
        assert agents.speculative_kwargs(c, MODEL, 0.0, {"stop": ["x"]}) == {}
        assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, {}) == {}      # VIS_SPECULATIVE is the Qwen engines' switch
        with pytest.raises(ValueError):
            c.complete_many(MODEL, [MSGS], max_tokens=4, prediction={"type": "content", "content": "x"})
    finally:
        monkeypatch.delenv("VIS_AUDITOR_SPECULATIVE", raising=False)
        drop_models()
