"""Repetition, frequency and presence penalties on MI355X: vis_penalize_f32 / vis_penalty_prompt against the float64
reference (penalties.penalize_ref) over every element, row independence, graph replay; then the engines' wiring step by
step, the decode forms, composition with JSON mode / nucleus sampling / logprobs, and the client's keywords.

Bound of every comparison with the reference (penalties.error_bound):
    |out - ref| <= 2^-23 (|x| max(r, 1 / r) + |f| c + |q|)
- the value is reached in three f32 roundings: the multiply or divide (at most 2^-24 |x| max(r, 1 / r)), f c + q as one fused
multiply-add (at most 2^-24 (|f| c + |q|)) and their difference (at most 2^-24 of a result no larger than the bracket); the
first two are roundings of parts of the bracket, so the sum stays within 2 x 2^-24 of the whole."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import load_golden
from vision_inspection_system_amd import hip
from vision_inspection_system_amd.penalties import error_bound, penalize_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TRIPLES = [(1.3, 0.5, 0.2), (1.0, 0.0, 0.0), (0.8, -1.0, 2.0), (2.0, 2.0, -0.5), (1.05, 0.0, 0.0), (1.0, 0.0, 1.5),
           (1.0, 1.25, 0.0)]
T_TOK = 16


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Rows:
    """B sequences driven by hand: logits in a padded buffer, prompts marked, tokens appended from the host."""

    def __init__(self, V, B, ld, ld_out, prompts, triples, step0):
        self.V, self.B = V, B
        self.xbuf = torch.zeros((B, ld), dtype=torch.float32, device="cuda")
        self.obuf = torch.full((B, ld_out), 7.0, dtype=torch.float32, device="cuda")
        self.x, self.out = self.xbuf[:, :V], self.obuf[:, :V]
        self.state = hip.penalty_state(V, B, "cuda")
        self.params = torch.tensor(triples, dtype=torch.float32, device="cuda").reshape(B, 3).contiguous()
        self.tokens = torch.full((B, T_TOK), -1, dtype=torch.int32, device="cuda")
        self.step = torch.tensor(step0, dtype=torch.int32, device="cuda")
        self.prompts, self.triples, self.step0 = prompts, triples, list(step0)
        self.hist = [[] for _ in range(B)]
        for b in range(B):
            hip.penalty_prompt(self.state[b], V, torch.from_numpy(np.asarray(prompts[b], dtype=np.int32)).cuda())

    def append(self, b, tok):
        pos = self.step0[b] + len(self.hist[b])
        self.tokens[b, pos] = tok
        self.hist[b].append(int(tok))
        self.step[b] = pos + 1

    def launch(self, x_np):
        self.xbuf[:, :self.V].copy_(torch.from_numpy(x_np))
        before = self.xbuf.clone()
        if self.B == 1:
            hip.penalize(self.x[0], self.state, self.params, self.tokens[0], self.step, self.out[0])
        else:
            hip.penalize(self.x, self.state, self.params, self.tokens, self.step, self.out)
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int32), self.xbuf.view(torch.int32)), "the raw logits changed"
        assert bool((self.obuf[:, self.V:] == 7.0).all()), "written past V"
        return self.out.cpu().numpy()

    def check(self, x_np, out, what):
        V = self.V
        for b in range(self.B):
            r, f, q = self.triples[b]
            ref = penalize_ref(x_np[b], self.prompts[b], self.hist[b], r, f, q)
            bound = error_bound(x_np[b], self.hist[b], r, f, q)
            err = np.abs(out[b].astype(np.float64) - ref)
            worst = int(np.argmax(err - bound))
            assert (err <= bound).all(), (what, b, worst, float(err[worst]), float(bound[worst]), float(x_np[b, worst]))
            seen = np.zeros(V, bool)
            ids = np.asarray(list(self.prompts[b]) + self.hist[b], dtype=np.int64)
            seen[ids[(ids >= 0) & (ids < V)]] = True
            same = _bits(out[b]) == _bits(x_np[b])
            assert same[~seen].all(), (what, b, "an unseen id changed")
            if (r, f, q) == (1.0, 0.0, 0.0):
                assert same.all(), (what, b, "the neutral triple changed a logit")


def _logits(rng, B, V):
    x = (rng.normal(0, 4, (B, V)) * rng.uniform(0.3, 3, (B, 1))).astype(np.float32)
    x[rng.random((B, V)) < 0.02] = 0.0                       # exact zeros
    return x


def _prompt(rng, V):
    n = int(rng.integers(8, min(2000, 3 * V)))
    p = rng.integers(0, V + 10, n)                           # ids >= V among them: skipped
    p[-3:] = [V, V + 5, V - 1]
    p[:n // 4] = p[n // 4:2 * (n // 4)]                      # repeated ids
    return p.tolist()


@pytest.mark.parametrize("V", [152064, 128256, 1000])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_kernel_matches_reference(V, B):
    for variant in range(2 if B == 1 else 1):                # one row: once penalised, once the neutral triple
        rng = np.random.default_rng(V + 7 * B + variant)
        # leading dimensions above V; at 3 rows odd ones (rows not 16-byte aligned: the scalar form of the kernel)
        ld, ld_out = (V + 5, V + 3) if B == 3 else (V + 8, V + 4)
        triples = [TRIPLES[(b + variant) % len(TRIPLES)] for b in range(B)]
        prompts = [_prompt(rng, V) for _ in range(B)]
        rows = _Rows(V, B, ld, ld_out, prompts, triples, [b % 3 for b in range(B)])
        x = _logits(rng, B, V)
        rows.check(x, rows.launch(x), "first launch: nothing to fold")
        for b in range(B):
            rows.append(b, int(rng.integers(0, V)))
        x = _logits(rng, B, V)
        rows.check(x, rows.launch(x), "one token")
        for b in range(B):
            rows.append(b, rows.hist[b][0])                  # the same token again
        x = _logits(rng, B, V)
        rows.check(x, rows.launch(x), "a token repeated")
        for b in range(B):
            inside = [t for t in prompts[b] if t < V]
            rows.append(b, inside[0])                        # a token that is also in the prompt
            if b % 2:
                rows.append(b, int(rng.integers(0, V)))      # two tokens to fold in one launch
        x = _logits(rng, B, V)
        out3 = rows.launch(x)
        rows.check(x, out3, "a prompt token generated")
        out4 = rows.launch(x)                                # nothing new to fold: the same result
        rows.check(x, out4, "nothing new")
        assert (_bits(out3) == _bits(out4)).all()


def test_many_tokens_fold_in_one_launch():
    """A launch that finds many unfolded tokens (all positions since the anchor) counts each of them."""
    V, B = 1000, 2
    rng = np.random.default_rng(3)
    rows = _Rows(V, B, V, V, [[1, 2, 3], [5]], [(1.3, 0.5, 0.2), (1.0, 1.0, 1.0)], [0, 2])
    x = _logits(rng, B, V)
    rows.check(x, rows.launch(x), "anchor")
    for k in range(12):
        rows.append(0, [7, 7, 9, 1][k % 4])
        rows.append(1, 5)
    rows.check(x, rows.launch(x), "twelve tokens in one launch")


def test_row_independence():
    V = 152064
    rng = np.random.default_rng(21)
    xs = [_logits(rng, 1, V)[0] for _ in range(3)]
    prompt = _prompt(rng, V)
    triple = (1.3, 0.5, 0.2)
    hist = [int(rng.integers(0, V)), prompt[0] % V, None]
    hist[2] = hist[0]
    outs = []
    for B, slot in ((1, 0), (3, 2), (64, 63)):
        r2 = np.random.default_rng(100 + B)
        prompts = [_prompt(r2, V) for _ in range(B)]
        triples = [TRIPLES[(b + 2) % len(TRIPLES)] for b in range(B)]
        prompts[slot], triples[slot] = prompt, triple
        step0 = [int(r2.integers(0, 4)) for _ in range(B)]
        rows = _Rows(V, B, V, V, prompts, triples, step0)
        got = []
        for k in range(3):
            x = _logits(r2, B, V)
            x[slot] = xs[k]
            got.append(_bits(rows.launch(x)[slot]).copy())
            for b in range(B):
                rows.append(b, hist[k] if b == slot else int(r2.integers(0, V)))
        outs.append(got)
    for k in range(3):
        assert (outs[0][k] == outs[1][k]).all() and (outs[0][k] == outs[2][k]).all(), k


def test_graph_replay_equals_eager():
    V, B, steps = 152064, 4, 8
    g = torch.Generator(device="cuda").manual_seed(12)
    x = (torch.randn((B, V), generator=g, device="cuda") * 2).contiguous()
    tokens = torch.zeros((B, T_TOK), dtype=torch.int32, device="cuda")
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    wv = torch.empty(256 * B, dtype=torch.float32, device="cuda")
    wi = torch.empty(256 * B, dtype=torch.int32, device="cuda")
    state = hip.penalty_state(V, B, "cuda")
    params = torch.zeros((B, 3), dtype=torch.float32, device="cuda")
    out = torch.empty((B, V), dtype=torch.float32, device="cuda")
    prompt = torch.arange(0, 3000, 3, dtype=torch.int32, device="cuda")

    def one():
        hip.penalize(x, state, params, tokens, step, out)
        hip.argmax(out, wv, wi, tokens, cur, step, 0.0, 0)

    def reset(vals):
        state.zero_(); step.zero_(); tokens.zero_()
        params.copy_(torch.tensor(vals, dtype=torch.float32))
        for b in range(B):
            hip.penalty_prompt(state[b], V, prompt)

    reset([TRIPLES[0]] * B)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        one()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one()
    first = [TRIPLES[0], TRIPLES[1], TRIPLES[2], TRIPLES[3]]
    second = [TRIPLES[5], TRIPLES[6], TRIPLES[1], TRIPLES[3]]
    results = []
    for replay in (True, False):
        reset(first)
        for k in range(steps):
            if k == steps // 2:                              # new values in device memory between two replays
                params.copy_(torch.tensor(second, dtype=torch.float32))
            graph.replay() if replay else one()
        results.append((tokens[:, :steps].clone(), out.clone()))
    assert torch.equal(results[0][0], results[1][0])
    assert torch.equal(results[0][1].view(torch.int32), results[1][1].view(torch.int32))
    toks = results[0][0].cpu().numpy()
    assert len(set(toks[3].tolist())) == steps               # r = 2, f = 2 throughout: the greedy pick moves on at every step
    assert len(set(toks[1, :steps // 2].tolist())) == 1      # neutral values: the argmax of x again and again ...
    assert toks[1, steps // 2] != toks[1, 0]                 # ... until f = 1.25 arrives and finds it counted four times


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


def _family(device, family):
    """(engine, request a, request b, keywords of a greedy run that ignores EOS)."""
    if family == "qwen":
        _, eng = _qwen_engine(device, max_batch=8)
        a, b = _qwen_reqs(device)
        return eng, a, b, dict(ignore_eos=True)
    eng, a, b = _mllama(device)
    return eng, a, b, dict(stop_on_eos=False)


class _Recorder:
    """hip.penalize wrapped: every call records, per slot it served, the raw row, the penalised row and the step."""

    def __init__(self, eng, monkeypatch):
        self.eng, self.calls, self.orig = eng, [], hip.penalize
        monkeypatch.setattr(hip, "penalize", self)

    def __call__(self, logits, state, params, tokens, step, out):
        self.orig(logits, state, params, tokens, step, out)
        V = logits.shape[-1]
        slot0 = (out.data_ptr() - self.eng._pen.out.data_ptr()) // (4 * V)
        raw, pen = logits.reshape(-1, V).cpu().numpy(), out.reshape(-1, V).cpu().numpy()
        for i in range(raw.shape[0]):
            self.calls.append((slot0 + i, raw[i].copy(), pen[i].copy(), int(step.reshape(-1)[i])))

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _check_request(calls, slot, prompt_ids, toks, triple, what):
    """Every pick of one request: the recorded penalised row against the reference of (raw row, prompt, tokens so far), and
    the returned token = first argmax of the recorded penalised row."""
    mine = [c for c in calls if c[0] == slot]
    assert len(mine) == len(toks), (what, len(mine), len(toks))
    r, f, q = triple
    for k, (_, raw, pen, step) in enumerate(mine):
        assert step == len(prompt_ids) - 1 + k, (what, k, step)
        ref = penalize_ref(raw, prompt_ids, toks[:k], r, f, q)
        err = np.abs(pen.astype(np.float64) - ref)
        bound = error_bound(raw, toks[:k], r, f, q)
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), (what, k, worst, float(err[worst]), float(bound[worst]))
        assert toks[k] == int(np.argmax(pen)), (what, k, toks[k], int(np.argmax(pen)))


@pytest.mark.parametrize("family", ["qwen", "mllama"])
def test_engine_wiring_step_by_step(device, monkeypatch, family):
    eng, a, b, kw = _family(device, family)
    rec = _Recorder(eng, monkeypatch)
    n = 12
    t1, t2 = (1.3, 0.5, 0.2), (1.0, 0.0, 1.5)
    plain = eng.generate(*a, max_new_tokens=n, use_graph=False, **kw)
    assert rec.take() == []
    singles = []
    for rep in range(2):                                     # twice in a row on the same engine: the state is reset
        toks = eng.generate(*a, max_new_tokens=n, use_graph=False, repetition_penalty=t1[0], frequency_penalty=t1[1],
                            presence_penalty=t1[2], **kw)
        assert len(toks) == n
        _check_request(rec.take(), 0, a[0], toks, t1, (family, "generate", rep))
        singles.append(toks)
    assert singles[0] == singles[1]

    def batch(reqs, triples):
        out = eng.generate_batch(reqs, max_new_tokens=n, use_graph=False, repetition_penalty=[t[0] for t in triples],
                                 frequency_penalty=[t[1] for t in triples], presence_penalty=[t[2] for t in triples], **kw)
        calls = rec.take()
        for slot, (req, toks, tr) in enumerate(zip(reqs, out, triples)):
            assert len(toks) == n
            _check_request(calls, slot, req[0], toks, tr, (family, "batch", slot))
        return out
    o1 = batch([a, b, a], [t1, t2, t1])
    o2 = batch([a, b, a], [t1, t2, t1])
    assert o1 == o2 and o1[0] == o1[2]
    o3 = batch([b, a, a], [t2, t1, t1])                      # the slots change, the replies do not
    assert o3 == [o1[1], o1[0], o1[0]]
    # a neutral request shares a batch with a penalised one: it gets its plain reply
    plain_b = eng.generate_batch([a, b], max_new_tokens=n, use_graph=False, **kw)
    assert rec.take() == []
    o4 = batch([a, b], [(1.0, 0.0, 0.0), t2])
    assert o4[0] == plain_b[0]
    assert eng.pen_on is False


def test_qwen_single_sequence_forms_graph_equals_eager(device, monkeypatch):
    a, _ = _qwen_reqs(device)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.2)
    for chain, weights in (("1", "bf16"), ("0", "bf16"), ("1", "fp8")):
        monkeypatch.setenv("VIS_DECODE_CHAIN", chain)
        cfg, eng = _qwen_engine(device, decode_splits=4, decode_weights=weights)
        if chain == "1" and weights == "bf16":
            assert eng.chain_sync is not None
        plain = eng.generate(*a, max_new_tokens=40, ignore_eos=True)
        eager = eng.generate(*a, max_new_tokens=40, ignore_eos=True, use_graph=False, **pen)
        assert eng.generate(*a, max_new_tokens=40, ignore_eos=True, use_graph=True, **pen) == eager, (chain, weights)
        assert eng.generate(*a, max_new_tokens=40, ignore_eos=True, use_graph=True, **pen) == eager      # the cached graph
        assert eager != plain
        assert eng.pen_on is False and eng.generate(*a, max_new_tokens=40, ignore_eos=True) == plain


@pytest.mark.parametrize("form,weights", [("plain", "bf16"), ("plain", "fp8"), ("fused", "bf16"), ("rows", "bf16")])
def test_qwen_batched_forms_graph_equals_eager(device, monkeypatch, form, weights):
    monkeypatch.setenv("VIS_DECODE_FUSED", "1" if form == "fused" else "0")
    monkeypatch.setenv("VIS_ROWS_GEMV", "2" if form == "rows" else "0")
    cfg, eng = _qwen_engine(device, max_batch=17, decode_weights=weights)
    a, b = _qwen_reqs(device)
    pen = dict(repetition_penalty=[1.3, 1.0], frequency_penalty=[0.5, 0.0], presence_penalty=[0.2, 1.5])
    eager = eng.generate_batch([a, b], max_new_tokens=30, ignore_eos=True, use_graph=False, **pen)
    for _ in range(2):
        assert eng.generate_batch([a, b], max_new_tokens=30, ignore_eos=True, use_graph=True, **pen) == eager, (form, weights)
    # other values through the graph captured above: they live in device memory
    pen2 = dict(repetition_penalty=1.05, frequency_penalty=[2.0, 1.0])
    assert eng.generate_batch([a, b], max_new_tokens=30, ignore_eos=True, use_graph=True, **pen2) == \
        eng.generate_batch([a, b], max_new_tokens=30, ignore_eos=True, use_graph=False, **pen2)


def test_mllama_graph_equals_eager(device):
    eng, a, b = _mllama(device)
    kw = dict(max_new_tokens=30, stop_on_eos=False)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.2)
    eager = eng.generate(*a, use_graph=False, **pen, **kw)
    assert eng.generate(*a, use_graph=True, **pen, **kw) == eager
    penb = dict(repetition_penalty=[1.3, 1.0], frequency_penalty=[0.5, 0.0], presence_penalty=[0.2, 1.5])
    eb = eng.generate_batch([a, b], use_graph=False, **penb, **kw)
    assert eng.generate_batch([a, b], use_graph=True, **penb, **kw) == eb


@pytest.mark.parametrize("family", ["qwen", "mllama"])
def test_penalties_make_the_reply_more_varied(device, family):
    eng, a, b, kw = _family(device, family)
    n = 60
    # the golden request `a`; should its unpenalised reply already be all-distinct, the other golden request is taken
    req = a
    base = eng.generate(*req, max_new_tokens=n, **kw)
    if len(set(base)) == len(base):
        req = b
        base = eng.generate(*req, max_new_tokens=n, **kw)
    pen = eng.generate(*req, max_new_tokens=n, frequency_penalty=2.0, presence_penalty=2.0, **kw)
    assert len(base) == n and len(pen) == n
    print(f"{family}: distinct tokens {len(set(base))} -> {len(set(pen))} of {n}")
    assert len(set(pen)) > len(set(base)), (len(set(pen)), len(set(base)))


@pytest.mark.parametrize("family", ["qwen", "mllama"])
def test_off_means_unchanged(device, monkeypatch, family):
    eng, a, b, kw = _family(device, family)
    kw = dict(kw, max_new_tokens=30)
    refs = {T: (eng.generate(*a, temperature=T, seed=2, **kw), eng.generate_batch([a, b], temperature=T, seed=2, **kw))
            for T in (0.0, 0.8)}
    # a penalised request first: the plain ones after it are back on the plain kernels
    eng.generate(*a, repetition_penalty=1.3, frequency_penalty=1.0, **kw)
    eng.generate_batch([a, b], presence_penalty=[1.0, 0.0], **kw)

    def boom(*args, **k):
        raise AssertionError("a penalty kernel launched with penalties off")
    monkeypatch.setattr(hip, "penalize", boom)
    monkeypatch.setattr(hip, "penalty_prompt", boom)
    for off in ({}, dict(repetition_penalty=None, frequency_penalty=None, presence_penalty=None),
                dict(repetition_penalty=1, frequency_penalty=0, presence_penalty=0),
                dict(repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)):
        for T in (0.0, 0.8):
            assert eng.generate(*a, temperature=T, seed=2, **off, **kw) == refs[T][0], (off, T)
            assert eng.generate_batch([a, b], temperature=T, seed=2, **off, **kw) == refs[T][1], (off, T)
    assert eng.generate_batch([a, b], repetition_penalty=[1, 1.0], presence_penalty=[0, None], **kw) == refs[0.0][1]


@pytest.mark.parametrize("family", ["qwen", "mllama"])
def test_composition_json_and_nucleus(device, family):
    from vision_inspection_system_amd import json_grammar as G
    eng, a, b, kw = _family(device, family)
    eos = set(eng.cfg.eos_ids)
    ended = 0
    for temp, seed in ((0.0, 0), (0.9, 1), (1.5, 2)):
        for use_graph in (False, True):
            toks = eng.generate(*a, max_new_tokens=60, temperature=temp, seed=seed, use_graph=use_graph, json_mode=True,
                                repetition_penalty=1.2)
            body = [t for t in toks if t not in eos]
            data = b"".join(eng._json.table.tokens[t] for t in body)
            if len(toks) < 60 or (toks and toks[-1] in eos):         # ended on EOS: a complete JSON object
                assert isinstance(json.loads(data.decode("utf-8")), dict), (temp, use_graph, data)
                ended += 1
            else:
                assert G.feed(data)[0] in ("progress", "done"), (temp, use_graph, data)
    print(f"{family}: {ended} of 6 JSON replies ended on EOS")
    # nucleus sampling with request seeds and penalties: repeatable, and independent of the slot
    skw = dict(kw, max_new_tokens=40, temperature=1.0, top_p=0.9, repetition_penalty=1.3, frequency_penalty=0.5)
    out = eng.generate_batch([a, b, a], seeds=[5, 9, 5], **skw)
    assert out[0] == out[2]
    assert eng.generate_batch([a, b, a], seeds=[5, 9, 5], **skw) == out
    re = eng.generate_batch([b, a, a], seeds=[9, 5, 5], **skw)
    assert re == [out[1], out[0], out[0]]
    assert eng.generate_batch([a, b, a], seeds=[5, 9, 5], use_graph=False, **skw) == out
    unpen = eng.generate_batch([a, b, a], seeds=[5, 9, 5], **dict(skw, repetition_penalty=None, frequency_penalty=None))
    assert unpen != out


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
def test_client_penalties(device, tmp_path, monkeypatch, model):
    from vision_inspection_system_amd.client import LocalVLMClient
    monkeypatch.setenv("VIS_IGNORE_EOS", "1")                # 24 tokens whatever the random weights pick
    monkeypatch.delenv("VIS_SYNTHETIC_REPLY", raising=False)
    c = LocalVLMClient()
    ma, mb = _msgs(tmp_path, 1), _msgs(tmp_path, 2)
    kw = dict(model=model, temperature=0.0, max_tokens=24)
    plain = c.chat.completions.create(messages=ma, logprobs=True, top_logprobs=3, **kw)
    p1 = c.chat.completions.create(messages=ma, repetition_penalty=1.3, frequency_penalty=0.5, **kw)
    p2 = c.chat.completions.create(messages=ma, repetition_penalty=1.3, frequency_penalty=0.5, **kw)
    assert p1.choices[0].message.content == p2.choices[0].message.content
    assert p1.choices[0].message.content != plain.choices[0].message.content
    assert p1.usage["completion_tokens"] == 24
    many = c.complete_many(model, [ma, mb, ma], temperature=0.0, max_tokens=24, repetition_penalty=1.3, frequency_penalty=0.5)
    assert many[0].choices[0].message.content == many[2].choices[0].message.content == p1.choices[0].message.content
    # text only (the mllama single-sequence path included)
    txt = [{"role": "user", "content": "Reply with OK."}]
    t1 = c.chat.completions.create(messages=txt, presence_penalty=2.0, frequency_penalty=2.0, **kw)
    t2 = c.chat.completions.create(messages=txt, presence_penalty=2.0, frequency_penalty=2.0, **kw)
    assert t1.choices[0].message.content == t2.choices[0].message.content
    # logprobs keep their raw-logit meaning.  Frequency / presence penalties leave the first pick alone (nothing has been
    # generated yet), so the first token is the same with and without them: its numbers agree.
    pen = c.chat.completions.create(messages=ma, logprobs=True, top_logprobs=3, frequency_penalty=2.0, presence_penalty=2.0,
                                    **kw)
    e1, e0 = pen.choices[0].logprobs.content[0], plain.choices[0].logprobs.content[0]
    assert e1.token == e0.token and e1.logprob == pytest.approx(e0.logprob, abs=1e-6)
    assert [t.token for t in e1.top_logprobs] == [t.token for t in e0.top_logprobs]
    for t1_, t0_ in zip(e1.top_logprobs, e0.top_logprobs):
        assert t1_.logprob == pytest.approx(t0_.logprob, abs=1e-6)
    # every later entry is still the log-softmax of the raw logits: a probability, whatever the penalty took off the logit
    assert all(e.logprob <= 1e-6 for e in pen.choices[0].logprobs.content)
