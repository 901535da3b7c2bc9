"""Speculative decoding of sampled requests on the GPU.  The kernel, vis_spec_accept_sampled: every row's pick against the token
vis_argmax_f32 stores for the same row, step and seed (bit for bit), against the float64 reference of tests/pick_exact.py, and
its bookkeeping against spec.accept_ref_sampled.  The engines and the client: a sampled request that speculates returns the
plain sampled reply token for token - all three weight formats, both engines, eager and replayed, with and without a
prediction."""
import numpy as np
import pytest
import torch

import spec_sampled_cases as C

pytestmark = pytest.mark.gpu

T_ROW = 1100      # token slots: the largest start is 1000


# ----------------------------------------------------------------------------------------------------------------- kernel
class _State:
    """The device ints of one accept launch."""

    def __init__(self, device, R, st, draft=(), d=None, limit=T_ROW - 1, counters=(5, 7, 3)):
        dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=device)      # noqa: E731
        self.tokens0 = np.arange(2000, 2000 + T_ROW, dtype=np.int32)
        self.draft = dev(list(draft) + [0] * (max(1, R - 1) - len(draft)))
        self.n_draft, self.limit = dev([len(draft) if d is None else d]), dev([limit])
        self.tokens, self.cur, self.step, self.counters = dev(self.tokens0), dev([-1]), dev([st]), dev(list(counters))
        self.ws_val = torch.empty(256 * R, dtype=torch.float32, device=device)
        self.ws_idx = torch.empty(256 * R, dtype=torch.int32, device=device)

    def launch(self, hip, logits, params):
        hip.spec_accept_sampled(logits, self.draft, self.n_draft, self.limit, self.ws_val, self.ws_idx, self.tokens, self.cur,
                                self.step, self.counters, params)
        return self.read()

    def read(self):
        return self.tokens.cpu().numpy(), int(self.cur.item()), int(self.step.item()), self.counters.cpu().tolist()


def _params(device, inv_temp, seed):
    return torch.from_numpy(C.params_words(inv_temp, seed)).to(device)


def _kernel_picks(hip, device, logits, st, params):
    """The kernel's own pick of every row: launch r plants the picks found so far as drafts, so row r's pick is stored."""
    picks = []
    for r in range(logits.shape[0]):
        tok, _, step, _ = _State(device, logits.shape[0], st, picks).launch(hip, logits, params)
        assert step == st + r + 1
        picks.append(int(tok[st + r]))
    return picks


def _argmax_token(hip, device, row, st, inv_temp, seed):
    """What vis_argmax_f32 (batch 1) stores for ``row`` at step ``st``."""
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device=device)      # noqa: E731
    tokens, cur, step = dev([-1] * T_ROW), dev([-1]), dev([st])
    ws_val, ws_idx = torch.empty(256, dtype=torch.float32, device=device), torch.empty(256, dtype=torch.int32, device=device)
    rc = hip.load().vis_argmax_f32(row.data_ptr(), row.numel(), ws_val.data_ptr(), ws_idx.data_ptr(), tokens.data_ptr(), T_ROW,
                                   cur.data_ptr(), step.data_ptr(), float(inv_temp), seed, 1, row.numel(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = int(tokens[st].item())
    assert int(cur.item()) == got and int(step.item()) == st + 1
    return got


@pytest.mark.parametrize("V", C.VS)
def test_picks_equal_vis_argmax_bit_for_bit(device, V):
    """Row r's pick == the token vis_argmax_f32 writes for the same logits row with step_ptr = st + r and the same seed: R =
    1..4, st in {0, 5, 1000}, inv_temp in {0, 0.5, 10}, seeds {0, 0xFFFFFFFF}; an all-NaN row and a planted tie among the rows;
    every second launch reads its rows at a stride of V + 5 with +inf in the padding.  The reference's drafts are planted, so
    the launch stores all R picks."""
    from vision_inspection_system_amd import hip
    rows = torch.tensor(C.diff_rows(V)).to(device)
    n = 0
    for inv_temp in C.INV_TEMPS:
        for seed in C.SEEDS:
            want = {}      # (row, step) -> vis_argmax_f32's token
            params = _params(device, inv_temp, seed)
            for st in C.STARTS:
                for R in (1, 2, 3, 4):
                    ids = C.diff_row_ids(R)
                    ref = []
                    for r, i in enumerate(ids):
                        if (i, st + r) not in want:
                            want[i, st + r] = _argmax_token(hip, device, rows[i], st + r, inv_temp, seed)
                        ref.append(want[i, st + r])
                    logits = rows[ids]
                    if n % 2:      # [R, V] at a row stride of V + 5
                        wide = torch.full((R, V + 5), float("inf"), dtype=torch.float32, device=device)
                        wide[:, :V] = logits
                        logits = wide[:, :V]
                    n += 1
                    tok, cur, step, cnt = _State(device, R, st, ref[:-1]).launch(hip, logits, params)
                    assert tok[st:st + R].tolist() == ref, (V, inv_temp, seed, st, R)
                    assert (cur, step, cnt) == (ref[-1], st + R, [6, 7 + R - 1, 3 + R - 1])
    # the rows did what they are there for: the NaN row picks id 0, the tie goes to the lower id at inv_temp 0
    assert _argmax_token(hip, device, rows[1], 5, 10.0, 0) == 0
    assert _argmax_token(hip, device, rows[0], 5, 0.0, 0) == min(3, V - 1)


@pytest.mark.parametrize("V", C.VS)
def test_picks_against_float64(device, V):
    """The table entries (tests/test_spec_sampled.py holds them against the ambiguity cap): a decisive draw is produced exactly,
    an ambiguous one lies among its candidates."""
    from vision_inspection_system_amd import hip
    for case in C.cases(V):
        logits = torch.tensor(case.logits).to(device)
        params = _params(device, case.inv_temp, case.seed)
        for st in C.STARTS:
            picks = _kernel_picks(hip, device, logits, st, params)
            for r, (got, cand) in enumerate(zip(picks, case.expected[st])):
                if cand.size == 1:
                    assert got == int(cand[0]), (case.name, st, r, case.kinds[r])
                else:
                    assert got in cand.tolist(), (case.name, st, r, case.kinds[r])


def test_bookkeeping_equals_accept_ref_sampled(device):
    """Planted drafts, right and wrong, draft counts short and too long, the limit inside the run and behind the step: tokens,
    cur_token, step_ptr and the counters equal spec.accept_ref_sampled on the kernel's own picks."""
    from vision_inspection_system_amd import hip, spec
    case = next(c for c in C.cases(4099) if c.R == 4 and c.inv_temp > 0)
    logits = torch.tensor(case.logits).to(device)
    params = _params(device, case.inv_temp, case.seed)
    st = 5
    picks = _kernel_picks(hip, device, logits, st, params)
    assert len(set(picks)) > 1
    wrong = lambda i: (picks[i] + 1) % case.V      # noqa: E731
    plans = [(picks[:3], None, T_ROW - 1), ([wrong(0), picks[1], picks[2]], None, T_ROW - 1),
             ([picks[0], wrong(1), picks[2]], None, T_ROW - 1), ([picks[0], picks[1], wrong(2)], None, T_ROW - 1),
             (picks[:3], 0, T_ROW - 1), (picks[:3], 2, T_ROW - 1), (picks[:3], 9, T_ROW - 1), (picks[:3], -4, T_ROW - 1),
             (picks[:3], None, st + 1), (picks[:3], None, st), (picks[:3], None, st - 1), (picks[:3], None, 10 ** 6)]
    for draft, d, limit in plans:
        s = _State(device, 4, st, draft, d, limit)
        got = s.launch(hip, logits, params)
        want = spec.accept_ref_sampled(picks, draft, len(draft) if d is None else d, st, limit, s.tokens0, [5, 7, 3])
        assert np.array_equal(got[0], want[0]), (draft, d, limit)
        assert got[1:] == (-1 if want[1] is None else want[1], want[2], want[3]), (draft, d, limit)
    # the limit clamps an accepted run; a step issued past the limit changes nothing at all
    s = _State(device, 4, st, picks[:3], None, st + 1)
    tok, cur, step, cnt = s.launch(hip, logits, params)
    assert (cur, step, cnt) == (picks[1], st + 2, [6, 10, 4]) and tok[st + 2] == s.tokens0[st + 2]
    tok, cur, step, cnt = s.launch(hip, logits, params)
    assert (cur, step, cnt) == (picks[1], st + 2, [6, 10, 4]) and np.array_equal(tok[st + 2:], s.tokens0[st + 2:])
    # R = 1: no drafts, one token
    one = _State(device, 1, st)
    tok, cur, step, cnt = one.launch(hip, logits[:1], params)
    assert (int(tok[st]), cur, step, cnt) == (picks[0], picks[0], st + 1, [6, 7, 3])


def test_params_are_read_when_the_launch_runs(device):
    """The same launch repeated after the 8 bytes changed picks accordingly: temperature and seed are no launch arguments."""
    from vision_inspection_system_amd import hip
    host = C.diff_rows(1000)[3:4]      # the Gaussian row of unit width: at inv_temp 0.5 the noise decides
    row = torch.tensor(host).to(device)
    params = _params(device, 0.0, 0)
    seen = {}
    for inv_temp, seed in ((0.0, 0), (0.5, 0), (0.5, 0xFFFFFFFF), (10.0, 0xFFFFFFFF), (0.0, 0xFFFFFFFF)):
        params.copy_(torch.from_numpy(C.params_words(inv_temp, seed)))
        s = _State(device, 1, 5)
        tok, _, _, _ = s.launch(hip, row, params)
        seen[inv_temp, seed] = int(tok[5])
        assert seen[inv_temp, seed] == _argmax_token(hip, device, row[0], 5, inv_temp, seed)
    assert seen[0.0, 0] == seen[0.0, 0xFFFFFFFF] == int(np.argmax(host[0]))      # inv_temp 0: vis_spec_accept's pick
    assert len(set(seen.values())) >= 3


def test_entry_refuses_bad_arguments(device):
    from vision_inspection_system_amd import hip
    lib = hip.load()
    P = 4096
    ok = [P, 1000, 1000, 2, P, P, P, P, P, P, 64, P, P, P, P, None]
    for at, bad in ((14, None), (14, P + 2), (0, None), (2, 999), (3, 5), (3, 0), (10, 0), (12, P + 1)):
        args = list(ok)
        args[at] = bad
        assert lib.vis_spec_accept_sampled(*args) == 1, (at, bad)
    z = torch.zeros(4, dtype=torch.int32, device=device)
    with pytest.raises(hip.HipLibraryError):      # params: two int32
        hip.spec_accept_sampled(torch.zeros((2, 8), device=device), z, z[:1], z[:1], torch.zeros(512, device=device),
                                torch.zeros(512, dtype=torch.int32, device=device), z, z[:1], z[:1], z[:3], z[:3])


# ---------------------------------------------------------------------------------------------------------------- engines
N_NEW = 24
PHRASE = [72, 105, 33, 116, 104, 101, 114, 101, 32, 119]
TEMPS = (0.1, 0.7, 1.5)
MODELS = ("tiny", "tiny25", "mllama-tiny")


@pytest.fixture(scope="module", params=MODELS)
def model(request, device):
    if request.param == "mllama-tiny":
        from vision_inspection_system_amd import mllama_weights as MW
        cfg = MW.MllamaConfig.tiny()
        return "mllama", cfg, MW.pack_device_weights(cfg, MW.synth_state_dict(cfg, 0), device)
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny() if request.param == "tiny" else Qwen2VLConfig.tiny_2_5()
    return "qwen", cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)


class _Eng:
    """One engine behind the one spelling the tests use: generate(prompt) with ignore-EOS, and its request."""

    def __init__(self, family, cfg, w, device, fmt, cross_kv="bf16"):
        self.family = family
        if family == "mllama":
            from vision_inspection_system_amd.mllama_engine import MllamaEngine
            self.e = MllamaEngine(cfg, w, device, max_ctx=256, decode_weights=fmt, cross_kv=cross_kv, speculative=True)
            frame = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (40, 56, 3), dtype=np.uint8)).to(device)
            self.ids, self.frames = [cfg.image_token_id, min(cfg.vocab - 1, 300)] + PHRASE * 4 + PHRASE[:4], frame
            self.kw = dict(stop_on_eos=False)
        else:
            from vision_inspection_system_amd.engine import Qwen2VLEngine
            self.e = Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_weights=fmt)
            self.ids, self.frames, self.kw = [256] + PHRASE * 5 + PHRASE[:4], [], dict(ignore_eos=True)

    def generate(self, **kw):
        return self.e.generate(self.ids, self.frames, max_new_tokens=N_NEW, **self.kw, **kw)


@pytest.fixture(scope="module", params=["bf16", "fp8", "mxfp4"])
def eng(request, model, device):
    return _Eng(*model, device, request.param)


def _spec(k):
    return {"method": "ngram", "num_speculative_tokens": k, "sampled": True}


@pytest.mark.parametrize("T", TEMPS)
def test_sampled_speculative_equals_sampled_plain(eng, T):
    """generate(temperature, seed, speculative={k, sampled}) == generate(temperature, seed), token for token: with a seed and
    without, k = 1..3, eager and replayed."""
    for seed in ({}, {"seed": 12345}):
        plain = eng.generate(temperature=T, **seed)
        fin = eng.e.last_finish
        assert len(plain) == N_NEW and "spec_steps" not in eng.e.last_timing
        for k in (1, 2, 3):
            for graph in (False, True):
                got = eng.generate(temperature=T, use_graph=graph, speculative=_spec(k), **seed)
                assert got == plain, (T, seed, k, graph)
                assert eng.e.last_finish == fin
                t = eng.e.last_timing
                assert t["spec_steps"] >= 1 and 0 <= t["spec_accepted"] <= t["spec_proposed"] <= k * t["spec_steps"]
        assert eng.generate(temperature=T, **seed) == plain      # nothing is left behind
    if T == TEMPS[0]:      # sampled=True on a greedy request is the greedy speculative request
        greedy = eng.generate()
        assert eng.generate(speculative=_spec(3)) == greedy == eng.generate(speculative=3)
        assert eng.generate(temperature=1.5, seed=1) != eng.generate(temperature=1.5, seed=2)      # the seed matters at all


@pytest.mark.parametrize("T", TEMPS)
def test_prediction_of_the_sampled_reply(eng, T):
    """prediction = the plain sampled reply of the same seed: the reply is equal and the counters are those of
    spec.simulate_prediction on it - every draft is the pick of the row in front of it only if row r draws at hash counter
    st + r.  Damaged at every 8th id: still the plain reply, counters still the simulation's."""
    from vision_inspection_system_amd import spec
    vocab = eng.e.cfg.vocab
    plain = eng.generate(temperature=T, seed=77)
    damaged = [(t + 1) % 490 if i % 8 == 7 else t for i, t in enumerate(plain)]
    names = ("spec_steps", "spec_proposed", "spec_accepted", "pred_accepted", "pred_rejected")
    for pred in (list(plain), damaged):
        for k, graph in ((3, True), (2, False), (1, True)):
            got = eng.generate(temperature=T, seed=77, use_graph=graph, speculative=_spec(k), prediction=pred)
            assert got == plain, (T, k, graph)
            sim = spec.simulate_prediction(plain, eng.ids, pred, k, 4, 2, N_NEW, vocab)
            assert {n: eng.e.last_timing[n] for n in names} == {n: sim[n] for n in names}, (T, k, graph)
    sim = spec.simulate_prediction(plain, eng.ids, list(plain), 3, 4, 2, N_NEW, vocab)
    assert sim["spec_accepted"] == N_NEW - 1 - sim["spec_steps"] and sim["spec_steps"] == -(-(N_NEW - 1) // 4)


def test_one_captured_graph_serves_every_temperature_and_seed(eng):
    """Temperature and seed are not in the graph key: the step captured for the first request is replayed for the second."""
    plains = {(T, s): eng.generate(temperature=T, seed=s) for T, s in ((0.7, 5), (1.5, 99))}
    assert plains[0.7, 5] != plains[1.5, 99]
    eng.e._spec_graphs.clear()
    for (T, s), plain in plains.items():
        damaged = [(t + 1) % 490 if i % 8 == 7 else t for i, t in enumerate(plain)]
        assert eng.generate(temperature=T, seed=s, speculative=_spec(3), prediction=damaged) == plain, (T, s)
        assert len(eng.e._spec_graphs) == 1
    (key,) = eng.e._spec_graphs
    assert "sampled" in key and 0.7 not in key and 1.5 not in key and 5 not in key and 99 not in key
    eng.generate(speculative=3, prediction=list(plains[0.7, 5]))      # the step that did not opt in keeps its own key
    assert len(eng.e._spec_graphs) == 2 and sum("sampled" in k for k in eng.e._spec_graphs) == 1


def test_mllama_fp8_cross_keys(device):
    """The second cross_kv format of the Auditor's engine (the accept is the only launch that differs)."""
    from vision_inspection_system_amd import mllama_weights as MW
    cfg = MW.MllamaConfig.tiny()
    e = _Eng("mllama", cfg, MW.pack_device_weights(cfg, MW.synth_state_dict(cfg, 0), device), device, "bf16", cross_kv="fp8")
    for T in (0.1, 1.5):
        plain = e.generate(temperature=T, seed=3)
        for k in (1, 3):
            assert e.generate(temperature=T, seed=3, speculative=_spec(k)) == plain
        assert e.generate(temperature=T, seed=3, speculative=_spec(3), prediction=list(plain)) == plain


def test_engines_still_refuse_without_the_opt_in(eng):
    with pytest.raises(ValueError, match="temperature"):
        eng.generate(temperature=0.7, speculative=2)
    with pytest.raises(ValueError, match="top_p"):
        eng.generate(temperature=0.7, speculative=_spec(2), top_p=0.9)


# ----------------------------------------------------------------------------------------------------------------- client
MSGS = [{"role": "user", "content": "list: alpha beta gamma; list: alpha beta gamma; list: alpha beta"}]


def _same(a, b):
    assert a.choices[0].message.content == b.choices[0].message.content
    assert a.choices[0].finish_reason == b.choices[0].finish_reason
    assert {n: v for n, v in a.usage.items() if n != "completion_tokens_details"} == b.usage


@pytest.mark.parametrize("model_id", ["synthetic:tiny", "synthetic:tiny25"])
def test_client_create_sampled_speculative(device, model_id):
    from vision_inspection_system_amd.client import LocalVLMClient, get_model
    c = LocalVLMClient()
    for kw in (dict(temperature=0.1, seed=7), dict(temperature=0.7), dict(temperature=1.5, seed=0)):
        plain = c.chat.completions.create(model=model_id, messages=MSGS, max_tokens=20, **kw)
        for k in (1, 3):
            sp = c.chat.completions.create(model=model_id, messages=MSGS, max_tokens=20, speculative=_spec(k), **kw)
            _same(sp, plain)
            assert sp.usage == plain.usage
        pr = c.chat.completions.create(model=model_id, messages=MSGS, max_tokens=20, speculative=_spec(3),
                                       prediction={"type": "content", "content": plain.choices[0].message.content}, **kw)
        _same(pr, plain)
        t = get_model(model_id).engine.last_timing
        assert pr.usage["completion_tokens_details"] == {"accepted_prediction_tokens": t["pred_accepted"],
                                                         "rejected_prediction_tokens": t["pred_rejected"]}
    with pytest.raises(ValueError, match="temperature"):
        c.chat.completions.create(model=model_id, messages=MSGS, max_tokens=20, temperature=0.7,
                                  speculative={"method": "ngram", "num_speculative_tokens": 2})


def test_client_create_sampled_speculative_auditor(device, monkeypatch):
    """The Auditor's model behind VIS_AUDITOR_SPECULATIVE (the engine built for speculative requests is cached under its own key)."""
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    model_id = "synthetic:mllama-tiny"
    monkeypatch.setenv("VIS_AUDITOR_SPECULATIVE", "2")
    for kw in (dict(temperature=0.2, seed=7), dict(temperature=0.7)):
        plain = c.chat.completions.create(model=model_id, messages=MSGS, max_tokens=20, **kw)
        sp = c.chat.completions.create(model=model_id, messages=MSGS, max_tokens=20, speculative=_spec(2), **kw)
        _same(sp, plain)
        assert sp.usage == plain.usage
