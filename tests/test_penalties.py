"""Repetition, frequency and presence penalties, the parts that need no GPU: the float64 reference against transformers'
RepetitionPenaltyLogitsProcessor and OpenAI's formula, the argument checks of the checkers, the client (before any model is
loaded), the engines, the vis_penalize_f32 / vis_penalty_prompt launchers (before any HIP call) and the agents' switch."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETRY_SUBSTRINGS = ("429", "rate", "413", "payload")


@pytest.fixture(scope="module")
def lib():
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    from vision_inspection_system_amd import hip
    return hip.load()


def _row(rng, V):
    """Logits of both signs with exact zeros planted."""
    x = rng.normal(0, 4, V).astype(np.float32)
    x[rng.choice(V, V // 10, replace=False)] = 0.0
    return x


@pytest.mark.parametrize("r", [0.8, 1.05, 1.3, 2.0])
def test_reference_equals_transformers_repetition_penalty(r):
    import torch
    from transformers import RepetitionPenaltyLogitsProcessor
    from vision_inspection_system_amd.penalties import penalize_ref
    rng = np.random.default_rng(int(r * 100))
    V = 500
    proc = RepetitionPenaltyLogitsProcessor(r)
    for n_ids in (1, 7, 60, 900):
        x = _row(rng, V)
        ids = rng.integers(0, V, n_ids)
        ids[n_ids // 2:] = ids[:n_ids - n_ids // 2]          # repeated ids
        ids[0] = int(np.flatnonzero(x == 0)[0])               # a zero logit, a negative and a positive one among them
        if n_ids > 2:
            ids[1], ids[2] = int(np.flatnonzero(x < 0)[0]), int(np.flatnonzero(x > 0)[0])
        want = proc(torch.from_numpy(ids[None].astype(np.int64)), torch.from_numpy(x[None].copy()))[0].numpy()
        # transformers has one id list (prompt + generated): either part of ours must give its result
        for split in (0, n_ids // 3, n_ids):
            got = penalize_ref(x, ids[:split], ids[split:], r, 0.0, 0.0)
            np.testing.assert_allclose(got, want.astype(np.float64), rtol=1e-6, atol=0)
            untouched = np.ones(V, bool)
            untouched[ids] = False
            assert (got[untouched] == x[untouched]).all()


def test_transformers_refuses_what_we_refuse():
    from transformers import RepetitionPenaltyLogitsProcessor
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            RepetitionPenaltyLogitsProcessor(bad)


def test_reference_equals_openai_formula():
    from vision_inspection_system_amd.penalties import penalize_ref
    rng = np.random.default_rng(5)
    V = 300
    for f, q in ((0.5, 0.0), (0.0, 1.5), (2.0, 2.0), (-1.0, 0.25), (0.0, 0.0)):
        x = _row(rng, V)
        prompt = rng.integers(0, V, 40)
        gen = rng.integers(0, V, 50)
        gen[25:] = gen[:25][::-1]
        gen[3] = prompt[0]                                    # a generated token that is also in the prompt
        counts = {}
        for t in gen.tolist():
            counts[t] = counts.get(t, 0) + 1
        f32, q32 = float(np.float32(f)), float(np.float32(q))
        want = np.array([float(x[v]) - f32 * counts.get(v, 0) - (q32 if counts.get(v, 0) > 0 else 0.0) for v in range(V)])
        got = penalize_ref(x, prompt, gen, 1.0, f, q)
        np.testing.assert_array_equal(got, want)
        # prompt ids do not enter c
        only_prompt = [int(t) for t in prompt if int(t) not in counts]
        assert only_prompt and (got[only_prompt] == x[only_prompt]).all()
        np.testing.assert_array_equal(penalize_ref(x, [], gen, 1.0, f, q), got)
    # all three, in order: repetition first, then frequency and presence; ids outside [0, V) ignored
    x = np.array([2.0, -2.0, 0.0, 4.0, 1.0])
    got = penalize_ref(x, [0, 5, -1, 99], [1, 1, 3, 7], 2.0, 0.5, 0.25)
    np.testing.assert_array_equal(got, [1.0, -4.0 - 1.0 - 0.25, 0.0, 2.0 - 0.5 - 0.25, 1.0])


def test_checkers():
    from vision_inspection_system_amd import penalties as P
    assert P.check_repetition_penalty(None) is None and P.check_repetition_penalty(1) == 1.0
    assert P.check_repetition_penalty(np.float32(1.5)) == 1.5 and P.check_repetition_penalty(0.01) == 0.01
    for bad in (0, 0.0, -1.3, float("nan"), float("inf"), True, "1.1", [1.1]):
        with pytest.raises(ValueError):
            P.check_repetition_penalty(bad)
    for chk in (P.check_frequency_penalty, P.check_presence_penalty):
        assert chk(None) is None and chk(0) == 0.0 and chk(-2) == -2.0 and chk(2.0) == 2.0 and chk(np.float64(0.5)) == 0.5
        for bad in (2.5, -2.01, float("nan"), float("inf"), True, "0.5"):
            with pytest.raises(ValueError) as e:
                chk(bad)
            assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS)
    # per request: a number for all, or one value per request; off = None
    assert P.check_penalties(None, None, None, 3) is None
    assert P.check_penalties(1, 0, 0.0, 3) is None and P.check_penalties([1, None, 1.0], None, [0, 0, 0], 3) is None
    assert P.check_penalties(1.3, None, None, 2) == [(1.3, 0.0, 0.0)] * 2
    assert P.check_penalties([1.3, 1], 0.5, [None, 1.5], 2) == [(1.3, 0.5, 0.0), (1.0, 0.5, 1.5)]
    for bad in (dict(r=[1.3]), dict(r=[1.3, 1, 1]), dict(f=[0.5, 0.5, 0.5]), dict(q=[0.1]), dict(r=[1.3, 0]), dict(f=[0.5, 3]),
                dict(q=[True, 0]), dict(r="12")):
        with pytest.raises(ValueError) as e:
            P.check_penalties(bad.get("r"), bad.get("f"), bad.get("q"), 2)
        assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS)


BAD_ARGS = [dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
            dict(repetition_penalty=float("inf")), dict(repetition_penalty=True), dict(repetition_penalty="1.1"),
            dict(frequency_penalty=2.5), dict(frequency_penalty=float("nan")), dict(frequency_penalty=True),
            dict(presence_penalty=2.5), dict(presence_penalty=float("nan")), dict(presence_penalty=True)]


@pytest.mark.parametrize("kw", BAD_ARGS)
def test_client_rejects_bad_penalties_before_loading(kw):
    from vision_inspection_system_amd import client as C
    c = C.LocalVLMClient()
    # a model id that does not exist: a check after loading would raise FileNotFoundError instead
    with pytest.raises(ValueError) as e:
        c.chat.completions.create(model="/nonexistent/model-dir", messages=[{"role": "user", "content": "hi"}],
                                  max_tokens=4, **kw)
    assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS), str(e.value)
    with pytest.raises(ValueError) as e:
        c.complete_many("/nonexistent/model-dir", [[{"role": "user", "content": "hi"}]], 0.0, 4, **kw)
    assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS)


@pytest.mark.parametrize("engine_mod,cls", [("engine", "Qwen2VLEngine"), ("mllama_engine", "MllamaEngine")])
def test_engines_check_penalties_first(engine_mod, cls):
    import importlib
    E = getattr(importlib.import_module(f"vision_inspection_system_amd.{engine_mod}"), cls)
    eng = E.__new__(E)           # no device state: the checks run before anything touches the GPU
    eng.max_batch = 4
    reqs = [([1, 2], None), ([3, 4], None)]
    for bad in (dict(repetition_penalty=0), dict(repetition_penalty=[1.1]), dict(repetition_penalty=[1.1, 1.2, 1.3]),
                dict(frequency_penalty=[0.5, 2.5]), dict(presence_penalty=True), dict(presence_penalty=[0.1])):
        with pytest.raises(ValueError):
            eng.generate_batch(reqs, **bad)
    for bad in (dict(repetition_penalty=-1), dict(frequency_penalty=float("nan")), dict(presence_penalty="1")):
        with pytest.raises(ValueError):
            eng.generate([1, 2], **bad)


def test_library_exports_and_launchers_reject_bad_arguments_without_gpu(lib):
    from vision_inspection_system_amd import hip
    for name in ("vis_penalty_state_bytes", "vis_penalty_prompt", "vis_penalize_f32"):
        assert name in hip.exported_symbols()
    V, B = 152064, 4
    one = int(lib.vis_penalty_state_bytes(V, 1))
    assert one == 16 + 2 * V and one % 16 == 0 and lib.vis_penalty_state_bytes(V, B) == B * one
    assert lib.vis_penalty_state_bytes(1000, 1) == 16 + 2 * 1000 and lib.vis_penalty_state_bytes(1001, 1) == 16 + 2 * 1008
    assert lib.vis_penalty_state_bytes(0, 1) == 0 and lib.vis_penalty_state_bytes(V, 65) == 0
    assert lib.vis_penalty_state_bytes(V, 0) == 0 and lib.vis_penalty_state_bytes(262145, 1) == 0
    p = 4096     # any non-null address: nothing is launched when an argument is refused

    def call(logits=p, V=V, ld=V, state=p, params=p, tokens=p, T=64, step=p, out=2 * p, ld_out=V, batch=B):
        return lib.vis_penalize_f32(logits, V, ld, state, params, tokens, T, step, out, ld_out, batch, None)
    for bad in (dict(logits=None), dict(state=None), dict(params=None), dict(tokens=None), dict(step=None), dict(out=None),
                dict(V=0), dict(V=-1), dict(V=262145), dict(batch=0), dict(batch=65), dict(ld=V - 1), dict(ld_out=V - 1),
                dict(batch=2, ld_out=V - 1), dict(T=0), dict(state=p + 8), dict(out=p)):
        assert call(**bad) == 1, bad

    def prompt(state=p, V=V, ids=p, n=10):
        return lib.vis_penalty_prompt(state, V, ids, n, None)
    for bad in (dict(state=None), dict(ids=None), dict(V=0), dict(V=262145), dict(n=-1), dict(state=p + 4)):
        assert prompt(**bad) == 1, bad
    assert prompt(n=0) == 0      # nothing to mark: no launch


def test_canned_client_records_only_the_penalties_given():
    from vision_inspection_system_amd.client import CannedResponseClient
    c = CannedResponseClient("OK")
    c.chat.completions.create(model="m", messages=[], top_p=0.9, seed=7)
    assert set(c.calls[0]) == {"model", "messages", "temperature", "max_tokens", "response_format", "top_p", "seed"}
    c.chat.completions.create(model="m", messages=[], repetition_penalty=1.05)
    assert c.calls[1]["repetition_penalty"] == 1.05 and "frequency_penalty" not in c.calls[1]
    c.chat.completions.create(model="m", messages=[], frequency_penalty=0.5, presence_penalty=-1)
    assert c.calls[2]["frequency_penalty"] == 0.5 and c.calls[2]["presence_penalty"] == -1
    assert "repetition_penalty" not in c.calls[2]


def test_agents_repetition_penalty_switch(monkeypatch):
    from vision_inspection_system_amd import agents
    from vision_inspection_system_amd.client import CannedResponseClient
    monkeypatch.delenv("VIS_REPETITION_PENALTY", raising=False)
    assert agents.penalty_kwargs() == {}
    monkeypatch.setenv("VIS_REPETITION_PENALTY", "")
    assert agents.penalty_kwargs() == {}
    monkeypatch.setenv("VIS_REPETITION_PENALTY", "1.05")
    assert agents.penalty_kwargs() == {"repetition_penalty": 1.05}
    monkeypatch.setenv("VIS_REPETITION_PENALTY", "x")
    with pytest.raises(ValueError):
        agents.penalty_kwargs()
    records = {}
    for env in (None, "1.05"):
        if env is None:
            monkeypatch.delenv("VIS_REPETITION_PENALTY", raising=False)
        else:
            monkeypatch.setenv("VIS_REPETITION_PENALTY", env)
        agent = agents.VLMInspectorAgent.__new__(agents.VLMInspectorAgent)
        agent.client, agent.model_id, agent.temperature, agent.max_tokens = CannedResponseClient(reply="{}"), "m", 0.1, 64
        agent.logger = agents._logger("t")
        msgs = [{"role": "user", "content": "x"}]
        assert agent._call_with_retry(msgs) == "{}"
        records[env] = agent.client.calls[-1]
    assert records["1.05"]["repetition_penalty"] == 1.05
    # unset: the recorded call is what it is without the feature
    assert records[None] == {"model": "m", "messages": msgs, "temperature": 0.1, "max_tokens": 64, "response_format": None,
                             "top_p": None, "seed": None}
