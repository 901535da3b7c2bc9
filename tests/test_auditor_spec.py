"""Speculative decoding on the Auditor, the parts that need no GPU: VIS_AUDITOR_SPECULATIVE and what it changes - the
constructor call, the engine cache key, what the clients and the agents accept for an mllama model - and that with the
variable unset everything is as it was: the same key, the same constructor call, the same refusals."""
import pytest

MODEL = "synthetic:mllama-tiny"
VAR = "VIS_AUDITOR_SPECULATIVE"
MSGS = [{"role": "user", "content": "hi"}]


class _FakeEngine:
    calls = []

    def __init__(self, *a, **kw):
        type(self).calls.append((a, kw))
        self.tokenizer = None


@pytest.fixture()
def loader(monkeypatch):
    from vision_inspection_system_amd import client, mllama_engine
    from vision_inspection_system_amd import mllama_weights as MW
    monkeypatch.setattr(mllama_engine, "MllamaEngine", _FakeEngine)
    monkeypatch.setattr(MW, "pack_device_weights", lambda cfg, sd, device: "weights")
    monkeypatch.setattr(MW, "synth_state_dict", lambda cfg, seed: {})
    for v in ("VIS_AUDITOR_DECODE_WEIGHTS", "VIS_AUDITOR_MXFP4_GEMM_FROM", "VIS_AUDITOR_CROSS_KV", VAR, "VIS_SPECULATIVE"):
        monkeypatch.delenv(v, raising=False)
    _FakeEngine.calls = []
    return client


def test_parsing_of_the_variable(monkeypatch):
    from vision_inspection_system_amd import spec
    monkeypatch.delenv(VAR, raising=False)
    assert spec.auditor_from_env() is None
    for off in ("", "0", "  ", " 0 "):
        monkeypatch.setenv(VAR, off)
        assert spec.auditor_from_env() is None
    for k in (1, 2, 3):
        monkeypatch.setenv(VAR, f" {k} ")
        assert spec.auditor_from_env() == spec.SpecConfig(k, 4, 2)
    for bad in ("4", "-1", "two", "1.5", "true", "00x"):
        monkeypatch.setenv(VAR, bad)
        with pytest.raises(ValueError, match=VAR):
            spec.auditor_from_env()
    # the Inspector's variable is another one
    monkeypatch.setenv(VAR, "2")
    monkeypatch.delenv("VIS_SPECULATIVE", raising=False)
    assert spec.from_env() is None
    monkeypatch.delenv(VAR)
    monkeypatch.setenv("VIS_SPECULATIVE", "3")
    assert spec.auditor_from_env() is None


def test_constructor_keywords_with_and_without_the_variable(loader, monkeypatch):
    assert loader._auditor_kwargs() == {}
    assert loader._auditor_settings() == ("bf16", None, "bf16")
    loader._load_mllama(MODEL, "cpu", 256, 3)
    (args, kw), = _FakeEngine.calls
    assert args[1:] == ("weights", "cpu") and kw == dict(max_ctx=256, max_batch=3)      # today's call
    monkeypatch.setenv(VAR, "2")
    assert loader._auditor_kwargs() == {"speculative": True}
    assert loader._auditor_settings() == ("bf16", None, "bf16")                          # a 3-tuple, untouched
    monkeypatch.setenv("VIS_AUDITOR_CROSS_KV", "fp8")
    assert loader._auditor_kwargs() == {"speculative": True, "cross_kv": "fp8"}
    loader._load_mllama(MODEL, "cpu", 256, 3)
    assert _FakeEngine.calls[-1][1] == dict(max_ctx=256, max_batch=3, cross_kv="fp8", speculative=True)
    monkeypatch.setenv(VAR, "0")
    assert loader._auditor_kwargs() == {"cross_kv": "fp8"}
    monkeypatch.setenv(VAR, "9")
    with pytest.raises(ValueError, match=VAR):
        loader._load_mllama(MODEL, "cpu", 256, 3)


def test_cache_key_distinct_when_set_and_todays_when_unset(loader, monkeypatch):
    loader.drop_models()
    try:
        a = loader.get_model(MODEL, "cpu")
        assert list(loader._ENGINES) == [(MODEL, "cpu", "bf16", None, "bf16")]          # today's key
        monkeypatch.setenv(VAR, "3")
        b = loader.get_model(MODEL, "cpu")
        assert b is not a and len(loader._ENGINES) == 2
        assert [kw.get("speculative") for _, kw in _FakeEngine.calls] == [None, True]
        assert loader.get_model(MODEL, "cpu") is b and loader.get_model(MODEL) is b      # no device named: the current settings' entry
        monkeypatch.setenv(VAR, "1")                                                      # k is the request's, not the engine's
        assert loader.get_model(MODEL, "cpu") is b
        monkeypatch.delenv(VAR)
        assert loader.get_model(MODEL, "cpu") is a and loader.get_model(MODEL) is a
        assert len(_FakeEngine.calls) == 2
    finally:
        loader.drop_models()


def test_default_engine_refuses_and_names_both_ways():
    """The class default and an object that never ran __init__ refuse; the text still names the Qwen2-VL engines and says how
    the Mllama engine is enabled.  A speculative= that is not a bool is refused before anything touches the device."""
    from vision_inspection_system_amd.generation import Generation
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig
    assert MllamaEngine.speculative_supported is False and Generation.speculative_supported is False
    e = object.__new__(MllamaEngine)
    e.max_ctx = 64
    for kw in (dict(speculative=2), dict(prediction=[1, 2, 3])):
        with pytest.raises(ValueError, match="Qwen2-VL") as ei:
            e.generate([1, 2, 3], None, max_new_tokens=4, **kw)
        assert "speculative=True" in str(ei.value) and VAR in str(ei.value)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="speculative"):
            MllamaEngine(MllamaConfig.tiny(), None, "cpu", speculative=bad)


def test_cross_rows_must_fit_the_mfma_columns():
    from types import SimpleNamespace
    from vision_inspection_system_amd import spec
    for heads, kv, rows in ((32, 8, 4), (2, 1, 4), (8, 1, 2), (7, 1, 2)):
        spec.check_cross_rows_fit(SimpleNamespace(heads=heads, kv_heads=kv), rows)
    for heads, kv, rows in ((16, 2, 3), (8, 1, 3), (7, 1, 3)):
        with pytest.raises(ValueError, match="16"):
            spec.check_cross_rows_fit(SimpleNamespace(heads=heads, kv_heads=kv), rows)


def test_clients_and_agents_follow_the_variable(monkeypatch):
    from vision_inspection_system_amd import agents
    from vision_inspection_system_amd.client import CannedResponseClient, LocalVLMClient
    sp = {"method": "ngram", "num_speculative_tokens": 1}
    pred = {"type": "content", "content": "x"}
    monkeypatch.delenv(VAR, raising=False)
    monkeypatch.delenv("VIS_SPECULATIVE", raising=False)
    local, canned = LocalVLMClient(), CannedResponseClient("OK")
    # unset: as today - refused before a model is loaded
    for kw in (dict(speculative=sp), dict(prediction=pred)):
        with pytest.raises(ValueError, match="Qwen2-VL"):
            local.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, **kw)
    with pytest.raises(ValueError, match="Qwen2-VL"):
        canned.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, prediction=pred)
    assert agents.speculative_kwargs(canned, MODEL, 0.0, {}) == {}
    monkeypatch.setenv("VIS_SPECULATIVE", "3")                      # the Qwen engines' switch does not reach an mllama model
    assert agents.speculative_kwargs(canned, MODEL, 0.0, {}) == {}
    assert agents.speculative_kwargs(canned, "synthetic:tiny", 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 3}}
    # set: the canned client takes both, the agents pass k under the exclusions
    monkeypatch.setenv(VAR, "2")
    assert canned.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, prediction=pred).choices[0].message.content == "OK"
    assert canned.calls[-1]["prediction"] == pred
    canned.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, speculative=sp)
    assert canned.calls[-1]["speculative"] == sp
    assert agents.speculative_kwargs(canned, MODEL, 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 2}}
    assert agents.speculative_kwargs(local, MODEL, 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 2}}
    assert agents.speculative_kwargs(canned, MODEL, 0.2, {}) == {}
    assert agents.speculative_kwargs(canned, MODEL, 0.0, {"stop": ["x"]}) == {}
    assert agents.speculative_kwargs(object(), MODEL, 0.0, {}) == {}
    assert agents.speculative_kwargs(canned, "synthetic:tiny", 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 3}}
    monkeypatch.delenv("VIS_SPECULATIVE")
    assert agents.speculative_kwargs(canned, "synthetic:tiny", 0.0, {}) == {}
    # what a speculative request excludes stays excluded, and a batch stays refused
    with pytest.raises(ValueError, match="temperature"):
        canned.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, temperature=0.5, speculative=sp)
    with pytest.raises(ValueError, match="stop"):
        local.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, speculative=sp, stop=["x"])
    with pytest.raises(ValueError):
        local.complete_many(MODEL, [MSGS], max_tokens=4, prediction=pred)
    monkeypatch.setenv(VAR, "7")
    with pytest.raises(ValueError, match=VAR):
        canned.chat.completions.create(model=MODEL, messages=MSGS, max_tokens=4, prediction=pred)
