"""Speculative decoding of a batch, the parts that need no GPU: the engine setting and the environment variable, the client's
cache keys, the eligibility predicate and the model-free walk the GPU tests compare the counters with."""
import pytest

from vision_inspection_system_amd import client as CL, spec, spec_batch
from vision_inspection_system_amd.config import Qwen2VLConfig
from vision_inspection_system_amd.engine import Qwen2VLEngine
from vision_inspection_system_amd.mllama_engine import MllamaEngine


# ----------------------------------------------------------------------------------------------------------- the setting
def test_check_setting_reads_k_or_a_dict_and_refuses_grammar():
    assert spec_batch.check_setting(None) is None
    assert spec_batch.check_setting(2) == spec.SpecConfig(2, 4, 2)
    cfg = spec_batch.check_setting({"num_speculative_tokens": 3, "prompt_lookup_max": 5, "prompt_lookup_min": 1, "sampled": True})
    assert (cfg.k, cfg.rows, cfg.lookup_max, cfg.lookup_min, cfg.sampled) == (3, 4, 5, 1, True)
    for bad in (0, 4, True, "2", {"num_speculative_tokens": 9}, {"method": "eagle", "num_speculative_tokens": 1}):
        with pytest.raises(ValueError):
            spec_batch.check_setting(bad)
    with pytest.raises(ValueError, match="grammar"):
        spec_batch.check_setting({"num_speculative_tokens": 2, "grammar": True})


def test_the_constructors_check_the_setting_before_anything_else():
    """Both refusals come before the GPU is asked for: k out of range and the grammar key on the Qwen2-VL engine, the keyword
    itself on the Mllama engine.  A default engine has no instance attribute of that name."""
    cfg = Qwen2VLConfig.tiny()
    for bad in (4, 0, {"num_speculative_tokens": 2, "grammar": True}):
        with pytest.raises(ValueError, match="speculative|grammar"):
            Qwen2VLEngine(cfg, None, "cuda:0", batch_speculative=bad)
    from vision_inspection_system_amd.mllama_weights import MllamaConfig
    with pytest.raises(ValueError, match="batch_speculative"):
        MllamaEngine(MllamaConfig.tiny(), None, "cuda:0", batch_speculative=2)
    assert Qwen2VLEngine.batch_speculative is None and MllamaEngine.batch_speculative is None
    eng = Qwen2VLEngine.__new__(Qwen2VLEngine)
    assert "batch_speculative" not in vars(eng) and eng.batch_speculative is None and eng._spec_batch is None


def test_from_env(monkeypatch):
    for unset in (None, "", "0", " 0 "):
        if unset is None:
            monkeypatch.delenv("VIS_SPECULATIVE_BATCH", raising=False)
        else:
            monkeypatch.setenv("VIS_SPECULATIVE_BATCH", unset)
        assert spec_batch.from_env() is None
    for k in (1, 2, 3):
        monkeypatch.setenv("VIS_SPECULATIVE_BATCH", str(k))
        assert spec_batch.from_env() == spec.SpecConfig(k, 4, 2)
    monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", "1")
    assert spec_batch.from_env() == spec.SpecConfig(3, 4, 2, True) and spec_batch.from_env().sampled
    monkeypatch.delenv("VIS_SPECULATIVE_SAMPLED")
    for bad in ("4", "-1", "two", "1.5"):
        monkeypatch.setenv("VIS_SPECULATIVE_BATCH", bad)
        with pytest.raises(ValueError, match="VIS_SPECULATIVE_BATCH"):
            spec_batch.from_env()
    monkeypatch.setenv("VIS_SPECULATIVE", "2")      # the single request's variable is another one
    monkeypatch.delenv("VIS_SPECULATIVE_BATCH")
    assert spec_batch.from_env() is None


# ------------------------------------------------------------------------------------------------------------ the client
class _FakeEngine:
    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw
        self.batch_speculative = kw.get("batch_speculative")
        self.tokenizer = None


@pytest.fixture
def fake_load(monkeypatch):
    """get_model with the engine, the weights and the device query replaced: what it would build and where it keeps it."""
    import torch
    from vision_inspection_system_amd import engine as E, weights as W
    monkeypatch.setattr(E, "Qwen2VLEngine", _FakeEngine)
    monkeypatch.setattr(W, "pack_device_weights", lambda cfg, sd, device: "weights")
    monkeypatch.setattr(W, "synth_state_dict", lambda cfg, seed: {})
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(CL, "_ENGINES", {})
    for name in ("VIS_SPECULATIVE_BATCH", "VIS_SPECULATIVE_SAMPLED"):
        monkeypatch.delenv(name, raising=False)
    return CL._ENGINES


def test_client_keys_and_constructor_call_are_unchanged_without_the_variable(fake_load):
    lm = CL.get_model("synthetic:tiny", "cuda:0")
    assert list(fake_load) == [("synthetic:tiny", "cuda:0")]
    assert sorted(lm.engine.kw) == ["decode_weights", "max_batch", "max_ctx", "mxfp4_gemm_from", "prefill_dtype"]
    assert CL.get_model("synthetic:tiny", "cuda:0") is lm and CL.get_model("synthetic:tiny") is lm


def test_client_builds_the_engine_with_the_setting_under_a_key_of_its_own(fake_load, monkeypatch):
    plain = CL.get_model("synthetic:tiny", "cuda:0")
    monkeypatch.setenv("VIS_SPECULATIVE_BATCH", "2")
    lm = CL.get_model("synthetic:tiny", "cuda:0")
    assert lm is not plain and lm.engine.kw["batch_speculative"] == spec.SpecConfig(2, 4, 2)
    assert set(fake_load) == {("synthetic:tiny", "cuda:0"), ("batch_speculative", "synthetic:tiny", "cuda:0", 2, 4, 2)}
    assert CL.get_model("synthetic:tiny", "cuda:0") is lm and CL.get_model("synthetic:tiny") is lm
    monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", "1")
    sampled = CL.get_model("synthetic:tiny", "cuda:0")
    assert sampled is not lm and sampled.engine.kw["batch_speculative"].sampled and len(fake_load) == 3
    monkeypatch.delenv("VIS_SPECULATIVE_SAMPLED")
    monkeypatch.delenv("VIS_SPECULATIVE_BATCH")
    assert CL.get_model("synthetic:tiny", "cuda:0") is plain
    monkeypatch.setenv("VIS_SPECULATIVE_BATCH", "7")
    with pytest.raises(ValueError, match="VIS_SPECULATIVE_BATCH"):
        CL.get_model("synthetic:tiny", "cuda:0")
    monkeypatch.delenv("VIS_SPECULATIVE_BATCH")
    CL.unregister_model("synthetic:tiny", "cuda:0")
    assert not fake_load


def test_complete_many_and_generate_batch_still_refuse_the_keyword():
    with pytest.raises(TypeError, match="speculative"):
        Qwen2VLEngine.__new__(Qwen2VLEngine).generate_batch([([1, 2, 3], None)], speculative=2)


# ------------------------------------------------------------------------------------------------------- the predicate
def test_eligible_is_the_conjunction_the_issue_names():
    ok = dict(n_req=4, n_live=4, rows=4, max_batch=64, plain_step="streamk", attn_streams=False, switches=[], temperature=0.0,
              sampled=False)
    assert spec_batch.eligible(**ok)
    for change in (dict(n_live=3), dict(n_req=1, n_live=1), dict(n_req=17, n_live=17), dict(max_batch=15),
                   dict(plain_step="rows"), dict(plain_step="fused"), dict(attn_streams=True), dict(switches=["top_p"]),
                   dict(temperature=0.7)):
        assert not spec_batch.eligible(**{**ok, **change}), change
    assert spec_batch.eligible(**{**ok, "n_req": 16, "n_live": 16})                  # 64 rows
    assert spec_batch.eligible(**{**ok, "max_batch": 16})                            # B * R == max_batch
    assert spec_batch.eligible(**{**ok, "n_req": 32, "n_live": 32, "rows": 2})
    assert spec_batch.eligible(**{**ok, "temperature": 0.7, "sampled": True})
    assert spec_batch.eligible(**{**ok, "n_req": 2, "n_live": 2})


class _Pick:      # the flags of pick.PickStage a group switches on
    lp_k, json_on, schema_on, top_p, pen_on, shape_on, ban_on, stop_on, stream_on = None, False, False, None, False, False, False, False, False


def test_switches_on_names_what_the_group_switched_on():
    e = _Pick()
    assert spec_batch.switches_on(e, None) == []
    e.top_p, e.stop_on, e.lp_k = 0.9, True, 0
    assert spec_batch.switches_on(e, [2, 1]) == ["logprobs", "top_p", "stop", "n"]


# ------------------------------------------------------------------------------------------------------------- the walk
def test_simulate_walks_the_steps_of_one_sequence():
    prompt = [1, 2, 3, 4, 1, 2, 3, 4, 1, 2]
    plain = [3, 4, 1, 2, 3, 9, 9, 9]
    w = spec_batch.simulate(plain, prompt, 3)
    # behind the prompt pass: history ..1 2 | 3 -> draft [4, 1, 2]: accepted 3 (reply 5 tokens); then [3, 4, 1] -> the 9
    # rejects at once; then lookups over .. 9 / 9 9: nothing matches twice in a row
    assert w["reply"] == plain and w["spec_steps"] == 4 and w["spec_accepted"] == 3 and w["spec_proposed"] >= 6
    cut = spec_batch.simulate(plain, prompt, 3, max_new_tokens=3)      # the limit cuts the first step's run
    assert cut == {"reply": plain[:3], "spec_steps": 1, "spec_proposed": 3, "spec_accepted": 1}
    none = spec_batch.simulate(plain, [7, 8], 3)
    assert none["spec_accepted"] <= none["spec_proposed"] and none["reply"] == plain
    assert spec_batch.simulate(plain, prompt, 1)["spec_steps"] > w["spec_steps"]
