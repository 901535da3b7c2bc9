"""Speculative decoding of sampled requests without a GPU: the opt-in (``"sampled": True`` / VIS_SPECULATIVE_SAMPLED) and what it
does and does not relax, the agents' and the clients' side of it, the accept walk over given picks, the off state of the
speculative step, and the input tables of tests/test_spec_sampled_gpu.py held against the cap that test relies on."""
import types

import numpy as np
import pytest

import spec_sampled_cases as C
from pick_exact import AMBIGUOUS_CAP, candidates, noise_u, perturbed

SPEC = {"method": "ngram", "num_speculative_tokens": 2}
SAMPLED = {**SPEC, "sampled": True}
MSGS = [{"role": "user", "content": "hello"}]


# ------------------------------------------------------------------------------------------------------------ the opt-in
def test_check_speculative_parses_sampled():
    from vision_inspection_system_amd.spec import SpecConfig, check_speculative
    assert check_speculative(SAMPLED) == SpecConfig(2, 4, 2, True) and check_speculative(SAMPLED).sampled is True
    assert check_speculative({**SPEC, "sampled": False}) == SpecConfig(2, 4, 2) and check_speculative(SPEC).sampled is False
    assert check_speculative(2).sampled is False
    assert SpecConfig(2, 4, 2, True) != SpecConfig(2, 4, 2) == SpecConfig(2, 4, 2, False)
    assert check_speculative(SpecConfig(3, 5, 1, True)) == SpecConfig(3, 5, 1, True)      # the opt-in survives a second reading
    c = SpecConfig(3, 5, 1, True)
    assert (c.k, c.lookup_max, c.lookup_min, c.sampled, c.rows) == (3, 5, 1, True, 4)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="sampled"):
            check_speculative({**SPEC, "sampled": bad})


def test_env_switch(monkeypatch):
    from vision_inspection_system_amd.spec import SpecConfig, auditor_from_env, from_env
    monkeypatch.setenv("VIS_SPECULATIVE", "2")
    monkeypatch.setenv("VIS_AUDITOR_SPECULATIVE", "3")
    for off in (None, "", "0"):
        if off is None:
            monkeypatch.delenv("VIS_SPECULATIVE_SAMPLED", raising=False)
        else:
            monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", off)
        assert from_env() == SpecConfig(2, 4, 2) and from_env().sampled is False
        assert auditor_from_env() == SpecConfig(3, 4, 2) and auditor_from_env().sampled is False
    monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", "1")
    assert from_env() == SpecConfig(2, 4, 2, True) and auditor_from_env() == SpecConfig(3, 4, 2, True)
    monkeypatch.setenv("VIS_SPECULATIVE", "0")
    assert from_env() is None      # the switch alone turns nothing on
    for bad in ("2", "true", "-1", "on"):
        monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", bad)
        with pytest.raises(ValueError, match="VIS_SPECULATIVE_SAMPLED"):
            from_env()
        with pytest.raises(ValueError, match="VIS_SPECULATIVE_SAMPLED"):
            auditor_from_env()


def test_check_exclusive_lets_temperature_and_seed_through_only_with_the_opt_in():
    from vision_inspection_system_amd.spec import check_exclusive, check_speculative, with_prediction
    on, off = check_speculative(SAMPLED), check_speculative(SPEC)
    check_exclusive(on, 0.7, 3)
    check_exclusive(on, 0.1, None)
    check_exclusive(on, 0.0, 7)
    check_exclusive(on, 0.0, None)      # on a greedy request: the greedy speculative request
    with pytest.raises(ValueError, match="temperature > 0 is not supported: acceptance is defined for the greedy pick"):
        check_exclusive(off, 0.7, None)
    with pytest.raises(ValueError, match="together with a seed is not supported"):
        check_exclusive(off, 0.0, 3)
    # a prediction alone stays greedy-only; next to the opt-in it may sample
    with pytest.raises(ValueError, match="temperature"):
        check_exclusive(with_prediction(None, True), 0.7, None, what="prediction (speculative decoding)")
    check_exclusive(with_prediction(SAMPLED, True), 0.7, 3, what="prediction (speculative decoding)")
    assert with_prediction(None, True).sampled is False


REST = [("top_p", 0.9), ("repetition_penalty", 1.1), ("frequency_penalty", 0.5), ("presence_penalty", 0.5), ("top_k", 5),
        ("min_p", 0.1), ("logit_bias", {5: -100.0}), ("no_repeat_ngram_size", 3), ("bad_words", ["foo"]), ("min_tokens", 2),
        ("json_mode", True), ("json_schema", object()), ("stop", ["\n"]), ("stream", True), ("on_stream", object()),
        ("logprobs", 0), ("n", 2), ("seeds", [1])]


@pytest.mark.parametrize("name,value", REST, ids=[r[0] for r in REST])
def test_check_exclusive_still_names_the_rest(name, value):
    from vision_inspection_system_amd.spec import check_exclusive, check_speculative
    msg = f"speculative together with {name} is not supported: it is a per-step state of the pick"
    for cfg in (check_speculative(SAMPLED), check_speculative(SPEC)):
        with pytest.raises(ValueError, match=msg):
            check_exclusive(cfg, 0.0, None, **{name: value})
    with pytest.raises(ValueError, match=msg):
        check_exclusive(check_speculative(SAMPLED), 0.7, 3, **{name: value})


# ------------------------------------------------------------------------------------------------------------ agents
def test_agents_pass_the_opt_in(monkeypatch):
    from vision_inspection_system_amd.agents import speculative_kwargs
    from vision_inspection_system_amd.client import CannedResponseClient
    c = CannedResponseClient()
    monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", "1")
    assert speculative_kwargs(c, "synthetic:tiny", 0.1, {}) == {}      # next to nothing it is nothing
    monkeypatch.setenv("VIS_SPECULATIVE", "3")
    want = {"speculative": {"method": "ngram", "num_speculative_tokens": 3, "sampled": True}}
    assert speculative_kwargs(c, "synthetic:tiny", 0.1, {}) == want
    assert speculative_kwargs(c, "synthetic:tiny", 0.0, {}) == want
    assert speculative_kwargs(c, "synthetic:tiny", 0.1, {"seed": 3}) == want
    assert speculative_kwargs(c, "synthetic:tiny", 0.1, {"stop": ["x"]}) == {}
    assert speculative_kwargs(c, "synthetic:tiny", 0.1, {"seed": 3, "top_p": 0.9}) == {}
    assert speculative_kwargs(object(), "synthetic:tiny", 0.1, {}) == {}
    assert speculative_kwargs(c, "synthetic:mllama-tiny", 0.2, {}) == {}      # the Auditor has its own k
    monkeypatch.setenv("VIS_AUDITOR_SPECULATIVE", "2")
    assert speculative_kwargs(c, "synthetic:mllama-tiny", 0.2, {"seed": 1}) == \
        {"speculative": {"method": "ngram", "num_speculative_tokens": 2, "sampled": True}}
    # without the new variable every return value is the one of before
    monkeypatch.delenv("VIS_SPECULATIVE_SAMPLED")
    assert speculative_kwargs(c, "synthetic:tiny", 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 3}}
    assert speculative_kwargs(c, "synthetic:tiny", 0.1, {}) == {}
    assert speculative_kwargs(c, "synthetic:tiny", 0.0, {"seed": 3}) == {}


# ------------------------------------------------------------------------------------------------------------ clients
def test_clients_accept_the_opt_in_and_refuse_without_it():
    from vision_inspection_system_amd.client import CannedResponseClient, LocalVLMClient
    m = CannedResponseClient()
    m.chat.completions.create(model="synthetic:tiny", messages=MSGS, max_tokens=8, speculative=SAMPLED, temperature=0.7)
    assert m.calls[-1]["speculative"] == SAMPLED and m.calls[-1]["temperature"] == 0.7
    m.chat.completions.create(model="synthetic:tiny", messages=MSGS, max_tokens=8, speculative=SAMPLED, temperature=0.1, seed=7,
                              prediction={"type": "content", "content": "hello there"})
    assert m.calls[-1]["speculative"] == SAMPLED and m.calls[-1]["seed"] == 7 and "prediction" in m.calls[-1]
    for client in (LocalVLMClient(), CannedResponseClient()):
        create = client.chat.completions.create
        with pytest.raises(ValueError, match="speculative together with temperature"):
            create(model="synthetic:tiny", messages=MSGS, max_tokens=8, speculative=SPEC, temperature=0.7)
        with pytest.raises(ValueError, match="speculative together with a seed"):
            create(model="synthetic:tiny", messages=MSGS, max_tokens=8, speculative=SPEC, seed=7)
        with pytest.raises(ValueError, match="temperature"):      # a prediction alone stays greedy-only
            create(model="synthetic:tiny", messages=MSGS, max_tokens=8, temperature=0.7,
                   prediction={"type": "content", "content": "hello there"})
        for name, value in (("top_p", 0.9), ("n", 2), ("stop", ["\n"]), ("logprobs", True), ("stream", True)):
            with pytest.raises(ValueError, match="speculative"):
                create(model="synthetic:tiny", messages=MSGS, max_tokens=8, speculative=SAMPLED, temperature=0.7, **{name: value})
        with pytest.raises(ValueError, match="sampled"):
            create(model="synthetic:tiny", messages=MSGS, max_tokens=8, speculative={**SPEC, "sampled": 1})
    with pytest.raises(TypeError):
        LocalVLMClient().complete_many("synthetic:tiny", [MSGS], temperature=0.7, speculative=SAMPLED)


def test_engines_accept_the_opt_in_before_any_gpu_work():
    """generate(): with the opt-in a temperature and a seed pass the checks (the call then fails on the engine object that was
    never initialised - anything but the refusal); top_p stays refused by name."""
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    eng = Qwen2VLEngine.__new__(Qwen2VLEngine)
    with pytest.raises(ValueError, match="speculative together with top_p"):
        eng.generate([1, 2, 3], speculative=SAMPLED, temperature=0.7, seed=3, top_p=0.9)
    with pytest.raises(ValueError, match="speculative together with temperature"):
        eng.generate([1, 2, 3], speculative=SPEC, temperature=0.7)
    with pytest.raises(AttributeError):
        eng.generate([1, 2, 3], speculative=SAMPLED, temperature=0.7, seed=3)


def test_sampled_seed_of_the_client():
    from vision_inspection_system_amd.spec import SpecConfig, sampled_seed
    assert sampled_seed(SpecConfig(2, 4, 2), None, 11) == ({}, None)      # not opted in: the call of before
    assert sampled_seed(SpecConfig(2, 4, 2), 0, 11) == ({}, None)
    assert sampled_seed(SpecConfig(2, 4, 2, True), None, 11) == ({"seed": 11}, None)      # the client's own seed
    assert sampled_seed(SpecConfig(2, 4, 2, True), 7, 11) == ({"seed": 7}, None)
    assert sampled_seed(SpecConfig(2, 4, 2, True), 0, 11) == ({"seed": 0}, None)
    with pytest.raises(ValueError, match="seed"):
        sampled_seed(SpecConfig(2, 4, 2, True), "7", 11)


# ------------------------------------------------------------------------------------------------------------ reference
def test_accept_ref_sampled_hand_written():
    from vision_inspection_system_amd.spec import accept_ref, accept_ref_sampled
    toks = np.zeros(10, dtype=np.int32)
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 6], 2, 4, 9, toks, [0, 0, 0])          # second draft wrong
    assert (cur, st, c) == (2, 6, [1, 2, 1]) and t.tolist() == [0, 0, 0, 0, 5, 2, 0, 0, 0, 0]
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 2, 4, 9, toks, [0, 0, 0])          # both right
    assert (cur, st, c) == (7, 7, [1, 2, 2]) and t[4:7].tolist() == [5, 2, 7]
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [9, 2], 2, 4, 9, toks, [3, 3, 3])          # first wrong
    assert (cur, st, c) == (5, 5, [4, 5, 3]) and t[4:6].tolist() == [5, 0]
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 2, 4, 5, toks, [0, 0, 0])          # the limit cuts the run
    assert (cur, st, c) == (2, 6, [1, 2, 1]) and t[6] == 0
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 2, 4, 99, toks, [0, 0, 0])         # ... and the token row's end
    assert (cur, st, c) == (7, 7, [1, 2, 2])
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 2, 9, 99, toks, [0, 0, 0])
    assert (cur, st, c) == (5, 10, [1, 2, 0]) and t[9] == 5
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 2, 6, 5, toks, [1, 1, 1])          # past the limit: nothing
    assert (cur, st, c) == (None, 6, [1, 1, 1]) and not t.any()
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 2, -1, 5, toks, [1, 1, 1])
    assert (cur, st, c) == (None, -1, [1, 1, 1])
    t, cur, st, c = accept_ref_sampled([5, 2, 7], [5, 2], 7, 0, 9, toks, [0, 0, 0])          # the draft count is clamped to R - 1
    assert (cur, st, c) == (7, 3, [1, 2, 2])
    t, cur, st, c = accept_ref_sampled([5], [], 0, 0, 9, toks, [0, 0, 0])                    # one row
    assert (cur, st, c) == (5, 1, [1, 0, 0])
    # it is the model-free half of accept_ref: on the greedy picks both walk alike
    lg = np.full((3, 8), -1.0, dtype=np.float32)
    lg[0, 5] = lg[1, 6] = lg[2, 7] = lg[1, 2] = 2.0
    for draft, step, limit in (([5, 6], 4, 9), ([5, 2], 4, 9), ([5, 2], 4, 5), ([5, 2], 6, 5)):
        a, b = accept_ref(lg, draft, 2, step, limit, toks, [0, 0, 0]), accept_ref_sampled([5, 2, 7], draft, 2, step, limit, toks, [0, 0, 0])
        assert a[1:] == b[1:] and np.array_equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------------------ off state
class _Recorder:
    """Stands in for the ``hip`` module: every launch is recorded by name, none runs."""
    ACT_SWIGLU = 3

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        def launch(*a, **kw):
            self.names.append(name)
        return launch


def _step_names(monkeypatch, cfg, pred=False):
    import torch
    from vision_inspection_system_amd import decode_stage
    from vision_inspection_system_amd.decode_stage import DecodeStage
    rec = _Recorder()
    monkeypatch.setattr(decode_stage, "hip", rec)
    z = torch.zeros((4, 8))
    st = DecodeStage.__new__(DecodeStage)
    st.cfg = types.SimpleNamespace(heads=2, kv_heads=1, head_dim=128, rms_eps=1e-6, vocab=8)
    st.decode_weights, st.dec_layers, st.dec_head, st.dec_norm_w = "bf16", [], {"bf16": (z,)}, z
    st.w = types.SimpleNamespace(embed=z)
    st.tokens, st.step = z, z
    st._spec = types.SimpleNamespace(x=z, x2=z, qkv=z, attn=z, act=z, logits=z, ids=z, draft=z, cur=z, n_draft=z, limit=z,
                                     ws_val=z, ws_idx=z, counters=z, params=z, prompt=z, prompt_len=z, gen_start=z, pred=z,
                                     pred_len=z, pred_state=z)
    st._spec_cfg, st._spec_pred = cfg, pred
    st._decode_step_spec(cfg.rows)
    return rec.names


def test_off_state_never_names_the_new_entry_point(monkeypatch):
    """The step of a configuration that did not opt in issues exactly the launches of before; the opted-in step differs in the
    accept alone."""
    from vision_inspection_system_amd.spec import SpecConfig
    for pred in (False, True):
        draft = "spec_draft_pred" if pred else "spec_draft"
        off = _step_names(monkeypatch, SpecConfig(2, 4, 2), pred)
        assert off == ["gather_rows", "gemv_rows", "spec_accept", draft]
        assert not any("sampled" in n for n in off)
        on = _step_names(monkeypatch, SpecConfig(2, 4, 2, True), pred)
        assert on == ["gather_rows", "gemv_rows", "spec_accept_sampled", draft]


def test_plain_steps_name_no_speculative_launch():
    import inspect
    from vision_inspection_system_amd.decode_stage import DecodeStage
    for fn in (DecodeStage._decode_step_rows, DecodeStage._decode_step_streamk, DecodeStage._decode_step_fused):
        assert "spec" not in inspect.getsource(fn)


def test_binding_names_the_entry_point():
    from vision_inspection_system_amd import hip
    assert hip._SIGS["vis_spec_accept_sampled"] == hip._SIGS["vis_spec_accept"] + "p"
    assert "vis_spec_accept_sampled" in hip.exported_symbols()


# ------------------------------------------------------------------------------------------------------------ input tables
@pytest.mark.parametrize("V", C.VS)
def test_tables_meet_the_ambiguity_cap(V):
    """The cap the GPU test relies on, asserted on what the tables finally hold; and the tables' decisive picks held against
    the reference's own intervals (`perturbed`): the pick's lower bound lies above every other id's upper bound."""
    entries = C.cases(V)
    assert {c.inv_temp for c in entries} == {0.0, 0.5, 10.0} and {c.seed for c in entries} == set(C.SEEDS)
    for case in entries:
        assert case.logits.shape == (case.R, V) and 1 <= case.R <= 4
        assert case.ambiguous_share() <= AMBIGUOUS_CAP, case.name
        for st in C.STARTS:
            for r, cand in enumerate(case.expected[st]):
                assert cand.size >= 1 and (cand >= 0).all() and (cand < V).all()
                if case.inv_temp == 0.0 or np.isnan(case.logits[r]).all() or cand.size != 1:
                    continue
                u = noise_u(case.seed, st + r, np.arange(V))
                assert ((u > 0) & (u < 1)).all()
                lo, hi = perturbed(case.logits[r], case.inv_temp, case.seed, st + r, np.arange(V))
                others = np.delete(hi, cand[0])
                assert lo[cand[0]] > others[~np.isnan(others)].max(), (case.name, st, r)
    assert any("nan" in c.kinds for v in C.VS for c in C.cases(v)) and any("tie_wg" in c.kinds for v in C.VS for c in C.cases(v))


def test_tables_depend_on_the_row_counter():
    """Row r draws at hash counter st + r: the expectation of a sampled row changes with r and with st (else the GPU test could
    not tell a kernel that used st for every row)."""
    case = next(c for c in C.cases(1000) if c.inv_temp == 0.5)
    row = case.logits[0]
    picks = {int(candidates(row, 0.5, case.seed, s, np.arange(1000))[0]) for s in range(8)}
    assert len(picks) > 3
    assert C.params_words(0.5, 0xFFFFFFFF).tolist() == [0x3F000000, -1]
    assert C.diff_rows(200).shape == (4, 200) and np.isnan(C.diff_rows(200)[1]).all()
    assert [C.diff_row_ids(R) for R in (1, 2, 3, 4)] == [[1], [2, 3], [3, 0, 1], [0, 1, 2, 3]]
