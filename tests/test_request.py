"""The request's way in, without a GPU: request.Switches (the record the engines build from their ``**switches``), the
client's one model-free check (client.engine_keywords), and the recorded pin of what reaches the engines - every call of
tests/golden/gen_request_keywords.py replayed against tests/golden/request_keywords.json, which was recorded in front of the
change that introduced the record."""
import dataclasses
import io
import json
import os
import sys
import tokenize

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_request_keywords as G  # noqa: E402

from vision_inspection_system_amd import client as CL  # noqa: E402
from vision_inspection_system_amd.ban import BanRequest, ban_kwargs, check_ban  # noqa: E402
from vision_inspection_system_amd.engine import Qwen2VLEngine  # noqa: E402
from vision_inspection_system_amd.mllama_engine import MllamaEngine  # noqa: E402
from vision_inspection_system_amd.penalties import check_penalties  # noqa: E402
from vision_inspection_system_amd.request import PENALTY_NAMES, Switches  # noqa: E402
from vision_inspection_system_amd.shaping import check_shaping, shaping_kwargs  # noqa: E402
from test_generation import Recorders, no_device_events  # noqa: E402,F401  (the autouse fixture comes along)

with open(os.path.join(HERE, "golden", "request_keywords.json")) as _f:
    GOLDEN = json.load(_f)
PKG = os.path.join(os.path.dirname(HERE), "vision-inspection-system_amd")
ENGINES = (Qwen2VLEngine, MllamaEngine)
MSGS = [{"role": "user", "content": "hi"}]


# ----------------------------------------------------------------------------- the recorded pin
@pytest.fixture(scope="module")
def stand_ins():
    with G.stand_ins() as engines:
        yield engines


def test_the_record_names_its_commit_and_covers_every_case():
    assert len(GOLDEN["header"]["recorded_at_commit"]) == 40
    assert sorted(GOLDEN["cases"]) == sorted(G.CASES)


@pytest.mark.parametrize("name", list(G.CASES))
def test_engines_and_mock_client_get_what_they_got(stand_ins, name):
    got, want = G.record(name, stand_ins), GOLDEN["cases"][name]
    assert sorted(got) == sorted(want)
    for who in want:
        assert G.text(got[who]) == G.text(want[who]), f"{name}: {who}"


# ----------------------------------------------------------------------------- the record
def test_no_keyword_is_the_defaults():
    for sw in (Switches(), Switches.single(), Switches.group()):
        assert all(getattr(sw, f.name) is f.default for f in dataclasses.fields(sw))
        assert sw.exclusive() == {} and sw.request(0) == sw
    assert [f.name for f in dataclasses.fields(Switches)] == [
        "logprobs", "json_mode", "top_p", "repetition_penalty", "frequency_penalty", "presence_penalty", "json_schema", "stop",
        "top_k", "min_p", "logit_bias", "on_stream", "no_repeat_ngram_size", "bad_words", "min_tokens", "seeds", "n",
        "speculative", "prediction"]


def test_exclusive_hands_over_what_is_on_in_the_order_of_the_fields():
    sw = Switches.single(min_tokens=2, stop="x", logprobs=0, json_mode=False, top_p=None, speculative=2, prediction=[1])
    assert list(sw.exclusive().items()) == [("logprobs", 0), ("stop", "x"), ("min_tokens", 2)]
    assert Switches.single(json_mode=0).exclusive() == {"json_mode": 0}      # not the default itself: the check's to judge


@pytest.mark.parametrize("E", ENGINES)
def test_an_unknown_keyword_is_a_type_error_that_names_it(E):
    eng = E.__new__(E)
    with pytest.raises(TypeError, match="best_of"):
        eng.generate([1, 2, 3], best_of=2)
    with pytest.raises(TypeError, match="best_of"):
        eng.generate_batch([([1, 2, 3], None)], best_of=2)
    for name in ("seeds", "n"):
        with pytest.raises(TypeError, match=name):
            eng.generate([1, 2, 3], **{name: [1]})
    with pytest.raises(TypeError, match="speculative"):
        eng.generate_batch([([1, 2, 3], None)], speculative=2)
    with pytest.raises(ValueError, match="serves one request per call"):
        eng.generate_batch([([1, 2, 3], None)], prediction=[1, 2])
    with pytest.raises(TypeError, match="speculative"):       # the keyword that is no switch is named before the prediction
        eng.generate_batch([([1, 2, 3], None)], prediction=[1, 2], speculative=2)


def test_complete_many_refuses_what_it_does_not_offer():
    c = CL.LocalVLMClient()
    with pytest.raises(TypeError, match="best_of"):
        c.complete_many("synthetic:tiny", [MSGS], best_of=2)
    with pytest.raises(TypeError, match="speculative"):
        c.complete_many("synthetic:tiny", [MSGS], speculative={"method": "ngram", "num_speculative_tokens": 2})
    with pytest.raises(ValueError, match="serves one request per call"):
        c.complete_many("synthetic:tiny", [MSGS], prediction={"type": "content", "content": "x"})
    with pytest.raises(TypeError, match="best_of"):
        CL.engine_keywords(8, best_of=2)


# three requests, pairwise different and none at its neutral value, in every per-request field
GROUP = dict(repetition_penalty=[1.1, 1.2, 1.3], frequency_penalty=[0.5, -0.5, 1], presence_penalty=[-1, 0.25, 2],
             top_k=[3, 40, 7], min_p=[0.05, 0.1, 0.5], logit_bias=[{5: -100}, {"7": 2.5, 9: 1}, {11: -1.5}],
             no_repeat_ngram_size=[2, 3, 4], min_tokens=[1, 2, 3], bad_words=["x", "As an AI"])
SHARED = dict(logprobs=2, top_p=0.9, stop=["END"], on_stream=object(), json_mode=False)


@pytest.mark.parametrize("b", range(3))
def test_request_b_is_what_the_single_route_was_handed(b):
    """The keywords the single-sequence route got in front of the record: the group's checked rows through shaping_kwargs /
    ban_kwargs / the zipped penalty triple, here for request ``b`` of three."""
    penalties = check_penalties(*(GROUP[name] for name in PENALTY_NAMES), 3)
    shaping = check_shaping(GROUP["top_k"], GROUP["min_p"], GROUP["logit_bias"], 3)
    ban = check_ban(GROUP["no_repeat_ngram_size"], GROUP["bad_words"], GROUP["min_tokens"], 3, 16)
    want = dict(SHARED, **dict(zip(PENALTY_NAMES, penalties[b])), **shaping_kwargs(shaping[b:b + 1]),
                **ban_kwargs(BanRequest(ban.rows[b:b + 1], ban.words)))
    assert want["logit_bias"] == [{5: -100.0}, {7: 2.5, 9: 1.0}, {11: -1.5}][b] and want["bad_words"] == ["x", "As an AI"]
    got = Switches.group(seeds=[4, 5, 6], n=[1, 2, 1], **GROUP, **SHARED).request(b)
    assert got == Switches.single(**want)
    assert got.seeds is None and got.n is None and got.min_tokens == b + 1 and got.top_k == [3, 40, 7][b]
    assert {name: getattr(got, name) for name in want} == want
    assert all(type(getattr(got, name)) is type(v) for name, v in want.items())


def test_request_of_one_value_for_the_group_and_of_switches_that_are_off():
    sw = Switches.group(top_k=5, repetition_penalty=1.2, min_tokens=0, min_p=0, logit_bias={}, bad_words=[], n=[1])
    one = sw.request(0)
    # shaping and the penalties are on: their whole family comes in the checked form; the bans are off: None throughout
    assert (one.top_k, one.min_p, one.logit_bias) == (5, None, None)
    assert (one.repetition_penalty, one.frequency_penalty, one.presence_penalty) == (1.2, 0.0, 0.0)
    assert (one.no_repeat_ngram_size, one.bad_words, one.min_tokens, one.n) == (None, None, None, None)
    on = Switches.group(min_tokens=3).request(0)
    assert (on.no_repeat_ngram_size, on.bad_words, on.min_tokens) == (0, None, 3)


class _Stub(Recorders, Qwen2VLEngine):
    keep_eos, spelling = False, "ignore_eos"

    def _generate(self, *args):
        self.log.append(("_generate", args[-1]))
        return super()._generate(*args)


def test_the_one_request_routes_pass_the_record_on():
    eng = _Stub()
    given = dict(top_k=[5], repetition_penalty=1.2, stop="x", seeds=[9])
    eng.stop_at = 3
    eng.generate_batch([(list(range(1, 11)), ["frame"])], max_new_tokens=6, n=[1], **given)
    passed = [c[1] for c in eng.log if c[0] == "_generate"]
    assert passed == [Switches.group(**given).request(0)] and passed[0].seeds is None and passed[0].top_k == 5


# ----------------------------------------------------------------------------- the client's one check
def test_a_streamed_call_checks_its_arguments_in_the_call_and_once(stand_ins, monkeypatch):
    from vision_inspection_system_amd import sampling
    calls = []
    real = sampling.check_top_p
    monkeypatch.setattr(sampling, "check_top_p", lambda p: calls.append(p) or real(p))
    c = CL.LocalVLMClient(device="cpu")
    with pytest.raises(ValueError, match="top_p"):       # from the call itself: no next() has run
        c.complete_many(G.QWEN, [MSGS], stream=True, top_p=1.5)
    assert calls == [1.5] and stand_ins[G.QWEN].calls.clear() is None
    del calls[:]
    chunks = list(c.complete_many(G.QWEN, [MSGS, MSGS], stream=True, top_p=0.5))
    assert calls == [0.5] and len(stand_ins[G.QWEN].calls) == 1 and chunks[-1].choices[0].finish_reason == "stop"
    del calls[:]
    c.complete_many(G.QWEN, [MSGS], top_p=0.5)
    assert calls == [0.5]


def test_engine_keywords_is_the_engines_spelling_of_what_is_on():
    assert CL.engine_keywords() == ({}, None)
    on, seed = CL.engine_keywords(16, logprobs=True, top_logprobs=2, response_format={"type": "json_object"}, top_p=1, seed=3,
                                  presence_penalty=1, top_k=4, logit_bias={"5": 1}, n=99, stream=True, stop="a")
    assert seed == 3 and on == dict(logprobs=2, json_mode=True, stop=(b"a",), repetition_penalty=1.0, frequency_penalty=0.0,
                                    presence_penalty=1.0, top_k=4, logit_bias={5: 1.0}, top_p=1.0)      # check_top_p's own
    # form of "the whole vocabulary": handed on, as the record of neutral_top_p has it
    for name in ("logprobs_k", "json_mode_of", "schema_of", "check_ban_keywords", "check_speculative_request", "is_mllama_model"):
        assert callable(getattr(CL, name))
    assert not hasattr(CL.LocalVLMClient, "_check_keywords")


# ----------------------------------------------------------------------------- where the names are written down
def _code_names(path):
    """The NAME tokens of a source file: docstrings and other strings, and comments, are not among them."""
    with open(path) as f:
        return {t.string for t in tokenize.generate_tokens(io.StringIO(f.read()).readline) if t.type == tokenize.NAME}


def test_the_engines_name_no_switch_and_the_way_in_got_no_longer():
    """``seeds`` stays a parameter of prefill_many and ``speculative`` one of MllamaEngine's constructor (whether the engine is
    built for it): neither is the request's switch.  ``n`` is left out: a local variable of that name is no switch."""
    switches = {f.name for f in dataclasses.fields(Switches)} - {"n"}
    assert _code_names(os.path.join(PKG, "engine.py")) & switches == {"seeds"}
    assert _code_names(os.path.join(PKG, "mllama_engine.py")) & switches == {"seeds", "speculative"}
    lines = 0
    for name in ("client.py", "generation.py", "engine.py", "mllama_engine.py", "request.py"):
        with open(os.path.join(PKG, name)) as f:
            lines += len(f.readlines())
    assert lines < 3413      # client.py + generation.py + engine.py + mllama_engine.py in front of the record
