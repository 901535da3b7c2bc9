"""The schema as a drafter (schema_draft.py) and the ``grammar`` opt-in of a speculative request (spec.py), without a GPU:
the jump tables against the DFA they are built from, the drafts from the report schema's start, the model-free walk, and
what check_speculative / check_exclusive / the environment let through."""
import os
import random
import re

import numpy as np
import pytest

from schema_cases import AllOptional, Closed, Flat, Nested, distance_to_accept, random_walk
from vision_inspection_system_amd import json_grammar as G
from vision_inspection_system_amd import json_schema as S
from vision_inspection_system_amd import schema_draft as D
from vision_inspection_system_amd import spec
from vision_inspection_system_amd.schemas import REPORT_SCHEMA
from vision_inspection_system_amd.spec import SpecConfig, check_exclusive, check_speculative

SCHEMAS = {"flat": Flat.model_json_schema(), "nested": Nested.model_json_schema(), "report": REPORT_SCHEMA,
           "optional": AllOptional.model_json_schema(), "closed": Closed.model_json_schema()}
WS = b" \t\n\r"


class _Bytes:
    """ids 0..255 the single bytes, 256 / 257 EOS."""

    def token_bytes(self, t):
        return bytes([t]) if t < 256 else b""


class _Merged(_Bytes):
    """The single bytes, then pieces a report's fixed text is made of (some twice: the lower id must win), then specials."""
    PIECES = [b'{"', b'":', b'",', b'","', b'": "', b'"object', b"object_identified", b"_identified", b'{"object_identified":',
              b"overall_", b"condition", b"defects", b'":[', b"true", b"false", b"null", b"name", b'{"name', b'{"name":"',
              b"count", b"title", b'{"', b"nul", b"ull", b"rue", b"alse", b'{"a', b'":', b"kind", b'"}', b"}"]

    def token_bytes(self, t):
        return super().token_bytes(t) if t < 258 else (self.PIECES[t - 258] if t - 258 < len(self.PIECES) else b"")


def _table(kind):
    if kind == "bytes":
        return G.build_token_table(_Bytes(), 258, [256, 257])
    return G.build_token_table(_Merged(), 258 + len(_Merged.PIECES) + 3, [256, 257])


@pytest.fixture(scope="module")
def dfas():
    return {k: S.compile_schema(v) for k, v in SCHEMAS.items()}


def _forced_path_by_definition(dfa, s):
    """The issue's definition, byte by byte over all 256 byte values."""
    out, seen = bytearray(), set()
    while len(out) < 48 and s not in seen and not dfa.state_flags[s] & S.STATE_ACCEPT:
        seen.add(s)
        live = [b for b in range(256) if S.step(dfa, s, b) != S.DEAD]
        solid = [b for b in live if b not in WS]
        if len(live) == 1:
            b = live[0]
        elif len(solid) == 1 and len(solid) < len(live):
            b = solid[0]
        else:
            break
        out.append(b)
        s = S.step(dfa, s, b)
    return bytes(out)


@pytest.mark.parametrize("kind", ["bytes", "merged"])
@pytest.mark.parametrize("name", list(SCHEMAS))
def test_jump_tables_follow_the_dfa(dfas, name, kind):
    dfa, table = dfas[name], _table(kind)
    t = D.build(dfa, table)
    assert t.jump_tok.shape == t.jump_next.shape == (S.SCHEMA_MAX_STATES,) and t.jump_tok.dtype == t.jump_next.dtype == np.int32
    assert (t.jump_tok[dfa.n_states:] == -1).all() and (t.jump_next[dfa.n_states:] == -1).all()
    drafted = 0
    for s in range(dfa.n_states):
        path = _forced_path_by_definition(dfa, s)
        assert D.forced_path(dfa, s) == path
        # the longest non-EOS token that spells a non-empty prefix of the path, the lowest id among equals
        best = -1
        for tok in range(table.vocab):
            b = table.tokens[tok]
            if b and not table.flags[tok] & G.FLAG_EOS and path.startswith(b) and \
                    (best < 0 or len(b) > len(table.tokens[best])):
                best = tok
        assert t.jump_tok[s] == best, (s, path)
        if best < 0:
            assert t.jump_next[s] == -1
            continue
        drafted += 1
        words = S.allowed_mask(dfa, s, table)
        assert (int(words[best >> 6]) >> (best & 63)) & 1, (s, best)
        assert t.jump_next[s] == S.walk(dfa, s, table.tokens[best]) != S.DEAD
    assert drafted > 0
    if kind == "bytes":      # every forced byte is a token: a state drafts exactly when it forces a byte
        assert drafted == int((D.forced_bytes(dfa) >= 0).sum())


@pytest.mark.parametrize("kind", ["bytes", "merged"])
def test_report_schema_starts_with_its_first_key(dfas, kind):
    dfa, table = dfas["report"], _table(kind)
    t = D.build(dfa, table)
    key = REPORT_SCHEMA["required"][0]
    want = b'{"' + key.encode()
    drafts, s, spelled = [], dfa.start, b""
    while len(spelled) < len(want):
        d = D.propose(dfa, t, s, 3)
        assert d, spelled
        for tok in d:
            spelled += table.tokens[tok]
            s = S.walk(dfa, s, table.tokens[tok])
        drafts += d
    assert spelled.startswith(want), spelled
    assert D.propose(dfa, t, dfa.start, 2) == drafts[:2] and D.propose(dfa, t, dfa.start, 1) == drafts[:1]
    if kind == "bytes":
        assert D.propose(dfa, t, dfa.start, 3) == list(want[:3])
    elif key == "object_identified":      # one jump covers the key, its colon included (the compact spelling)
        assert drafts[0] == 258 + _Merged.PIECES.index(b'{"object_identified":')
    accept = int(np.flatnonzero(dfa.state_flags & S.STATE_ACCEPT)[0])
    assert D.propose(dfa, t, accept, 3) == [] and D.propose(dfa, t, S.DEAD, 3) == []


@pytest.mark.parametrize("name", ["report", "closed", "nested"])
def test_simulate_drafts_every_forced_byte(dfas, name):
    dfa, table = dfas[name], _table("bytes")
    t = D.build(dfa, table)
    rng = random.Random(7)
    doc, end = random_walk(dfa, rng, distance_to_accept(dfa), wander=0)
    assert dfa.state_flags[end] & S.STATE_ACCEPT
    reply = list(doc) + [256]
    forced = D.forced_bytes(dfa)
    for k in (1, 3):
        cfg = SpecConfig(k, 4, 2, False, True)
        out = D.simulate(dfa, t, table, reply, cfg)
        assert out["reply"] == reply
        assert out["spec_steps"] + out["spec_accepted"] == len(reply) - 1
        assert 0 < out["spec_accepted"] <= out["spec_proposed"]
        assert out["spec_steps"] < len(reply) - 1, "the schema's forced bytes saved no step"
        # step by step: in a state that forces a byte the schema drafts it, and a compact-spelled document accepts what it
        # is offered unless it spelled whitespace there
        s, n, steps = S.walk(dfa, dfa.start, bytes(reply[:1])), 1, 0
        while n < len(reply):
            d = D.propose(dfa, t, s, k)
            assert bool(d) == (forced[s] >= 0)
            a = 0
            while a < len(d) and n + a < len(reply) - 1 and d[a] == reply[n + a]:
                a += 1
            for tok in reply[n:n + a + 1]:
                s = S.walk(dfa, s, table.tokens[tok]) if tok < 256 else s
            n, steps = n + a + 1, steps + 1
        assert steps == out["spec_steps"]
    # the mask alone: the lookup's drafts only, and a cut by max_new_tokens
    off = D.simulate(dfa, t, table, reply, SpecConfig(3, 4, 2, False, True, False), prompt=reply[:20])
    assert off["schema_proposed"] == 0 and off["reply"] == reply
    cut = D.simulate(dfa, t, table, reply, SpecConfig(3, 4, 2, False, True), max_new_tokens=9)
    assert cut["reply"] == reply[:9]


def test_config_record_and_opt_in():
    assert SpecConfig(2, 4, 2) == SpecConfig(2, 4, 2, False) == SpecConfig(2, 4, 2, False, False) == SpecConfig(2, 4, 2, False, False, None)
    assert tuple(SpecConfig(2, 4, 2, False, False, False)) == (2, 4, 2) and tuple(SpecConfig(2, 4, 2, True)) == (2, 4, 2, True)
    base = SpecConfig(2, 4, 2)
    assert (base.sampled, base.grammar, base.schema_drafts) == (False, False, False)
    g = check_speculative({"num_speculative_tokens": 2, "grammar": True})
    assert (g.k, g.sampled, g.grammar, g.schema_drafts) == (2, False, True, True) and g != base and g == SpecConfig(2, 4, 2, False, True)
    m = check_speculative({"num_speculative_tokens": 2, "grammar": True, "schema_drafts": False})
    assert (m.grammar, m.schema_drafts) == (True, False) and m != g
    sg = check_speculative({"num_speculative_tokens": 3, "sampled": True, "grammar": True})
    assert (sg.sampled, sg.grammar, sg.schema_drafts, sg.rows) == (True, True, True, 4)
    for c in (base, g, m, sg, SpecConfig(1, 5, 1, True)):
        assert check_speculative(c) == c      # the opt-ins survive a second reading
    assert check_speculative({"num_speculative_tokens": 2, "grammar": False, "schema_drafts": False}) == base
    for bad in ({"grammar": 1}, {"grammar": "yes"}, {"grammar": True, "schema_drafts": 1}, {"schema_drafts": True}, {"grammer": True}):
        with pytest.raises(ValueError):
            check_speculative({"num_speculative_tokens": 2, **bad})
    assert "grammar=True" in repr(g) and "grammar" not in repr(base)


RF = {"type": "json_schema", "json_schema": {"name": "r", "schema": SCHEMAS["closed"]}}
TODAY = ("speculative together with {} is not supported: it is a per-step state of the pick, and a speculative step yields "
         "several tokens")


def test_grammar_lets_only_the_schema_through(dfas):
    plain, g = SpecConfig(2, 4, 2), SpecConfig(2, 4, 2, False, True)
    dfa = dfas["closed"]
    # without the opt-in: today's refusals, word for word
    for name, v in (("json_schema", dfa), ("response_format", RF), ("response_format", {"type": "json_object"}), ("json_mode", True)):
        with pytest.raises(ValueError) as e:
            check_exclusive(plain, **{name: v})
        assert str(e.value) == TODAY.format(name)
    check_exclusive(g, json_schema=dfa)
    check_exclusive(g, response_format=RF)
    check_exclusive(g, json_schema=dfa, top_p=1.0, n=1, stream=False)      # neutral values stay neutral
    # grammar without a schema
    for kw in ({}, {"response_format": {"type": "text"}}, {"response_format": None}, {"json_schema": None}):
        with pytest.raises(ValueError, match="'grammar' needs a JSON Schema"):
            check_exclusive(g, **kw)
    # every other switch stays refused, with today's message
    others = {"json_mode": True, "top_p": 0.9, "repetition_penalty": 1.1, "frequency_penalty": 0.5, "presence_penalty": 0.5,
              "top_k": 5, "min_p": 0.1, "logit_bias": {1: 1.0}, "no_repeat_ngram_size": 2, "bad_words": ["x"], "min_tokens": 2,
              "stop": "a", "stream": True, "on_stream": object(), "logprobs": True, "top_logprobs": 2, "n": 2, "seeds": [1]}
    for name, v in others.items():
        with pytest.raises(ValueError) as e:
            check_exclusive(g, json_schema=dfa, **{name: v})
        assert str(e.value) == TODAY.format(name), name
    with pytest.raises(ValueError) as e:
        check_exclusive(g, response_format={"type": "json_object"})
    assert "'grammar' needs a JSON Schema" in str(e.value)
    with pytest.raises(ValueError) as e:
        check_exclusive(g, response_format={"type": "json_object"}, json_schema=dfa)
    assert str(e.value) == TODAY.format("response_format")
    # temperature and seed: as for every speculative request
    with pytest.raises(ValueError, match="temperature > 0"):
        check_exclusive(g, 0.5, json_schema=dfa)
    with pytest.raises(ValueError, match="together with a seed"):
        check_exclusive(g, 0.0, 3, json_schema=dfa)
    check_exclusive(SpecConfig(2, 4, 2, True, True), 0.5, 3, json_schema=dfa)
    with pytest.raises(ValueError) as e:
        check_exclusive(SpecConfig(2, 4, 2, True), 0.5, 3, json_schema=dfa)
    assert str(e.value) == TODAY.format("json_schema")


def test_prediction_and_the_schemas_drafts():
    with pytest.raises(ValueError, match="schema_drafts"):
        spec.with_prediction({"num_speculative_tokens": 2, "grammar": True}, True)
    c = spec.with_prediction({"num_speculative_tokens": 2, "grammar": True, "schema_drafts": False}, True)
    assert c.grammar and not c.schema_drafts
    assert spec.with_prediction({"num_speculative_tokens": 2, "grammar": True}, False).schema_drafts
    assert spec.with_prediction(None, True) == spec.PRED_DEFAULT == SpecConfig(3, 4, 2)


def test_client_checks_without_a_model():
    from vision_inspection_system_amd.client import CannedResponseClient, check_speculative_request
    sp = {"method": "ngram", "num_speculative_tokens": 2}
    g = {**sp, "grammar": True}
    assert check_speculative_request(g, response_format=RF).grammar
    with pytest.raises(ValueError) as e:
        check_speculative_request(sp, response_format=RF)
    assert str(e.value) == TODAY.format("response_format")
    with pytest.raises(ValueError, match="'grammar' needs a JSON Schema"):
        check_speculative_request(g)
    with pytest.raises(ValueError):
        check_speculative_request(g, response_format=RF, prediction={"type": "content", "content": "{}"})
    assert check_speculative_request({**g, "schema_drafts": False}, response_format=RF,
                                     prediction={"type": "content", "content": "{}"}).grammar
    on, seed = spec.sampled_seed(check_speculative(g), None, 11, RF)
    assert seed is None and set(on) == {"json_schema"} and isinstance(on["json_schema"], S.SchemaDFA)
    on, _ = spec.sampled_seed(check_speculative({**g, "sampled": True}), 5, 11, RF)
    assert on["seed"] == 5 and isinstance(on["json_schema"], S.SchemaDFA)
    c = CannedResponseClient("{}")
    msgs = [{"role": "user", "content": "x"}]
    c.chat.completions.create(model="m", messages=msgs, response_format=RF, speculative=g)
    assert c.calls[-1]["speculative"] == g and c.calls[-1]["response_format"] == RF
    with pytest.raises(ValueError):
        c.chat.completions.create(model="m", messages=msgs, response_format=RF, speculative=sp)


def test_environment_switch(monkeypatch):
    from vision_inspection_system_amd import agents
    from vision_inspection_system_amd.client import CannedResponseClient
    from vision_inspection_system_amd.schemas import REPORT_RESPONSE_FORMAT
    for name in ("VIS_SPECULATIVE", "VIS_AUDITOR_SPECULATIVE", "VIS_SPECULATIVE_SAMPLED", "VIS_SPECULATIVE_GRAMMAR", "VIS_JSON_SCHEMA"):
        monkeypatch.delenv(name, raising=False)
    c = CannedResponseClient("{}")
    rf = {"response_format": REPORT_RESPONSE_FORMAT}
    monkeypatch.setenv("VIS_SPECULATIVE_GRAMMAR", "1")
    assert spec.grammar_from_env() is True and spec.from_env() is None and spec.auditor_from_env() is None
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, rf) == {}      # alone it turns nothing on
    monkeypatch.setenv("VIS_SPECULATIVE", "2")
    monkeypatch.setenv("VIS_AUDITOR_SPECULATIVE", "3")
    assert spec.from_env() == SpecConfig(2, 4, 2, False, True) and spec.auditor_from_env() == SpecConfig(3, 4, 2, False, True)
    want = {"speculative": {"method": "ngram", "num_speculative_tokens": 2, "grammar": True}}
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, rf) == want
    assert agents.speculative_kwargs(c, "synthetic:mllama-tiny", 0.0, rf)["speculative"]["num_speculative_tokens"] == 3
    # a request without the schema: the dict of before; another switch, or a temperature: still no speculation
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, {}) == {"speculative": {"method": "ngram", "num_speculative_tokens": 2}}
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, {"response_format": {"type": "json_object"}}) == {}
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, {**rf, "stop": "a"}) == {}
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.2, rf) == {}
    monkeypatch.setenv("VIS_SPECULATIVE_SAMPLED", "1")
    assert agents.speculative_kwargs(c, "synthetic:tiny", 0.2, {**rf, "seed": 3})["speculative"] == \
        {"method": "ngram", "num_speculative_tokens": 2, "sampled": True, "grammar": True}
    monkeypatch.delenv("VIS_SPECULATIVE_SAMPLED")
    for off in ("", "0"):
        monkeypatch.setenv("VIS_SPECULATIVE_GRAMMAR", off)
        assert spec.grammar_from_env() is False and spec.from_env() == SpecConfig(2, 4, 2)
        assert agents.speculative_kwargs(c, "synthetic:tiny", 0.0, rf) == {}
    for bad in ("2", "yes", "true"):
        monkeypatch.setenv("VIS_SPECULATIVE_GRAMMAR", bad)
        with pytest.raises(ValueError, match="VIS_SPECULATIVE_GRAMMAR"):
            spec.from_env()


def test_shared_kernel_header_is_schema_masks_own():
    """csrc/schema_common.hip.h restates schema_mask.hip's constants, slot words and byte walk for spec_schema.hip."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vision-inspection-system_amd", "csrc")
    own, shared = (open(os.path.join(csrc, n)).read() for n in ("schema_mask.hip", "schema_common.hip.h"))
    defines = lambda src: dict(re.findall(r"^#define (SM_\w+) (.+?)\s*(?://.*)?$", src, re.M))      # noqa: E731
    assert defines(shared) == defines(own) and len(defines(own)) >= 17
    assert "enum { SW_STATE, SW_ERR, SW_POS, SW_ANCHOR };" in own and "enum { SW_STATE, SW_ERR, SW_POS, SW_ANCHOR };" in shared
    walk = re.search(r"template <typename T>\n__device__ __forceinline__ unsigned sm_walk\(.*?\n}\n", own, re.S).group(0)
    assert walk in shared
    spec = open(os.path.join(csrc, "spec_schema.hip")).read()
    assert '#include "schema_common.hip.h"' in spec and not re.search(r"^#define SM_", spec, re.M)
