"""Schema-constrained decoding, the parts that need no GPU: the schema compiler and its DFA (json_schema, the reference of
vis_schema_mask) against pydantic in both directions, near-misses, live prefixes, refused schemas, the constants shared with
the kernel, allowed_mask against a per-token walk, and the client's / agents' response_format handling."""
import json
import os
import random
import re

import numpy as np
import pytest

from schema_cases import AllOptional, Flat, Nested, distance_to_accept, random_instance, random_walk
from vision_inspection_system_amd import json_grammar as G
from vision_inspection_system_amd import json_schema as S
from vision_inspection_system_amd.schemas import REPORT_SCHEMA, VLMAnalysisResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HF = os.path.join(ROOT, "tests", "golden", "hf_dirs")
RETRY_SUBSTRINGS = ("429", "rate", "413", "payload")
MODELS = [Flat, Nested, AllOptional, VLMAnalysisResult]
WALK_MODELS = [Flat, Nested, AllOptional]        # no code validators: the schema is the whole contract


@pytest.fixture(scope="module")
def dfas():
    return {m: S.compile_schema(m.model_json_schema()) for m in MODELS}


def _strict_loads(text: str):
    def no_constants(name):
        raise ValueError(f"not JSON: {name}")
    return json.loads(text, parse_constant=no_constants)


# ----------------------------------------------------------------------------- 1. pydantic as the oracle
@pytest.mark.parametrize("model", MODELS)
def test_pydantic_instances_are_accepted_in_both_spellings(dfas, model):
    rng = random.Random(7)
    dfa = dfas[model]
    for _ in range(150):
        inst = random_instance(model, rng)
        compact = inst.model_dump_json()
        spaced = json.dumps(inst.model_dump(mode="json"))
        assert ", " in spaced or ": " in spaced
        for text in (compact, spaced, json.dumps(inst.model_dump(mode="json"), ensure_ascii=False)):
            assert S.accepts(dfa, text.encode("utf-8")), text
    # a key that is not required may be left out, whatever else is present
    if model is AllOptional:
        for doc in ("{}", '{"a":1}', '{"b":"x"}', '{"c":[]}', '{"a":1,"c":[2]}', '{"b":"","c":null}', '{"a":null,"b":null,"c":null}'):
            assert S.accepts(dfa, doc.encode()), doc
            AllOptional.model_validate(json.loads(doc))


@pytest.mark.parametrize("model", WALK_MODELS)
def test_random_accepted_walks_satisfy_pydantic(dfas, model):
    rng = random.Random(11)
    dfa = dfas[model]
    dist = distance_to_accept(dfa)
    assert dist.max() < 10 ** 9                        # every state can still reach the end
    schema = model.model_json_schema()
    seen = set()
    for i in range(300):
        data, s = random_walk(dfa, rng, dist, wander=rng.choice([0, 20, 60, 150]))
        assert dfa.state_flags[s] & S.STATE_ACCEPT, data
        text = data.decode("utf-8")                     # strict
        obj = _strict_loads(text)
        assert S.validate(schema, obj), text
        model.model_validate(obj)       # (json.loads keeps a lone \\uD800 escape, which RFC 8259's grammar and JSON mode allow)
        assert set(obj) <= set(model.model_fields)
        seen.add(tuple(obj))
    assert len(seen) > 1 or model is Flat              # optional keys were both present and absent


# ----------------------------------------------------------------------------- 2. near-misses
GOOD = {"name": "n", "count": 3, "ratio": 1.5, "ok": True, "kind": "ab", "note": None}


def _doc(**changes):
    d = dict(GOOD)
    d.update(changes)
    return json.dumps(d, separators=(",", ":"))


@pytest.mark.parametrize("name,text", [
    ("wrong key", _doc().replace('"count"', '"counts"')),
    ("misspelt key", _doc().replace('"ratio"', '"ratlo"')),
    ("keys out of order", '{"count":3,"name":"n","ratio":1.5,"ok":true,"kind":"ab"}'),
    ("missing required key", '{"name":"n","ratio":1.5,"ok":true,"kind":"ab"}'),
    ("missing last required key", '{"name":"n","count":3,"ratio":1.5,"ok":true}'),
    ("extra key", _doc()[:-1] + ',"extra":1}'),
    ("extra key in front", '{"extra":1,' + _doc()[1:]),
    ("duplicate key", '{"name":"n","name":"n",' + _doc()[12:]),
    ("enum off by one character", _doc(kind="ac")),
    ("enum too long", _doc(kind="abc")),
    ("enum prefix", _doc(kind="")),
    ("enum case", _doc(kind="A")),
    ("1.0 for an integer", _doc().replace('"count":3', '"count":3.0')),
    ("exponent for an integer", _doc().replace('"count":3', '"count":3e0')),
    ("string for a number", _doc(ratio="1.5")),
    ("number for a string", _doc(name=1)),
    ("null for a required string", _doc(name=None)),
    ("1 for a boolean", _doc(ok=1)),
    ("trailing comma", _doc()[:-1] + ",}"),
    ("comma in front", "{," + _doc()[1:]),
    ("byte after the final brace", _doc() + " "),
    ("newline after the final brace", _doc() + "\n"),
    ("second object", _doc() + "{}"),
    ("whitespace before the object", " " + _doc()),
    ("too much whitespace", _doc().replace(":3", ":" + " " * (S.SCHEMA_MAX_WS + 1) + "3")),
    ("too much whitespace after a comma", _doc().replace(',"count"', "," + " " * (S.SCHEMA_MAX_WS + 1) + '"count"')),
    ("array for an object", "[" + _doc() + "]"),
    ("leading zero", _doc().replace('"count":3', '"count":03')),
    ("raw control byte in a string", _doc().replace('"n"', '"\x01"')),
])
def test_near_misses_are_rejected(dfas, name, text):
    dfa = dfas[Flat]
    assert S.accepts(dfa, _doc().encode()) and S.accepts(dfa, json.dumps(GOOD).encode())
    assert S.accepts(dfa, _doc().replace(":3", ":" + " " * S.SCHEMA_MAX_WS + "3").encode())
    assert not S.accepts(dfa, text.encode("utf-8")), name


def test_nested_near_misses(dfas):
    dfa = dfas[Nested]
    ok = '{"title":"t","items":[{"id":1,"tag":"yy","pos":{"x":1,"y":2.5}},{"id":2,"tag":"x"}],"level":"low","version":3}'
    assert S.accepts(dfa, ok.encode())
    for bad in (ok.replace('"yy"', '"y"'), ok.replace('"x":1,"y":2.5', '"y":2.5,"x":1'), ok.replace('"x":1,', ""),
                ok.replace('{"id":2,"tag":"x"}', '{"id":2,"tag":"x"},'), ok.replace('"level":"low"', '"level":"mid"'),
                ok.replace('"version":3', '"version":4'), ok.replace('"version":3', '"version":3.0'),
                ok.replace('"items":[', '"items":[,'), ok.replace('"items":[', '"items":{').replace("],", "},"),
                ok.replace('"tag":"x"', '"tag":"x","pos":null,"more":1'), ok.replace('"level":"low",', '"level":"low",,')):
        assert bad != ok and not S.accepts(dfa, bad.encode()), bad
    for good in (ok.replace('"level":"low",', ""), ok.replace('"level":"low"', '"level":null'),
                 ok.replace('"tag":"x"', '"tag":"x","pos":null'), ok.replace(',"version":3', ""),
                 ok.replace('"yy"', '"naïve"'), ok.replace('"yy"', '"na\\u00efve"'),
                 '{"title":"","items":[]}', '{ "title" : "" , "items" : [ ] }'):
        assert S.accepts(dfa, good.encode()), good


# ----------------------------------------------------------------------------- 3. live prefixes
@pytest.mark.parametrize("model", MODELS)
def test_every_prefix_of_an_accepted_document_is_live(dfas, model):
    rng = random.Random(3)
    dfa = dfas[model]
    for _ in range(40):
        data = json.dumps(random_instance(model, rng).model_dump(mode="json"), ensure_ascii=False).encode("utf-8")
        s = dfa.start
        for i, b in enumerate(data):
            assert not dfa.state_flags[s] & S.STATE_ACCEPT, (data, i)       # the end state only at the end
            s = S.step(dfa, s, b)
            assert s != S.DEAD, (data[:i + 1], i)
        assert S.walk(dfa, dfa.start, data) == s
        assert dfa.state_flags[s] & S.STATE_ACCEPT
        assert all(S.step(dfa, s, b) == S.DEAD for b in range(256))        # no byte after the top-level '}'
    assert S.step(dfa, S.DEAD, 0x7B) == S.DEAD


def test_table_shape_and_flags(dfas):
    for model, dfa in dfas.items():
        n, c = dfa.trans.shape
        assert dfa.trans.dtype == np.uint16 and dfa.byte_class.dtype == np.uint8 and dfa.state_flags.dtype == np.uint8
        assert dfa.byte_class.shape == (256,) and dfa.state_flags.shape == (n,) and int(dfa.byte_class.max()) == c - 1
        assert ((dfa.trans < n) | (dfa.trans == S.DEAD)).all() and 0 <= dfa.start < n <= S.SCHEMA_MAX_STATES
        assert len({tuple(col) for col in dfa.trans.T}) == c                  # bytes with identical columns are merged
        assert (dfa.state_flags & S.STATE_ACCEPT).sum() == 1
        plain = [b for b in range(0x20, 0x7F) if b not in (0x22, 0x5C)]
        for s in range(n):
            loops = all(dfa.trans[s, dfa.byte_class[b]] == s for b in plain)
            assert bool(dfa.state_flags[s] & S.STATE_PLAIN) == loops
        assert (dfa.state_flags & S.STATE_PLAIN).any()
    # the whitespace cap is what the states pay for
    sizes = [S.compile_schema(REPORT_SCHEMA, ws).n_states for ws in (0, 1, S.SCHEMA_MAX_WS, S.SCHEMA_MAX_WS + 1)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    assert S.SCHEMA_MAX_WS >= 1
    report = S.compile_schema(REPORT_SCHEMA)
    assert report.trans.nbytes <= 72 * 1024, "the report schema's table is meant to fit the kernel's LDS staging buffer"
    # compiling is deterministic: the cache key is the schema's text
    again = S.compile_schema(json.loads(S.canonical(REPORT_SCHEMA)))
    assert np.array_equal(again.trans, report.trans) and np.array_equal(again.byte_class, report.byte_class)


def test_report_schema_matches_what_the_parser_reads():
    from vision_inspection_system_amd.response_parsing import parse_json_robust, validate_and_fix_result
    dfa = S.compile_schema(REPORT_SCHEMA)
    dist = distance_to_accept(dfa)
    rng = random.Random(5)
    own = {"timestamp", "analysis_failed", "failure_reason", "defect_id"}
    assert not own & set(REPORT_SCHEMA["properties"]) and not own & set(REPORT_SCHEMA["properties"]["defects"]["items"]["properties"])
    assert set(REPORT_SCHEMA["properties"]) <= set(VLMAnalysisResult.model_fields)
    for _ in range(100):
        data, s = random_walk(dfa, rng, dist, wander=rng.choice([0, 80, 200]))
        assert dfa.state_flags[s] & S.STATE_ACCEPT
        obj = _strict_loads(data.decode("utf-8"))
        assert S.validate(REPORT_SCHEMA, obj)
        assert parse_json_robust(data.decode("utf-8")) == obj
        for d in obj["defects"]:
            d.pop("bbox", None)             # the schema does not promise BoundingBox's range validators
        fixed = validate_and_fix_result(obj)
        VLMAnalysisResult(**fixed)


# ----------------------------------------------------------------------------- 4. refused schemas
OBJ = {"type": "object", "properties": {"a": {"type": "integer"}}, "required": ["a"]}


def _with(prop):
    return {"type": "object", "properties": {"a": prop}, "required": ["a"]}


def _big_schema():
    keys = [f"a_rather_long_property_name_{i:03d}" for i in range(110)]
    return {"type": "object", "required": keys, "properties": {k: {"type": "string"} for k in keys}}


@pytest.mark.parametrize("schema,needle", [
    (_with({"type": "string", "pattern": "^a"}), "pattern"),
    (_with({"type": "string", "minLength": 1}), "minLength"),
    (_with({"type": "number", "minimum": 0}), "minimum"),
    (_with({"oneOf": [{"type": "string"}, {"type": "null"}]}), "oneOf"),
    (dict(OBJ, patternProperties={"^x": {}}), "patternProperties"),
    (_with({"type": "array", "items": {"type": "integer"}, "minItems": 1}), "minItems"),
    (_with({"type": "array", "items": {"type": "integer"}, "maxItems": 3}), "maxItems"),
    (dict(OBJ, additionalProperties=True), "additionalProperties"),
    ({"type": "object", "properties": {"n": {"$ref": "#/$defs/N"}},
      "$defs": {"N": {"type": "object", "properties": {"next": {"anyOf": [{"$ref": "#/$defs/N"}, {"type": "null"}]}}}}}, "recursive"),
    (_with({"anyOf": [{"type": "string"}, {"enum": ["x", "y"]}]}), "ambiguous"),
    (_with({"anyOf": [{"type": "integer"}, {"type": "number"}]}), "ambiguous"),
    ({"type": "array", "items": OBJ}, "top level"),
    ({"type": "string"}, "top level"),
    ({}, "top level"),
    (_with({}), "type"),
    (_with({"$ref": "#/$defs/Missing"}), "unresolved"),
    (_with({"$ref": "other.json#/x"}), "$ref"),
    (_with({"type": "array"}), "items"),
    (_with({"type": "frob"}), "frob"),
    (_with({"enum": [[1]]}), "enum"),
    (_big_schema(), "states"),
])
def test_unsupported_schemas_are_value_errors_naming_the_cause(schema, needle):
    with pytest.raises(ValueError) as e:
        S.compile_schema(schema)
    assert needle in str(e.value), str(e.value)
    assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS), str(e.value)
    if needle == "states":
        assert str(S.SCHEMA_MAX_STATES) in str(e.value) and re.search(r"compiles to \d+ states", str(e.value))


def test_client_compiles_the_schema_before_any_model_loads():
    from vision_inspection_system_amd import client as C
    c = C.LocalVLMClient()
    msgs = [{"role": "user", "content": "hi"}]

    def rf(schema, **more):
        return {"type": "json_schema", "json_schema": {"name": "x", "schema": schema, **more}}

    for ok in (rf(OBJ), rf(OBJ, strict=True), rf(OBJ, strict=False), rf(Nested.model_json_schema()), rf(REPORT_SCHEMA),
               {"type": "json_schema", "json_schema": {"schema": OBJ}}):
        with pytest.raises(FileNotFoundError):          # valid: gets as far as loading the (missing) model
            c.chat.completions.create(model="no/such-model", messages=msgs, response_format=ok)
        with pytest.raises(FileNotFoundError):
            c.complete_many("no/such-model", [msgs], response_format=ok)
    for bad in (rf({}), rf(_with({"type": "string", "pattern": "a"})), rf({"type": "array", "items": OBJ}),
                rf("object"), {"type": "json_schema"}, {"type": "json_schema", "json_schema": OBJ},
                {"type": "json_schema", "schema": OBJ}, rf(OBJ, strict="yes"), rf(OBJ, grammar="x")):
        with pytest.raises(ValueError) as e:
            c.chat.completions.create(model="no/such-model", messages=msgs, response_format=bad)
        assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS), str(e.value)
        with pytest.raises(ValueError):
            c.complete_many("no/such-model", [msgs], response_format=bad)
    # compiled once per schema text; the order of the properties is part of it (it is the order of the reply's keys)
    a = C.schema_of(rf(OBJ))
    b = C.schema_of(rf(json.loads(json.dumps(OBJ))))
    assert a is b and isinstance(a, S.SchemaDFA)
    two = {"type": "object", "properties": {"a": {"type": "null"}, "b": {"type": "null"}}}
    swapped = {"type": "object", "properties": {"b": {"type": "null"}, "a": {"type": "null"}}}
    assert S.accepts(C.schema_of(rf(two)), b'{"a":null,"b":null}') and not S.accepts(C.schema_of(rf(swapped)), b'{"a":null,"b":null}')
    assert C.schema_of(None) is None and C.schema_of({"type": "json_object"}) is None and C.schema_of({"type": "text"}) is None
    # json_mode_of keeps its results
    assert C.json_mode_of(None) is False and C.json_mode_of({"type": "text"}) is False
    assert C.json_mode_of({"type": "json_object"}) is True
    with pytest.raises(ValueError):
        C.json_mode_of(rf(OBJ))


def test_engine_keyword_checks_need_no_gpu():
    from vision_inspection_system_amd.json_mode import check_schema
    dfa = S.compile_schema(OBJ)
    check_schema(False, None)
    check_schema(True, None)
    check_schema(False, dfa)
    with pytest.raises(ValueError):
        check_schema(True, dfa)
    with pytest.raises(ValueError):
        check_schema(False, OBJ)            # the engines take the compiled form


# ----------------------------------------------------------------------------- 5. constants shared with the kernel
def test_constants_match_the_kernel_and_the_binding():
    src = open(os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "schema_mask.hip")).read()
    for name, val in (("SM_MAX_STATES", S.SCHEMA_MAX_STATES), ("SM_MAX_CLASSES", S.SCHEMA_MAX_CLASSES), ("SM_DEAD", S.DEAD),
                      ("SM_SLOT_INTS", S.SLOT_INTS), ("SM_STATE_INTS", S.STATE_INTS), ("SM_COUNT", S.COUNT_WORD),
                      ("SM_TICKET", S.TICKET_WORD), ("SM_HEADER_INTS", S.HEADER_INTS), ("SM_FLAG_EOS", G.FLAG_EOS),
                      ("SM_FLAG_PLAIN", G.FLAG_PLAIN), ("SM_STATE_ACCEPT", S.STATE_ACCEPT), ("SM_STATE_PLAIN", S.STATE_PLAIN)):
        assert re.search(rf"#define {name} {val}\s", src), name
    enum = re.search(r"enum \{ (SW_STATE[^}]*) \};", src).group(1)
    assert [n.strip() for n in enum.split(",")] == ["SW_STATE", "SW_ERR", "SW_POS", "SW_ANCHOR"]
    assert (S.STATE, S.ERR, S.POS, S.ANCHOR) == (0, 1, 2, 3)
    # one state layout for both masks: the engines reset and read either through the same [slots, 32] rows
    assert (S.SLOT_INTS, S.STATE_INTS, S.COUNT_WORD, S.TICKET_WORD) == (G.SLOT_INTS, G.STATE_INTS, G.COUNT_WORD, G.TICKET_WORD)
    assert S.SCHEMA_MAX_STATES < S.DEAD
    from vision_inspection_system_amd import hip
    header = open(os.path.join(ROOT, "include", "vis_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    proto = re.search(r"\bvis_schema_mask\s*\(([^)]*)\)\s*;", header).group(1)
    want = "".join("p" if "*" in p or "vis_stream_t" in p else "i" for p in proto.split(","))
    assert hip._SIGS["vis_schema_mask"] == want and len(want) == 20
    assert "vis_schema_mask" in hip.exported_symbols()


@pytest.fixture(scope="module")
def lib():
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    from vision_inspection_system_amd import hip
    return hip.load()


def test_entry_point_rejects_bad_arguments_without_gpu(lib):
    V, B, T = 152064, 4, 64
    nw = (V + 63) // 64
    p = 4096     # any aligned non-null address: nothing is launched when an argument is refused

    def mask(state=p, tokens=p, T=T, step=p, off=p, data=p, flags=p, eos=p, n_eos=2, V=V, allow=p, ld=nw, header=p, trans=p,
             cls=p, sflags=p, cap_states=S.SCHEMA_MAX_STATES, cap_classes=256, batch=B):
        return lib.vis_schema_mask(state, tokens, T, step, off, data, flags, eos, n_eos, V, allow, ld, header, trans, cls,
                                   sflags, cap_states, cap_classes, batch, None)

    for bad in (dict(state=None), dict(tokens=None), dict(step=None), dict(off=None), dict(data=None), dict(flags=None),
                dict(eos=None), dict(allow=None), dict(header=None), dict(trans=None), dict(cls=None), dict(sflags=None),
                dict(V=0), dict(V=262145), dict(T=0), dict(n_eos=0), dict(n_eos=65), dict(batch=0), dict(batch=65),
                dict(ld=nw - 1), dict(allow=p + 4), dict(data=p + 2), dict(state=p + 2), dict(header=p + 2), dict(trans=p + 8),
                dict(cap_states=0), dict(cap_states=S.SCHEMA_MAX_STATES + 1), dict(cap_classes=0), dict(cap_classes=257),
                dict(cap_states=3, cap_classes=1)):
        assert mask(**bad) == 1, bad


# ----------------------------------------------------------------------------- 6. allowed_mask against a per-token walk
def _brute(dfa, state, table):
    ok = np.zeros(table.vocab, dtype=bool)
    for t, b in enumerate(table.tokens):
        if table.flags[t] & G.FLAG_EOS:
            ok[t] = bool(dfa.state_flags[state] & S.STATE_ACCEPT)
        elif b:
            ok[t] = S.walk(dfa, state, b) != S.DEAD
    err = not ok.any()
    if err:
        ok[table.eos_ids] = True
    return ok, err


def _tables():
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    out = [("bytes", G.build_token_table(ByteTokenizer(300, 290, 291, 292, [293, 295]), 300, [293, 295]))]
    import importlib.util
    assert importlib.util.find_spec("tokenizers") is not None, "the real vocabularies need the tokenizers package"
    from vision_inspection_system_amd.tokenizer import HFTokenizer, LlamaHFTokenizer
    for name in sorted(os.listdir(HF)):
        if not os.path.exists(os.path.join(HF, name, "tokenizer.json")):
            continue
        if "mllama" in name:
            tok = LlamaHFTokenizer(os.path.join(HF, name), 510, [501])
            out.append((name, G.build_token_table(tok, 513, list(tok.eos_ids))))
        else:
            out.append((name, G.build_token_table(HFTokenizer(os.path.join(HF, name), 500, 501, 502, [503, 505]), 520, [503, 505])))
    assert len(out) >= 3
    return out


def test_allowed_mask_equals_a_per_token_walk(dfas):
    rng = random.Random(21)
    for name, table in _tables():
        for model in (Nested, VLMAnalysisResult):
            dfa = dfas[model]
            dist = distance_to_accept(dfa)
            states = {dfa.start, int(np.flatnonzero(dfa.state_flags & S.STATE_ACCEPT)[0])}
            states |= set(np.flatnonzero(dfa.state_flags & S.STATE_PLAIN)[:2].tolist())
            for _ in range(12):
                cut = rng.randint(1, 120)
                states.add(random_walk(dfa, rng, dist, wander=200, stop_at=lambda s, out: len(out) >= cut)[1])
            for s in sorted(states):
                ok, err = S.allowed(dfa, [s, 0], table)
                want, werr = _brute(dfa, s, table)
                assert np.array_equal(ok, want) and err == werr, (name, model.__name__, s)
                words = S.allowed_mask(dfa, s, table)
                assert words.dtype == np.uint64 and len(words) == (table.vocab + 63) // 64
                bits = np.unpackbits(words.view(np.uint8), bitorder="little")
                assert np.array_equal(bits[:table.vocab].astype(bool), want) and not bits[table.vocab:].any()
            ok, err = S.allowed(dfa, [dfa.start, 1], table)               # the error state: EOS ids only
            assert err and ok.nonzero()[0].tolist() == table.eos_ids.tolist()


def test_advance_follows_the_byte_walk():
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    table = G.build_token_table(ByteTokenizer(300, 290, 291, 292, [293, 295]), 300, [293, 295])
    dfa = S.compile_schema(Flat.model_json_schema())
    doc = json.dumps(dict(GOOD, name="é😀"), ensure_ascii=False).encode("utf-8")
    st = S.initial_state(dfa)
    for b in doc:
        ok, err = S.allowed(dfa, st, table)
        assert not err and ok[b] and not ok[293] and not ok[256]
        assert ok.sum() == sum(S.step(dfa, st[0], c) != S.DEAD for c in range(256))
        S.advance(dfa, st, b, table)
        assert not st[1]
    ok, err = S.allowed(dfa, st, table)
    assert dfa.state_flags[st[0]] & S.STATE_ACCEPT and not err and ok.nonzero()[0].tolist() == [293, 295]
    S.advance(dfa, st, 293, table)
    assert not st[1]
    for bad in (293, ord("]"), 256, 300, -1):       # EOS before the end, a rejected token, an empty one, ids out of range
        s = S.initial_state(dfa)
        S.advance(dfa, s, ord("{"), table)
        before = s[0]
        S.advance(dfa, s, bad, table)
        assert s == [before, 1]
        ok, err = S.allowed(dfa, s, table)
        assert err and ok.nonzero()[0].tolist() == [293, 295]
    # a vocabulary without '"' cannot start the first key: nothing allowed after '{'
    class NoQuote:
        def token_bytes(self, t):
            return b"" if t == ord('"') or t > 255 else bytes([t])
    nq = G.build_token_table(NoQuote(), 300, [293, 295])
    s = S.initial_state(dfa)
    S.advance(dfa, s, ord("{"), nq)
    for _ in range(S.SCHEMA_MAX_WS):
        ok, err = S.allowed(dfa, s, nq)
        assert not err and set(ok.nonzero()[0].tolist()) == {0x20, 0x09, 0x0A, 0x0D}
        S.advance(dfa, s, 0x20, nq)
    ok, err = S.allowed(dfa, s, nq)
    assert err and ok.nonzero()[0].tolist() == [293, 295]


# ----------------------------------------------------------------------------- 7. agents
def _done(value):
    from concurrent.futures import Future
    f = Future()
    f.set_result(value)
    return f


def test_agents_send_the_report_schema_only_when_asked(monkeypatch):
    from vision_inspection_system_amd import agents
    from vision_inspection_system_amd.client import CannedResponseClient, schema_of
    from vision_inspection_system_amd.schemas import REPORT_RESPONSE_FORMAT

    class Many(CannedResponseClient):
        def complete_many(self, model, batch, temperature=None, max_tokens=None, **kw):
            return [self._complete(model, m, temperature, max_tokens, **kw) for m in batch]

    assert REPORT_RESPONSE_FORMAT["json_schema"]["schema"] is REPORT_SCHEMA
    assert isinstance(schema_of(REPORT_RESPONSE_FORMAT), S.SchemaDFA)
    obj = {"type": "json_object"}
    for schema_env, mode_env, want in ((None, None, None), ("0", None, None), (None, "1", obj), ("0", "1", obj),
                                       ("1", None, REPORT_RESPONSE_FORMAT), ("1", "1", REPORT_RESPONSE_FORMAT),
                                       ("1", "0", REPORT_RESPONSE_FORMAT)):
        for name, v in (("VIS_JSON_SCHEMA", schema_env), ("VIS_JSON_MODE", mode_env)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        assert agents.json_mode_kwargs() == ({} if want is None else {"response_format": want})
        for cls in (agents.VLMInspectorAgent, agents.VLMAuditorAgent):      # analysis and verify requests
            agent = cls.__new__(cls)
            agent.client, agent.model_id, agent.temperature, agent.max_tokens = CannedResponseClient(reply="{}"), "m", 0.1, 64
            agent.logger, agent.nickname = agents._logger("t"), "t"
            assert agent._call_with_retry([{"role": "user", "content": "x"}]) == "{}"
            assert agent.client.calls[-1]["response_format"] == want
            agent.client = Many(reply="{}")
            agents._many(agent, ["a.jpg"], [None], prepared=[_done([{"role": "user", "content": "x"}])])
            assert agent.client.calls[-1]["response_format"] == want
            agent.client = CannedResponseClient(reply="OK")                 # the ping never carries it
            assert agent.health_check() is True
            assert agent.client.calls[-1]["response_format"] is None and agent.client.calls[-1]["max_tokens"] == 10
