"""Schema-constrained decoding on MI355X: vis_schema_mask against json_schema (allowed / advance) bit for bit, and the
engines' / client's json_schema replies replayed through the CPU DFA token by token and judged by pydantic."""
import json
import os
import random

import numpy as np
import pytest
import torch

from helpers import load_golden
from schema_cases import AllOptional, Closed, Flat, Nested, distance_to_accept, random_walk
from test_json_mode_gpu import _Vocab, _dev_table, _qwen_engine
from vision_inspection_system_amd import hip
from vision_inspection_system_amd import json_grammar as G
from vision_inspection_system_amd import json_schema as S
from vision_inspection_system_amd.schemas import REPORT_SCHEMA

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HF = os.path.join(HERE, "golden", "hf_dirs")
SCHEMAS = {"flat": Flat.model_json_schema(), "nested": Nested.model_json_schema(), "report": REPORT_SCHEMA,
           "optional": AllOptional.model_json_schema(), "closed": Closed.model_json_schema()}
MODEL_OF = {"flat": Flat, "nested": Nested, "optional": AllOptional, "closed": Closed}
CLOSED_MAX = 28 + 13 * S.SCHEMA_MAX_WS + 1      # the longest Closed document, whitespace at the cap everywhere, and EOS


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


@pytest.fixture(scope="module")
def dfas():
    return {k: S.compile_schema(v) for k, v in SCHEMAS.items()}


class _Dev:
    """A DFA in fixed-capacity device tables, as SchemaBuffers holds it."""

    def __init__(self, cap_states=S.SCHEMA_MAX_STATES, cap_classes=S.SCHEMA_MAX_CLASSES):
        self.header = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.trans = torch.full((cap_states, cap_classes), -1, dtype=torch.int16, device="cuda")
        self.cls = torch.zeros(256, dtype=torch.uint8, device="cuda")
        self.flags = torch.zeros(cap_states, dtype=torch.uint8, device="cuda")

    def load(self, dfa):
        n, c = dfa.trans.shape
        self.trans.view(-1)[:n * c].copy_(torch.from_numpy(dfa.trans.reshape(-1).view(np.int16).copy()))
        self.cls.copy_(torch.from_numpy(dfa.byte_class.copy()))
        self.flags[:n].copy_(torch.from_numpy(dfa.state_flags.copy()))
        self.header.copy_(torch.tensor([n, c, dfa.start, 0], dtype=torch.int32))
        return self

    def args(self):
        return self.header, self.trans, self.cls, self.flags


def _prefixes(dfa, rng, n=10, limit=250):
    """Byte prefixes reaching: start, mid-key, in a string with a UTF-8 sequence open, in an enum, whitespace at the cap, the
    accepting state, and seeded random cuts."""
    dist = distance_to_accept(dfa)
    whole, s = random_walk(dfa, rng, dist, wander=0)
    assert dfa.state_flags[s] & S.STATE_ACCEPT
    out = [b"", b'{"', whole, b"{" + b" " * S.SCHEMA_MAX_WS]
    doc, _ = random_walk(dfa, rng, dist, wander=150)
    out += [doc[:rng.randint(1, len(doc))] for _ in range(n)]
    # a string body with an open UTF-8 sequence, and the middle of an enum literal, found by walking
    for want in ("utf8", "plain"):
        def hit(s, o, want=want):
            if want == "plain":
                return bool(dfa.state_flags[s] & S.STATE_PLAIN)
            return len(o) > 0 and o[-1] >= 0xC2 and S.step(dfa, s, 0x22) == S.DEAD
        for _ in range(50):
            p, s = random_walk(dfa, rng, dist, wander=400, stop_at=hit)
            if hit(s, p):
                out.append(p)
                break
    return [p for p in out if len(p) <= limit and S.walk(dfa, dfa.start, p) != S.DEAD]


def _run(prefixes, table, dt, dev, T=256, pending=None):
    """One launch for len(prefixes) rows.  Row r holds the single-byte tokens of prefixes[r]; the slot the launch reads was
    written ``pending[r]`` tokens ago (default: everything is pending, anchored at position 0 in the start state)."""
    B, V = len(prefixes), table.vocab
    tokens = torch.zeros((B, T), dtype=torch.int32)
    state = torch.zeros((B, S.STATE_INTS), dtype=torch.int32)
    step = torch.zeros(B, dtype=torch.int32)
    for r, (p, dfa) in enumerate(prefixes):
        tokens[r, :len(p)] = torch.tensor(list(p), dtype=torch.int32)
        step[r] = len(p)
        k = len(p) if pending is None else min(pending[r], len(p))
        rd = (len(p) & 1) * S.SLOT_INTS
        if len(p) or pending is not None:
            state[r, rd + S.STATE] = S.walk(dfa, dfa.start, p[:len(p) - k])
            state[r, rd + S.ANCHOR] = 1
            state[r, rd + S.POS] = len(p) - k
    tokens, state, step = tokens.cuda(), state.cuda(), step.cuda()
    allow = torch.full((B, (V + 63) // 64 + 3), -1, dtype=torch.int64, device="cuda")
    hip.schema_mask(state, tokens, step, *dt, allow, *dev.args())
    torch.cuda.synchronize()
    first = (state.cpu(), allow.cpu())
    hip.schema_mask(state, tokens, step, *dt, allow, *dev.args())       # a repeated launch at the same step
    torch.cuda.synchronize()
    assert torch.equal(state.cpu(), first[0]) and torch.equal(allow.cpu(), first[1])
    return first


def _check(prefixes, table, state, allow):
    nw = (table.vocab + 63) // 64
    for r, (p, dfa) in enumerate(prefixes):
        st = [S.walk(dfa, dfa.start, p), 0]
        ok, err = S.allowed(dfa, st, table)
        wr = ((len(p) + 1) & 1) * S.SLOT_INTS
        got = state[r, wr:wr + 4].tolist()
        assert got == [st[0], int(err), len(p), 1], (p, got, st, err)
        assert state[r, S.COUNT_WORD] == 0 and state[r, S.TICKET_WORD] == 0
        assert np.array_equal(allow[r, :nw].numpy(), G.mask_words(ok)), p
        assert np.array_equal(allow[r, :nw].numpy().view(np.uint64), S.allowed_mask(dfa, st[0], table)) or err
        assert (allow[r, nw:] == -1).all(), "wrote past the row's words"


@pytest.fixture(scope="module")
def big(device):
    V = 152064 - 5                      # not a multiple of 64
    table = G.build_token_table(_Vocab(V, seed=11), V, [V - 3, V - 1])
    return table, _dev_table(table)


@pytest.mark.parametrize("name", list(SCHEMAS))
def test_mask_equals_reference_synthetic_vocab(big, dfas, name):
    """Multi-byte tokens that cross structural boundaries (_Vocab's JSON-heavy strings), V not divisible by 64."""
    table, dt = big
    dfa = dfas[name]
    dev = _Dev().load(dfa)
    rng = random.Random(len(name))
    ps = [(p, dfa) for p in _prefixes(dfa, rng)]
    if (dfa.state_flags & S.STATE_PLAIN).any():             # a schema with a string: some row sits in its body
        assert any(dfa.state_flags[S.walk(dfa, dfa.start, p)] & S.STATE_PLAIN for p, _ in ps)
    for p in ps[:6]:                                            # B = 1
        _check([p], table, *_run([p], table, dt, dev))
    for B in (7, 64):                                           # odd B and the cap
        rows = [ps[r % len(ps)] for r in range(B)]
        _check(rows, table, *_run(rows, table, dt, dev))
    # folding 0 / 1 / several pending tokens gives the same state and row
    rows = [ps[r % len(ps)] for r in range(12)]
    for pend in ([0] * 12, [1] * 12, [r % 5 for r in range(12)]):
        _check(rows, table, *_run(rows, table, dt, dev, pending=pend))
    assert table.vocab % 64 != 0


def test_table_read_through_l2_when_it_does_not_fit_lds(big):
    """A schema whose table exceeds the LDS staging buffer takes the kernel's global-memory path: same rows."""
    table, dt = big
    keys = {f"property_{i:02d}": {"enum": ["alpha", "beta", "gamma"]} for i in range(40)}
    dfa = S.compile_schema({"type": "object", "properties": keys, "required": list(keys)[::3]})
    assert dfa.trans.nbytes > 72 * 1024
    dev = _Dev().load(dfa)
    rng = random.Random(2)
    ps = [(p, dfa) for p in _prefixes(dfa, rng, n=6, limit=2000)]
    _check(ps, table, *_run(ps, table, dt, dev, T=2048))


def test_header_outside_the_capacity_is_an_error_state(big, dfas):
    table, dt = big
    dfa = dfas["flat"]
    dev = _Dev(cap_states=(dfa.n_states + 7) & ~7, cap_classes=dfa.n_classes).load(dfa)
    _check([(b'{"', dfa)], table, *_run([(b'{"', dfa)], table, dt, dev))
    eos_only = G.mask_words(np.isin(np.arange(table.vocab), table.eos_ids))
    for bad in ([dfa.n_states + 8, dfa.n_classes, dfa.start, 0], [dfa.n_states, dfa.n_classes + 1, dfa.start, 0],
                [dfa.n_states, dfa.n_classes, dfa.n_states, 0], [0, 0, 0, 0], [-1, -1, -1, 0]):
        dev.header.copy_(torch.tensor(bad, dtype=torch.int32))
        state, allow = _run([(b"", dfa)], table, dt, dev)
        assert np.array_equal(allow[0, :len(eos_only)].numpy(), eos_only), bad
        assert state[0, S.SLOT_INTS + S.ERR] == 1


@pytest.mark.parametrize("name,V", [("qwen2vl_tiny", 520), ("mllama_tiny", 513)])
def test_mask_and_fold_follow_the_reference_step_by_step(dfas, name, V):
    """The real vocabularies: random logits, the masked Gumbel-max pick, the next launch folds it."""
    pytest.importorskip("tokenizers")
    from vision_inspection_system_amd.tokenizer import HFTokenizer, LlamaHFTokenizer
    tok = HFTokenizer(os.path.join(HF, name), 500, 501, 502, [503, 505]) if name == "qwen2vl_tiny" else \
        LlamaHFTokenizer(os.path.join(HF, name), 510, [501])
    eos = [503, 505] if name == "qwen2vl_tiny" else list(tok.eos_ids)
    table = G.build_token_table(tok, V, eos)
    dt = _dev_table(table)
    dfa = dfas["nested"]
    dev = _Dev().load(dfa)
    B, T, P0 = 5, 160, 3
    state = torch.zeros((B, S.STATE_INTS), dtype=torch.int32, device="cuda")
    tokens = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    step = torch.full((B,), P0, dtype=torch.int32, device="cuda")
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    allow = torch.zeros((B, (V + 63) // 64), dtype=torch.int64, device="cuda")
    wv = torch.empty(256 * B, dtype=torch.float32, device="cuda")
    wi = torch.empty(256 * B, dtype=torch.int32, device="cuda")
    ref = [S.initial_state(dfa) for _ in range(B)]
    g = torch.Generator(device="cuda").manual_seed(3)
    for it in range(120):
        hip.schema_mask(state, tokens, step, *dt, allow, *dev.args())
        st, al, n = state.cpu(), allow.cpu().numpy(), P0 + it
        for b in range(B):
            ok, err = S.allowed(dfa, ref[b], table)
            assert not err
            wr = ((n + 1) & 1) * S.SLOT_INTS
            assert st[b, wr:wr + 2].tolist() == ref[b], (it, b)
            assert np.array_equal(al[b], G.mask_words(ok)), (it, b)
        logits = torch.randn((B, V), generator=g, device="cuda") * 3
        hip.argmax_masked(logits, wv, wi, tokens, cur, step, allow, temperature=0.9, seed=it)
        picked = tokens[:, n].cpu().tolist()
        for b in range(B):
            assert S.allowed(dfa, ref[b], table)[0][picked[b]], (it, b, picked[b])
            S.advance(dfa, ref[b], picked[b], table)
            assert not ref[b][1]


# ----------------------------------------------------------------------------- engines
def _replay(dfa, schema, model, table, toks, eos_ids, what="", eos_in_output=False):
    """Every token was allowed by the CPU DFA at its step; a reply that reached the end is a document of the schema."""
    st = S.initial_state(dfa)
    for i, t in enumerate(toks):
        ok, err = S.allowed(dfa, st, table)
        assert not err and ok[t], (what, i, t, toks)
        S.advance(dfa, st, t, table)
        assert not st[1]
        if t in eos_ids:
            assert i == len(toks) - 1, (what, "tokens after EOS")
    data = b"".join(table.tokens[t] for t in toks)
    assert S.walk(dfa, dfa.start, data) == st[0] != S.DEAD, (what, data)
    done = bool(dfa.state_flags[st[0]] & S.STATE_ACCEPT)
    if done:
        obj = json.loads(data.decode("utf-8"))
        assert S.validate(schema, obj), (what, data)
        if model is not None:
            model.model_validate(obj)
    return done


def _table(eng):
    return eng._schema.table


def test_qwen_engine_paths(device, dfas):
    cfg, eng = _qwen_engine(device, decode_splits=4, max_batch=5)
    g = load_golden()
    ids = g["ids_a"].tolist()
    fr = [torch.from_numpy(g["frame_a"]).to(device)]
    eos = set(cfg.eos_ids)
    off = eng.generate(ids, fr, max_new_tokens=40, ignore_eos=True)
    jm = eng.generate(ids, fr, max_new_tokens=40, json_mode=True)
    assert eng.generate(ids, fr, max_new_tokens=40, ignore_eos=True, json_schema=None) == off
    with pytest.raises(ValueError):
        eng.generate(ids, fr, max_new_tokens=8, json_mode=True, json_schema=dfas["flat"])
    with pytest.raises(ValueError):
        eng.generate_batch([(ids, fr)] * 2, max_new_tokens=8, json_mode=True, json_schema=dfas["flat"])
    finished = 0
    for name in ("closed", "flat", "nested"):
        dfa = dfas[name]
        for temp, seed, extra in ((0.0, 0, {}), (0.9, 1, {}), (0.8, 2, {"top_p": 0.9}),
                                  (0.7, 3, {"repetition_penalty": 1.3, "frequency_penalty": 0.5, "logprobs": 3})):
            outs = {}
            for use_graph in (False, True):
                toks = eng.generate(ids, fr, max_new_tokens=120, temperature=temp, seed=seed, use_graph=use_graph,
                                    json_schema=dfa, **extra)
                assert eng.schema_on is False and eng.json_on is False
                outs[use_graph] = toks
                done = _replay(dfa, SCHEMAS[name], MODEL_OF[name], _table(eng), toks, eos, (name, temp, use_graph))
                assert done or name != "closed", (name, temp, toks)
                finished += done
                if "logprobs" in extra:
                    rec = eng.last_logprobs[0]
                    assert len(rec.token_logprobs) == len(toks) and all(len(t) == 3 for t in rec.top_ids)
            assert outs[False] == outs[True], (name, temp)
        # the batch: the same schema for every request, other requests next to it; per-request seeds
        reqs = [(ids, fr), ([256, 72, 105, 33, 90, 41], []), (ids, fr)]
        for temp, kw in ((0.0, {}), (0.9, {"seeds": [5, 6, 5], "top_p": 0.95})):
            res = {}
            for use_graph in (False, True):
                out = eng.generate_batch(reqs, max_new_tokens=120, temperature=temp, seed=4, use_graph=use_graph,
                                         json_schema=dfa, **kw)
                for i, t in enumerate(out):
                    finished += _replay(dfa, SCHEMAS[name], MODEL_OF[name], _table(eng), t, eos, (name, "batch", temp, i))
                res[use_graph] = out
            assert res[False] == res[True]
            if kw:
                assert res[True][0] == res[True][2]                 # its own seed: the reply does not depend on the slot
    assert finished > 0, "no reply reached the end of its document: the accepting path was never exercised"
    assert eng._schema.table is eng._json.table and eng._schema.off is eng._json.off       # one token table per engine
    # json_schema=None changes nothing: the unmasked and the JSON-mode tokens are what they were
    assert eng.generate(ids, fr, max_new_tokens=40, ignore_eos=True) == off
    assert eng.generate(ids, fr, max_new_tokens=40, json_mode=True) == jm


def test_two_schemas_in_succession_reuse_the_graph(device, dfas):
    cfg, eng = _qwen_engine(device, max_batch=4)
    g = load_golden()
    fr = [torch.from_numpy(g["frame_a"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fr), ([256, 72, 105, 33, 90, 41], []), (g["ids_a"].tolist(), fr)]
    eos = set(cfg.eos_ids)
    a = eng.generate_batch(reqs, max_new_tokens=100, temperature=0.0, json_schema=dfas["flat"])
    graphs = len(eng._graphs) if hasattr(eng, "_graphs") else None
    b = eng.generate_batch(reqs[::-1], max_new_tokens=100, temperature=0.0, json_schema=dfas["nested"])
    if graphs is not None:
        assert len(eng._graphs) == graphs, "the second schema captured a graph of its own"
    c = eng.generate_batch(reqs, max_new_tokens=100, temperature=0.0, json_schema=dfas["flat"])
    assert a == c
    for i, t in enumerate(a):
        _replay(dfas["flat"], SCHEMAS["flat"], Flat, _table(eng), t, eos, ("first", i))
    for i, t in enumerate(b):
        _replay(dfas["nested"], SCHEMAS["nested"], Nested, _table(eng), t, eos, ("second", i))
    _, fresh = _qwen_engine(device, max_batch=4)
    assert fresh.generate_batch(reqs[::-1], max_new_tokens=100, temperature=0.0, json_schema=dfas["nested"]) == b
    one = eng.generate(*reqs[0], max_new_tokens=100, json_schema=dfas["nested"])
    assert fresh.generate(*reqs[0], max_new_tokens=100, json_schema=dfas["nested"]) == one
    assert eng.generate(*reqs[0], max_new_tokens=100, json_schema=dfas["flat"]) == \
        fresh.generate(*reqs[0], max_new_tokens=100, json_schema=dfas["flat"])


def test_failure_is_reported(device, dfas):
    """A vocabulary without '"' cannot write the first key: EOS + the error bit, and the request fails."""
    from vision_inspection_system_amd.json_mode import JsonModeError
    cfg, eng = _qwen_engine(device, max_batch=2)

    class NoQuote:
        def token_bytes(self, t):
            return b"" if t == ord('"') or t > 255 else bytes([t])

    eng.tokenizer = NoQuote()
    g = load_golden()
    req = (g["ids_a"].tolist(), [torch.from_numpy(g["frame_a"]).to(device)])
    with pytest.raises(JsonModeError):
        eng.generate(*req, max_new_tokens=30, json_schema=dfas["flat"])
    out = eng.generate_batch([req, req], max_new_tokens=30, json_schema=dfas["flat"])
    assert all(isinstance(o, JsonModeError) for o in out)


def test_mllama_engine_paths(device, dfas):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=5)
    eng.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
    gm = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    frame = torch.from_numpy(gm["a_image"]).to(device)
    ids = gm["a_ids"].tolist()
    eos = set(cfg.eos_ids)
    off = eng.generate(ids, frame, max_new_tokens=30, stop_on_eos=False)
    jm = eng.generate(ids, frame, max_new_tokens=30, json_mode=True)
    with pytest.raises(ValueError):
        eng.generate(ids, frame, max_new_tokens=8, json_mode=True, json_schema=dfas["flat"])
    for name in ("closed", "flat"):
        dfa = dfas[name]
        for temp, extra in ((0.0, {}), (0.9, {}), (0.8, {"top_p": 0.9, "presence_penalty": 0.5, "logprobs": 2})):
            a = eng.generate(ids, frame, max_new_tokens=100, temperature=temp, seed=3, use_graph=False, json_schema=dfa, **extra)
            b = eng.generate(ids, frame, max_new_tokens=100, temperature=temp, seed=3, json_schema=dfa, **extra)
            assert a == b
            done = _replay(dfa, SCHEMAS[name], MODEL_OF[name], _table(eng), b, eos, ("mllama", name, temp))
            assert done or name != "closed", (name, temp, b)
            reqs = [(ids, frame), (gm["b_ids"].tolist(), torch.from_numpy(gm["b_image"]).to(device))] * 2 + [(ids, frame)]
            outs = {ug: eng.generate_batch(reqs, max_new_tokens=80, temperature=temp, seed=3, use_graph=ug, json_schema=dfa,
                                           **extra) for ug in (False, True)}
            assert outs[False] == outs[True]
            for i, t in enumerate(outs[True]):
                _replay(dfa, SCHEMAS[name], MODEL_OF[name], _table(eng), t, eos, ("mllama batch", name, temp, i))
    assert eng.generate(ids, frame, max_new_tokens=30, stop_on_eos=False) == off
    assert eng.generate(ids, frame, max_new_tokens=30, json_mode=True) == jm


# ----------------------------------------------------------------------------- client
@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_response_format_json_schema(device, tmp_path, model):
    from PIL import Image
    from vision_inspection_system_amd.client import LocalVLMClient, schema_of
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    p = tmp_path / "img.png"
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    url = encode_image_optimized(str(p), 256)
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": [{"type": "text", "text": "Inspect."},
                                         {"type": "image_url", "image_url": {"url": url}}]}]
    schema = Closed.model_json_schema()
    rf = {"type": "json_schema", "json_schema": {"name": "r", "schema": schema, "strict": True}}
    dfa = schema_of(rf)
    plain = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=CLOSED_MAX + 8)
    complete = 0
    for temp in (0.0, 0.9):
        r = c.chat.completions.create(model=model, messages=msgs, temperature=temp, max_tokens=CLOSED_MAX + 8, response_format=rf,
                                      logprobs=True, top_logprobs=4, seed=7)
        many = c.complete_many(model, [msgs, msgs], temperature=temp, max_tokens=CLOSED_MAX + 8, response_format=rf, logprobs=True, seed=7)
        for m in [r] + many:
            content = m.choices[0].logprobs.content
            assert len(content) == m.usage["completion_tokens"] > 0
            assert m.usage["prompt_tokens"] == plain.usage["prompt_tokens"]
            assert m.usage["total_tokens"] == m.usage["prompt_tokens"] + m.usage["completion_tokens"]
            data = bytes(b for e in content for b in e.bytes)
            s = S.walk(dfa, dfa.start, data)
            assert s != S.DEAD, data
            assert dfa.state_flags[s] & S.STATE_ACCEPT, data        # a Closed document always fits max_tokens
            complete += 1
            obj = json.loads(m.choices[0].message.content)
            assert S.validate(schema, obj)
            Closed.model_validate(obj)
        assert all(len(e.top_logprobs) == 4 for e in r.choices[0].logprobs.content)
        assert many[0].choices[0].message.content == many[1].choices[0].message.content
    assert complete > 0
    assert c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=CLOSED_MAX + 8).choices[0].message.content \
        == plain.choices[0].message.content
