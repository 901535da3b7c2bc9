"""pick.PickStage without a GPU: a stub engine on the CPU with the HIP launches replaced by recorders.  Which launches a
pick issues under every combination of the request switches (the table below is written out from the engines' _pick /
_gemv_pick as they stood before the two copies became one), what the prompt pass's pick adds, that a request's switches are
off again however the request ends, and what the decode-graph key depends on."""
import itertools
import os

import pytest
import torch

from vision_inspection_system_amd import hip, json_schema
from vision_inspection_system_amd.json_mode import JsonBuffers, SchemaBuffers
from vision_inspection_system_amd.pick import PickStage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, T, SLOTS, K = 320, 16, 3, 64
TRIPLE = (1.3, 0.5, -0.25)


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The buffer classes size their workspaces through the library's host-only queries."""
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    return hip.load()


class _Cfg:
    vocab, eos_ids = V, (V - 1,)


class _Tokenizer:
    def token_bytes(self, t: int) -> bytes:
        return bytes([t]) if t < 256 else b""


class Stub(PickStage):
    """What PickStage's docstring asks of an engine, on the CPU."""

    def __init__(self, tokenizer=None):
        dev = torch.device("cpu")
        self.cfg, self.max_batch, self.device = _Cfg(), SLOTS, dev
        self.tokens_b = torch.zeros((SLOTS, T), dtype=torch.int32, device=dev)
        self.logits_b = torch.zeros((SLOTS, V), dtype=torch.float32, device=dev)
        self.step_b = torch.zeros(SLOTS, dtype=torch.int32, device=dev)
        self.cur_b = torch.zeros(SLOTS, dtype=torch.int32, device=dev)
        self.ws_val = torch.zeros(2048, dtype=torch.float32, device=dev)
        self.ws_idx = torch.zeros(2048, dtype=torch.int32, device=dev)
        self.temperature, self.seed = 0.7, 11
        self.tokenizer = tokenizer
        self._init_pick_stage()


@pytest.fixture
def calls(monkeypatch):
    """Every launch the pick stage can issue, as (name, args, kwargs) in issue order."""
    log = []

    def rec(name):
        def f(*a, **kw):
            log.append((name, a, kw))
        return f

    for name in ("argmax", "argmax_masked", "gemv", "gemv_argmax", "gemv_argmax_masked", "sample", "penalize",
                 "penalty_prompt", "logprobs"):
        monkeypatch.setattr(hip, name, rec(name))

    def mask(name):
        def f(self, tokens, step, slot=0):
            B = tokens.shape[0] if tokens.dim() == 2 else 1
            log.append((name, (tokens, step, slot), {}))
            return self.allow[slot:slot + B]
        return f

    monkeypatch.setattr(JsonBuffers, "mask", mask("json_mask"))
    monkeypatch.setattr(SchemaBuffers, "mask", mask("schema_mask"))
    monkeypatch.setattr(JsonBuffers, "reset", lambda self, slot: log.append(("reset", (self, slot), {})))
    monkeypatch.setattr(SchemaBuffers, "load", lambda self, dfa, streams=(): log.append(("load", (dfa, tuple(streams)), {})))
    return log


def _names(log):
    return [c[0] for c in log]


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape


def _dfa():
    return json_schema.compile_schema({"type": "object", "properties": {"ok": {"type": "boolean"}}, "required": ["ok"],
                                       "additionalProperties": False})


def _switch(eng, pen: bool, smp: bool, mask: str):
    """The switches through the engine's own _begin_* calls, in the order a request switches them on; both mask buffers
    exist afterwards, whichever is on."""
    eng._begin_schema(False, _dfa())
    eng._begin_json(True)
    assert isinstance(eng._schema, SchemaBuffers) and type(eng._json) is JsonBuffers
    eng.schema_on, eng.json_on = mask == "schema", mask == "json"
    eng._begin_sampling(0.9 if smp else None, False)
    eng._begin_penalties([TRIPLE] if pen else None)


# (penalties, sampling, mask) -> launches of _pick, in order
PICK = {
    (False, False, "none"): ["argmax"],
    (False, False, "json"): ["json_mask", "argmax_masked"],
    (False, False, "schema"): ["schema_mask", "argmax_masked"],
    (False, True, "none"): ["sample"],
    (False, True, "json"): ["json_mask", "sample"],
    (False, True, "schema"): ["schema_mask", "sample"],
    (True, False, "none"): ["penalize", "argmax"],
    (True, False, "json"): ["penalize", "json_mask", "argmax_masked"],
    (True, False, "schema"): ["penalize", "schema_mask", "argmax_masked"],
    (True, True, "none"): ["penalize", "sample"],
    (True, True, "json"): ["penalize", "json_mask", "sample"],
    (True, True, "schema"): ["penalize", "schema_mask", "sample"],
}
# ... and of _gemv_pick: the fused lm_head + pick, or the plain GEMV and then _pick while sampling or penalties are on
GEMV_PICK = {
    (False, False, "none"): ["gemv_argmax"],
    (False, False, "json"): ["json_mask", "gemv_argmax_masked"],
    (False, False, "schema"): ["schema_mask", "gemv_argmax_masked"],
    (False, True, "none"): ["gemv", "sample"],
    (False, True, "json"): ["gemv", "json_mask", "sample"],
    (False, True, "schema"): ["gemv", "schema_mask", "sample"],
    (True, False, "none"): ["gemv", "penalize", "argmax"],
    (True, False, "json"): ["gemv", "penalize", "json_mask", "argmax_masked"],
    (True, False, "schema"): ["gemv", "penalize", "schema_mask", "argmax_masked"],
    (True, True, "none"): ["gemv", "penalize", "sample"],
    (True, True, "json"): ["gemv", "penalize", "json_mask", "sample"],
    (True, True, "schema"): ["gemv", "penalize", "schema_mask", "sample"],
}
COMBOS = list(itertools.product((False, True), (False, True), ("none", "json", "schema")))


def test_tables_cover_every_combination():
    assert sorted(PICK) == sorted(COMBOS) == sorted(GEMV_PICK) and len(COMBOS) == 12


@pytest.mark.parametrize("pen,smp,mask", COMBOS)
@pytest.mark.parametrize("B", [1, 2])
def test_pick_dispatch(calls, pen, smp, mask, B):
    eng = Stub(_Tokenizer())
    _switch(eng, pen, smp, mask)
    del calls[:]
    logits, tokens, cur, step = eng.logits_b[:B], eng.tokens_b[:B], eng.cur_b[:B], eng.step_b[:B]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == PICK[(pen, smp, mask)]
    by = {c[0]: c for c in calls}
    rows = eng._pen.out[:B] if pen else logits                  # the pick reads the penalised rows, the penalty the raw ones
    if pen:
        assert _same(by["penalize"][1][0], logits) and _same(by["penalize"][1][5], rows)
    allow = None if mask == "none" else eng._mask.allow[:B]
    assert (eng._mask is None) if mask == "none" else (eng._mask is (eng._schema if mask == "schema" else eng._json))
    if smp:
        a, kw = by["sample"][1], by["sample"][2]
        assert _same(a[0], rows) and _same(a[4], eng._smp.seeds[:B]) and a[6:] == (0.7, 0.9)
        assert (kw["allow"] is None) if allow is None else _same(kw["allow"], allow)
    elif mask == "none":
        a = by["argmax"][1]
        assert _same(a[0], rows) and a[6:] == (0.7, 11) and a[1] is eng.ws_val and a[2] is eng.ws_idx
    else:
        a = by["argmax_masked"][1]
        assert _same(a[0], rows) and _same(a[6], allow) and a[7:] == (0.7, 11)


@pytest.mark.parametrize("pen,smp,mask", COMBOS)
def test_gemv_pick_dispatch(calls, pen, smp, mask):
    eng = Stub(_Tokenizer())
    _switch(eng, pen, smp, mask)
    del calls[:]
    x, w, nw = torch.zeros(K, dtype=torch.bfloat16), torch.zeros((V, K), dtype=torch.bfloat16), torch.ones(K, dtype=torch.bfloat16)
    eng._gemv_pick(x, w, eng.logits_b[0], eng.ws_val, eng.ws_idx, eng.tokens_b[0], eng.cur_b[0:1], eng.step_b[0:1],
                   norm_w=nw, eps=1e-5, temperature=0.7, seed=11)
    assert _names(calls) == GEMV_PICK[(pen, smp, mask)]
    first = calls[0]
    if pen or smp:
        assert first[1][0] is x and first[1][1] is w and _same(first[1][2], eng.logits_b[0])
        assert first[2]["norm_w"] is nw and first[2]["eps"] == 1e-5 and len(first[2]) == 2
        last = calls[-1]
        if not smp:
            assert last[1][-2:] == (0.7, 11)         # temperature and seed reach the pick that follows the GEMV
    else:
        fused = calls[-1]
        assert fused[1][0] is x and fused[1][1] is w and _same(fused[1][2], eng.logits_b[0])
        assert fused[2]["norm_w"] is nw and {k: v for k, v in fused[2].items() if k != "norm_w"} == \
            {"eps": 1e-5, "temperature": 0.7, "seed": 11}
        if mask != "none":
            assert _same(fused[1][8], eng._mask.allow[0])


def test_schema_mask_wins_over_json_mask(calls):
    eng = Stub(_Tokenizer())
    _switch(eng, False, False, "schema")
    eng.json_on = True                               # both on cannot be requested; the schema's rows are the ones used
    del calls[:]
    eng._pick(eng.logits_b[:1], eng.ws_val, eng.ws_idx, eng.tokens_b[:1], eng.cur_b[:1], eng.step_b[:1], 0.0, 0)
    assert _names(calls) == ["schema_mask", "argmax_masked"]
    assert eng._schema.off is eng._json.off          # one token table for both masks


def test_prompt_pick_sequence(calls):
    eng = Stub(_Tokenizer())
    slot = 2
    ids = torch.arange(5, dtype=torch.int32)
    with eng._pick_request(3, True, None, None, False, None):
        del calls[:]
        eng._prompt_pick(slot, ids, eng.logits_b[slot], eng.tokens_b[slot], eng.cur_b[slot:slot + 1], eng.step_b[slot:slot + 1])
    assert _names(calls) == ["reset", "json_mask", "argmax_masked", "logprobs"]
    assert calls[0][1][0] is eng._json and calls[0][1][1] == slot and calls[1][1][2] == slot
    a = calls[2][1]
    assert _same(a[1], eng.ws_val[256 * slot:256 * (slot + 1)]) and _same(a[2], eng.ws_idx[256 * slot:256 * (slot + 1)])
    assert a[7:] == (0.7, 11 + 0x9E3779B9 * slot)
    lp = calls[3][1]
    assert _same(lp[0], eng.logits_b[slot:slot + 1]) and _same(lp[2], eng.step_b[slot:slot + 1]) and lp[3] == 3

    with eng._pick_request(None, False, None, 0.9, True, [TRIPLE, (1.0, 0.0, 1.0), (2.0, 0.0, 0.0)]):
        eng._slot_seed[1] = 77
        eng._slot_pen[1] = (1.0, 0.0, 1.0)
        del calls[:]
        for s in (1, 2):
            eng._prompt_pick(s, ids, eng.logits_b[s], eng.tokens_b[s], eng.cur_b[s:s + 1], eng.step_b[s:s + 1])
        assert _names(calls) == ["penalty_prompt", "penalize", "sample"] * 2
        assert int(eng._smp.seeds[1]) == 77                                          # the request's own seed
        assert int(eng._smp.seeds[2]) & 0xFFFFFFFF == (11 + 0x9E3779B9 * 2) & 0xFFFFFFFF   # the slot-derived one
        assert eng._pen.params[1].tolist() == [1.0, 0.0, 1.0] and eng._pen.params[2].tolist() == [1.0, 0.0, 0.0]
        assert _same(calls[0][1][2], ids)


# ----------------------------------------------------------------------------- the request scope
def _assert_off(eng):
    assert eng.lp_k is None
    assert eng.json_on is False and eng.schema_on is False and eng.smp_on is False and eng.pen_on is False
    assert eng.top_p is None and eng.seeded is False
    assert eng._slot_seed == {} and eng._slot_pen == {}
    assert eng._mask is None
    assert eng._pick_key() == (None, False, False, None, False, False)


def test_scope_switches_on_in_order_and_off_again(calls):
    eng = Stub(_Tokenizer())
    order = []
    for name in ("_begin_logprobs", "_begin_schema", "_begin_json", "_begin_sampling", "_begin_penalties"):
        def wrap(*a, _f=getattr(eng, name), _n=name):
            order.append(_n)
            return _f(*a)
        setattr(eng, name, wrap)
    with eng._pick_request(3, True, None, 0.9, False, [TRIPLE]):
        assert order == ["_begin_logprobs", "_begin_schema", "_begin_json", "_begin_sampling", "_begin_penalties"]
        assert eng.lp_k == 3 and eng.json_on and not eng.schema_on and eng.smp_on and eng.top_p == 0.9 and eng.pen_on
        assert eng._slot_pen == {0: TRIPLE}          # a single request runs in slot 0
        assert eng._mask is eng._json
    _assert_off(eng)
    dfa = _dfa()
    with eng._pick_request(None, False, dfa, 1.0, True, [TRIPLE, TRIPLE]):
        assert eng.lp_k is None and eng.schema_on and not eng.json_on and eng._mask is eng._schema
        assert eng.smp_on and eng.seeded and eng.top_p is None          # top_p = 1 is off; the seeds alone switch sampling on
        assert eng.pen_on and eng._slot_pen == {}    # a batch's triples are placed by its prompt passes
        assert [c[1][0] is dfa and c[1][1] == () for c in calls if c[0] == "load"] == [True]
    _assert_off(eng)
    with eng._pick_request(None, False, None, None, False, None):
        _assert_off(eng)
    _assert_off(eng)


ON = dict(logprobs=3, json_mode=False, json_schema=None, top_p=0.9, seeded=True, penalties=[TRIPLE])


@pytest.mark.parametrize("tokenizer,change,message", [
    (None, dict(json_mode=True), "tokenizer"),                                  # raised while switching on, after logprobs
    (None, dict(json_schema="dfa"), "tokenizer"),
    (_Tokenizer(), dict(json_mode=True, json_schema="dfa"), "two grammars"),
    (_Tokenizer(), dict(json_schema={"type": "object"}), "SchemaDFA"),
    (_Tokenizer(), dict(json_mode=1), "json_mode"),
    (_Tokenizer(), dict(logprobs=21), "logprobs"),
    (_Tokenizer(), dict(logprobs=True), "logprobs"),
    (_Tokenizer(), dict(top_p=1.5), "top_p"),
    (_Tokenizer(), dict(top_p="0.9"), "top_p"),
])
def test_scope_is_clean_after_a_failure_to_switch_on(calls, tokenizer, change, message):
    eng = Stub(tokenizer)
    args = dict(ON, **change)
    if args["json_schema"] == "dfa":
        args["json_schema"] = _dfa()
    entered = []
    with pytest.raises(ValueError, match=message):
        with eng._pick_request(**args):
            entered.append(1)
    assert not entered
    _assert_off(eng)
    assert _names(calls) == []                       # nothing was launched or uploaded


def test_scope_is_clean_after_the_body_raises(calls):
    eng = Stub(_Tokenizer())
    for args in (dict(ON, json_mode=True), dict(ON, json_schema=_dfa())):
        with pytest.raises(RuntimeError, match="boom"):
            with eng._pick_request(**args):
                assert eng.lp_k == 3 and eng.smp_on and eng.pen_on and eng._mask is not None
                eng._slot_seed[0] = 5
                raise RuntimeError("boom")
        _assert_off(eng)


def test_scope_is_clean_when_a_schema_does_not_fit_the_device_tables(monkeypatch):
    eng, dfa = Stub(_Tokenizer()), _dfa()
    monkeypatch.setattr(json_schema, "SCHEMA_MAX_STATES", 1)      # SchemaBuffers.load refuses before it touches the device
    with pytest.raises(ValueError, match="exceed the device tables"):
        with eng._pick_request(**dict(ON, json_schema=dfa)):
            pass
    _assert_off(eng)


# ----------------------------------------------------------------------------- after the run
def test_record_logprobs_and_mask_failed(calls):
    eng = Stub(_Tokenizer())
    eng.last_logprobs = "stale"
    eng._record_logprobs([(0, 1, 2)])
    assert eng.last_logprobs == "stale" and eng._mask_failed(range(SLOTS)) == []      # both off: nothing happens
    with eng._pick_request(2, True, None, None, False, None):
        assert eng.last_logprobs is None
        eng._lp.lp[1, 4:7, 0] = torch.tensor([-1.0, -2.0, -3.0])
        eng._record_logprobs([(1, 4, 3), None, (0, 0, 0)])
        recs = eng.last_logprobs
        assert recs[1] is None and len(recs) == 3
        assert recs[0].token_logprobs.tolist() == [-1.0, -2.0, -3.0] and recs[0].top_ids.shape == (3, 2)
        assert len(recs[2].token_logprobs) == 0
        from vision_inspection_system_amd.json_grammar import ERR, SLOT_INTS
        eng._json.state[2, ERR] = 1
        eng._json.state[0, SLOT_INTS + ERR] = 1
        assert eng._mask_failed(range(SLOTS)) == [0, 2] and eng._mask_failed([1]) == [] and eng._mask_failed([2]) == [2]


# ----------------------------------------------------------------------------- the decode-graph key
def test_pick_key_follows_the_six_switches_and_nothing_else(calls):
    eng = Stub(_Tokenizer())
    base = (None, False, False, None, False, False)
    assert eng._pick_key() == base
    seen = {base}
    for field, values in (("lp_k", (0, 5)), ("json_on", (True,)), ("schema_on", (True,)), ("top_p", (0.9, 0.5)),
                          ("seeded", (True,)), ("pen_on", (True,))):
        for v in values:
            setattr(eng, field, v)
            key = eng._pick_key()
            assert key not in seen, (field, v)
            seen.add(key)
        setattr(eng, field, base[("lp_k", "json_on", "schema_on", "top_p", "seeded", "pen_on").index(field)])
        assert eng._pick_key() == base
    # the same through the request scope; what is read from device memory at replay (seeds, penalty values), the sampling
    # parameters the engines key themselves and the results of the last request are not part of it
    with eng._pick_request(5, False, None, 0.9, True, [TRIPLE]):
        key = eng._pick_key()
        assert key == (5, False, False, 0.9, True, True)
        eng._slot_seed[0], eng._slot_pen[0] = 123, (2.0, 1.0, 1.0)
        eng.temperature, eng.seed, eng.last_logprobs = 1.5, 99, []
        assert eng._pick_key() == key
    with eng._pick_request(5, False, None, 0.9, True, [(2.0, 1.0, 1.0), TRIPLE]):
        assert eng._pick_key() == key
    with eng._pick_request(None, True, None, 1.0, False, None):
        assert eng._pick_key() == (None, True, False, None, False, False)
    assert eng._pick_key() == base
