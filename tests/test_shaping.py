"""top_k / min_p / logit_bias without a GPU: the validators, shaping.reference_shape on hand-written rows, where the shaping
launch sits among the pick stage's launches under every combination of the other switches (the recorder technique and the
tables of test_pick_stage.py), the decode-graph keys, the request scope, and the agents' environment switches."""
import math
import os

import numpy as np
import pytest
import torch

from test_pick_stage import COMBOS, GEMV_PICK, PICK, TRIPLE, Stub, _names, _same, _switch, _Tokenizer
from vision_inspection_system_amd import hip, shaping
from vision_inspection_system_amd.json_mode import JsonBuffers, SchemaBuffers
from vision_inspection_system_amd.shaping import (MAX_BIAS, check_logit_bias, check_min_p, check_shaping, check_top_k,
                                                  min_p_delta, reference_shape)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -math.inf


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The buffer classes size their workspaces through the library's host-only queries."""
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    return hip.load()


# ----------------------------------------------------------------------------- validators
def test_check_top_k():
    assert check_top_k(None) is None and check_top_k(1) == 1 and check_top_k(np.int64(40)) == 40
    assert check_top_k(10 ** 9) == 10 ** 9                   # beyond any vocabulary: cuts nothing
    for bad in (0, -1, 1.0, 2.5, True, "3", [3]):
        with pytest.raises(ValueError, match="top_k"):
            check_top_k(bad)


def test_check_min_p():
    assert check_min_p(None) is None and check_min_p(0) == 0.0 and check_min_p(1) == 1.0 and check_min_p(np.float32(0.5)) == 0.5
    for bad in (-0.01, 1.01, float("nan"), float("inf"), True, "0.1", [0.1]):
        with pytest.raises(ValueError, match="min_p"):
            check_min_p(bad)


def test_check_logit_bias():
    assert check_logit_bias(None, 100) is None and check_logit_bias({}, 100) is None
    assert check_logit_bias({"7": -100, 99: 100, 0: 0.5, np.int32(3): np.float32(1.5)}, 100) == \
        ((7, -100.0), (99, 100.0), (0, 0.5), (3, 1.5))
    assert len(check_logit_bias({i: 1 for i in range(MAX_BIAS)}, 1000)) == MAX_BIAS
    assert check_logit_bias({5000: 1}) == ((5000, 1.0),)     # without a vocabulary size only the lower bound is asked ...
    with pytest.raises(ValueError, match="outside the vocabulary"):
        shaping.check_vocab([(None, None, ((5000, 1.0),))], 320)                # ... and the upper one when the request starts
    shaping.check_vocab([(None, None, ((319, 1.0),)), (3, None, None)], 320)
    shaping.check_vocab(None, 320)
    for bad, msg in (({i: 1 for i in range(MAX_BIAS + 1)}, "at most"), ({100: 1}, "outside"), ({-1: 1}, "outside"),
                     ({"-1": 1}, "not an integer"), ({"1.5": 1}, "not an integer"), ({1.0: 1}, "not an integer"),
                     ({"": 1}, "not an integer"), ({True: 1}, "not an integer"), ({"7": 1, 7: 2}, "twice"),
                     ({"07": 1, "7": 2}, "twice"), ({1: 100.5}, "finite"), ({1: -101}, "finite"), ({1: float("nan")}, "finite"),
                     ({1: float("inf")}, "finite"), ({1: "3"}, "finite"), ({1: None}, "finite"), ({1: True}, "finite"),
                     ([(1, 2)], "dict"), ("{}", "dict")):
        with pytest.raises(ValueError, match=msg):
            check_logit_bias(bad, 100)


def test_check_shaping_per_request_and_off_values():
    assert check_shaping(None, None, None, 3) is None
    assert check_shaping(None, 0, {}, 2) is None and check_shaping([None, None], [0.0, None], [None, {}], 2) is None
    assert check_shaping(40, 0.05, {"3": 1}, 2) == [(40, 0.05, ((3, 1.0),))] * 2
    assert check_shaping([1, None], None, [None, {5: -100}], 2) == [(1, None, None), (None, None, ((5, -100.0),))]
    for bad in (dict(top_k=[1]), dict(min_p=[0.1, 0.2, 0.3]), dict(logit_bias=[{}]), dict(top_k=[1, 0]), dict(logit_bias="x")):
        with pytest.raises(ValueError):
            check_shaping(**dict(dict(top_k=None, min_p=None, logit_bias=None), **bad), n=2)
    assert shaping.shaping_kwargs(None) == {}
    assert shaping.shaping_kwargs([(3, None, ((5, -100.0),))]) == {"top_k": 3, "min_p": None, "logit_bias": {5: -100.0}}


def test_min_p_delta():
    assert min_p_delta(None, 1.0) == NINF and min_p_delta(0.0, 1.0) == NINF and min_p_delta(0.5, 0.0) == NINF
    assert min_p_delta(1.0, 0.7) == 0.0
    assert min_p_delta(0.05, 2.0) == float(np.float32(math.log(0.05) / (1.0 / 2.0)))
    assert min_p_delta(0.05, 0.5) == float(np.float32(math.log(0.05) / 2.0))


# ----------------------------------------------------------------------------- the reference on hand-written rows
def _f32(*v):
    return np.array(v, dtype=np.float32)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32).tolist()


def test_reference_tie_run_straddles_the_kth_place():
    x = _f32(1, 3, 2, 3, 3, 0, 5)
    r = reference_shape(x, k=2)                              # the 2nd largest is 3 and all three of them stay
    assert r.out.tolist() == [NINF, 3, NINF, 3, 3, NINF, 5] and r.nkept == 4
    assert reference_shape(x, k=4).nkept == 4 and reference_shape(x, k=5).out.tolist() == [NINF, 3, 2, 3, 3, NINF, 5]
    assert reference_shape(x, k=1).out.tolist() == [NINF] * 6 + [5]


def test_reference_zeros_compare_equal_and_keep_their_bits():
    x = _f32(-0.0, 0.0, -1, 0.0, -0.0, -2)
    r = reference_shape(x, k=1)                              # four zeros tie for the first place
    assert r.nkept == 4 and _bits(r.out) == _bits([-0.0, 0.0, NINF, 0.0, -0.0, NINF])
    r = reference_shape(x, delta=min_p_delta(1.0, 1.0))
    assert r.nkept == 4 and _bits(r.out) == _bits([-0.0, 0.0, NINF, 0.0, -0.0, NINF])


def test_reference_min_p():
    x = _f32(0, -1, -2.9, -3.1, 0, -10)
    assert reference_shape(x, delta=min_p_delta(1.0, 1.0)).out.tolist() == [0, NINF, NINF, NINF, 0, NINF]    # only the maxima
    d = min_p_delta(0.05, 1.0)                               # ln 0.05 = -2.9957
    assert reference_shape(x, delta=d).out.tolist() == _f32(0, -1, -2.9, NINF, 0, NINF).tolist()
    assert reference_shape(x, delta=min_p_delta(0.05, 2.0)).out.tolist() == _f32(0, -1, -2.9, -3.1, 0, NINF).tolist()   # -5.99 at T = 2
    assert reference_shape(x, delta=NINF).nkept == 6 and reference_shape(x, delta=min_p_delta(0.05, 0.0)).nkept == 6
    # f32 subtraction, f32 compare: an element exactly at the threshold stays
    t = np.float32(d)
    assert reference_shape(_f32(0, t, np.nextafter(t, np.float32(-1e9))), delta=d).out.tolist()[:2] == [0, float(t)]
    assert reference_shape(_f32(0, t, np.nextafter(t, np.float32(-1e9))), delta=d).nkept == 2


def test_reference_k_at_least_the_candidates_filters_nothing():
    x = _f32(4, 1, 3, 2)
    for k in (0, 4, 5, 10 ** 6):
        assert reference_shape(x, k=k).out.tolist() == x.tolist()
    allow = np.array([True, False, True, False])
    for k in (2, 3, 40):                                     # an allow row with fewer than k ids: every allowed id stays
        assert reference_shape(x, k=k, allow=allow).out.tolist() == [4, NINF, 3, NINF]
    assert reference_shape(x, k=1, allow=allow).out.tolist() == [4, NINF, NINF, NINF]
    r = reference_shape(x, k=1, allow=np.zeros(4, dtype=bool))
    assert r.nkept == 0 and r.out.tolist() == [NINF] * 4


def test_reference_bias_moves_the_maximum():
    x = _f32(4, 1, 3, 2)
    r = reference_shape(x, k=1, bias=[(1, 5.0)])
    assert r.out.tolist() == [NINF, 6, NINF, NINF]
    r = reference_shape(x, delta=min_p_delta(0.5, 1.0), bias=[(0, -100.0), (3, 0.75)])     # the maximum is now x[2] = 3
    assert r.out.tolist() == [NINF, NINF, 3, 2.75]
    assert reference_shape(x, bias=[(1, 5.0), (1, 7.0), (9, 1.0), (-1, 1.0)]).out.tolist() == [4, 6, 3, 2]    # first entry; ids outside
    r = reference_shape(x, k=1, bias=[(1, 100.0)], allow=np.array([True, False, True, True]))                 # a bias outside A
    assert r.out.tolist() == [4, NINF, NINF, NINF]
    one = np.float32(0.1) + np.float32(0.2)                  # one f32 add
    assert _bits(reference_shape(_f32(0.1), bias=[(0, 0.2)]).out) == _bits([one])


# ----------------------------------------------------------------------------- launch order
@pytest.fixture
def calls(monkeypatch):
    """Every launch the pick stage can issue, the shaping launch included, as (name, args, kwargs) in issue order."""
    log = []

    def rec(name):
        def f(*a, **kw):
            log.append((name, a, kw))
        return f

    for name in ("argmax", "argmax_masked", "gemv", "gemv_argmax", "gemv_argmax_masked", "sample", "penalize",
                 "penalty_prompt", "logprobs", "shape_logits", "stop_scan"):
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


SHAPING = [(40, 0.05, ((7, -100.0), (3, 2.5)))]


def _shaped(names):
    """The launches of a pick with the shaping launch in front of the pick itself."""
    return names[:-1] + ["shape_logits", names[-1]]


@pytest.mark.parametrize("pen,smp,mask", COMBOS)
@pytest.mark.parametrize("B", [1, 2])
def test_pick_dispatch_with_shaping(calls, pen, smp, mask, B):
    eng = Stub(_Tokenizer())
    _switch(eng, pen, smp, mask)
    logits, tokens, cur, step = eng.logits_b[:B], eng.tokens_b[:B], eng.cur_b[:B], eng.step_b[:B]
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == PICK[(pen, smp, mask)]           # shaping off: the lists test_pick_stage.py pins
    eng._begin_shaping(SHAPING * B)
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == _shaped(PICK[(pen, smp, mask)])
    by = {c[0]: c for c in calls}
    a, kw = by["shape_logits"][1], by["shape_logits"][2]
    src = eng._pen.out[:B] if pen else logits                # the penalised rows when penalties are on, else the raw ones
    shp = eng._shp
    assert _same(a[0], src) and _same(a[6], shp.out[:B]) and _same(a[7], shp.nkept[:B]) and _same(a[8], shp.ws[:B])
    assert _same(a[1], shp.k[:B]) and _same(a[2], shp.delta[:B]) and _same(a[3], shp.nbias[:B])
    assert _same(a[4], shp.bias_ids[:B]) and _same(a[5], shp.bias_vals[:B])
    allow = None if mask == "none" else eng._mask.allow[:B]
    assert (kw["allow"] is None) if allow is None else _same(kw["allow"], allow)      # the mask's rows reach the shaping launch
    pick = calls[-1]
    assert _same(pick[1][0], shp.out[:B])                    # ... and the pick reads the shaped rows
    if smp:
        assert (pick[2]["allow"] is None) if allow is None else _same(pick[2]["allow"], allow)
    elif mask != "none":
        assert _same(pick[1][6], allow)
    eng._end_shaping()
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == PICK[(pen, smp, mask)]


@pytest.mark.parametrize("pen,smp,mask", COMBOS)
def test_gemv_pick_dispatch_with_shaping(calls, pen, smp, mask):
    eng = Stub(_Tokenizer())
    _switch(eng, pen, smp, mask)
    x, w = torch.zeros(64, dtype=torch.bfloat16), torch.zeros((eng.cfg.vocab, 64), dtype=torch.bfloat16)

    def run():
        del calls[:]
        eng._gemv_pick(x, w, eng.logits_b[0], eng.ws_val, eng.ws_idx, eng.tokens_b[0], eng.cur_b[0:1], eng.step_b[0:1],
                       norm_w=None, eps=1e-5, temperature=0.7, seed=11)
        return _names(calls)

    assert run() == GEMV_PICK[(pen, smp, mask)]
    eng._begin_shaping(SHAPING)
    assert run() == ["gemv"] + _shaped(PICK[(pen, smp, mask)])      # the plain lm_head GEMV, then _pick
    assert _same(calls[0][1][2], eng.logits_b[0]) and _same(calls[-1][1][0], eng._shp.out[0])
    if not smp:
        assert calls[-1][1][-2:] == (0.7, 11)
    eng._end_shaping()
    assert run() == GEMV_PICK[(pen, smp, mask)]


def test_prompt_pick_places_the_slot_parameters(calls):
    eng = Stub(_Tokenizer())
    ids = torch.arange(5, dtype=torch.int32)
    three = [(40, 0.05, ((7, -100.0), (3, 2.5))), (None, None, ((319, 100.0),)), (2, 1.0, None)]
    with eng._pick_request(None, False, None, None, False, None, shaping=three):
        assert eng.shape_on and eng._slot_shape == {}        # a batch's parameters are placed by its prompt passes
        eng._slot_shape[1], eng._slot_shape[2] = three[1], three[2]
        eng._shp.bias_ids[1, :2] = 55                        # stale entries of the slot's previous request
        del calls[:]
        for s in (1, 2, 0):
            eng._prompt_pick(s, ids, eng.logits_b[s], eng.tokens_b[s], eng.cur_b[s:s + 1], eng.step_b[s:s + 1])
        assert _names(calls) == ["shape_logits", "argmax"] * 3
        shp = eng._shp
        assert shp.k.tolist() == [0, 0, 2] and shp.nbias.tolist() == [0, 1, 0]
        assert shp.delta.tolist() == [NINF, NINF, min_p_delta(1.0, 0.7)]                 # slot 0 had no entry: neutral
        assert shp.bias_ids[1, 0] == 319 and shp.bias_vals[1, 0] == 100.0
        assert _same(calls[0][1][6], shp.out[1]) and _same(calls[2][1][6], shp.out[2])
    with eng._pick_request(None, False, None, None, False, None, shaping=three[:1]):
        assert eng._slot_shape == {0: three[0]}              # a single request runs in slot 0
        eng._prompt_pick(0, ids, eng.logits_b[0], eng.tokens_b[0], eng.cur_b[0:1], eng.step_b[0:1])
        shp = eng._shp
        assert shp.k[0] == 40 and shp.nbias[0] == 2 and shp.bias_ids[0, :2].tolist() == [7, 3]
        assert shp.bias_vals[0, :2].tolist() == [-100.0, 2.5] and float(shp.delta[0]) == min_p_delta(0.05, 0.7)
        eng.temperature = 0.0                                # a greedy request: logit_bias only
        eng._shape_slot(0)
        assert float(shp.delta[0]) == NINF and shp.k[0] == 40
        eng.temperature = 0.7


# ----------------------------------------------------------------------------- keys and the request scope
def test_keys(calls):
    eng = Stub(_Tokenizer())
    base = (None, False, False, None, False, False)
    assert eng._pick_key() == base and eng._shape_key() == (False,)
    with eng._pick_request(None, False, None, None, False, None, shaping=SHAPING):
        assert eng._pick_key() == base and len(eng._pick_key()) == 6          # still the six-tuple
        on = eng._shape_key()
        assert on == (True,)
    with eng._pick_request(5, False, None, 0.9, True, [TRIPLE], shaping=[(1, None, None), (None, 1.0, ((0, 1.0),))]):
        assert eng._pick_key() == (5, False, False, 0.9, True, True)
        assert eng._shape_key() == on                        # the values are read from device memory at replay
    assert eng._shape_key() == (False,) and eng._pick_key() == base
    with eng._pick_request(None, False, None, None, False, None):
        assert eng._shape_key() == (False,) and eng._shp is not None


def test_scope_is_clean_after_a_request_that_raises(calls):
    eng = Stub(_Tokenizer())
    with pytest.raises(RuntimeError, match="boom"):
        with eng._pick_request(3, True, None, 0.9, True, [TRIPLE], shaping=SHAPING):
            assert eng.shape_on and eng._slot_shape == {0: SHAPING[0]}
            raise RuntimeError("boom")
    assert eng.shape_on is False and eng._slot_shape == {} and eng._shape_key() == (False,)
    assert eng.lp_k is None and not eng.json_on and not eng.smp_on and not eng.pen_on
    entered = []
    with pytest.raises(ValueError, match="outside the vocabulary"):      # raised while switching on
        with eng._pick_request(None, False, None, None, False, None, shaping=[(None, None, ((eng.cfg.vocab, 1.0),))]):
            entered.append(1)
    with pytest.raises(ValueError, match="top_p"):                       # another switch refuses: shaping never comes on
        with eng._pick_request(None, False, None, 1.5, False, None, shaping=SHAPING):
            entered.append(1)
    assert not entered and eng.shape_on is False and eng._slot_shape == {}
    del calls[:]
    eng._pick(eng.logits_b[:1], eng.ws_val, eng.ws_idx, eng.tokens_b[:1], eng.cur_b[:1], eng.step_b[:1], 0.0, 0)
    assert _names(calls) == ["argmax"]


@pytest.mark.parametrize("engine_mod,cls", [("engine", "Qwen2VLEngine"), ("mllama_engine", "MllamaEngine")])
def test_engines_check_shaping_arguments_first(engine_mod, cls):
    import importlib
    E = getattr(importlib.import_module(f"vision_inspection_system_amd.{engine_mod}"), cls)
    eng = E.__new__(E)           # no device state: the checks run before anything touches the GPU or the model
    eng.max_batch = 4
    reqs = [([1, 2], None), ([3, 4], None)]
    for bad in (dict(top_k=0), dict(top_k=[1]), dict(min_p=1.5), dict(min_p=[0.1, "x"]), dict(logit_bias={1: 101}),
                dict(logit_bias=[{}, {}, {}]), dict(logit_bias={"a": 1})):
        with pytest.raises(ValueError):
            eng.generate_batch(reqs, **bad)
    for bad in (dict(top_k=0), dict(top_k=2.0), dict(min_p=1.5), dict(min_p="x"), dict(logit_bias={1: 101}),
                dict(logit_bias=[{}, {}]), dict(logit_bias={"a": 1})):
        with pytest.raises(ValueError):
            eng.generate([1, 2], **bad)


def test_canned_client_records_shaping_arguments():
    from vision_inspection_system_amd.client import CannedResponseClient
    c = CannedResponseClient("OK")
    c.chat.completions.create(model="m", messages=[], top_k=40, min_p=0.05, logit_bias={"5": -100})
    c.chat.completions.create(model="m", messages=[])
    assert c.calls[0]["top_k"] == 40 and c.calls[0]["min_p"] == 0.05 and c.calls[0]["logit_bias"] == {"5": -100}
    assert not {"top_k", "min_p", "logit_bias"} & set(c.calls[1])       # only the keywords that were given


# ----------------------------------------------------------------------------- the agents' switches
def test_shaping_kwargs_env(monkeypatch):
    from vision_inspection_system_amd.agents import shaping_kwargs
    for name in ("VIS_TOP_K", "VIS_MIN_P", "VIS_LOGIT_BIAS"):
        monkeypatch.delenv(name, raising=False)
    assert shaping_kwargs() == {}
    monkeypatch.setenv("VIS_TOP_K", " 40 ")
    assert shaping_kwargs() == {"top_k": 40}
    monkeypatch.setenv("VIS_MIN_P", "0.05")
    monkeypatch.setenv("VIS_LOGIT_BIAS", '{"74": -100, "5": 2.5}')
    assert shaping_kwargs() == {"top_k": 40, "min_p": 0.05, "logit_bias": {"74": -100, "5": 2.5}}
    for name, bad in (("VIS_TOP_K", "0"), ("VIS_TOP_K", "4.5"), ("VIS_TOP_K", "many"), ("VIS_MIN_P", "2"), ("VIS_MIN_P", "p"),
                      ("VIS_LOGIT_BIAS", "[1]"), ("VIS_LOGIT_BIAS", "{5: 1}"), ("VIS_LOGIT_BIAS", '{"5": 500}')):
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError, match=name if name != "VIS_LOGIT_BIAS" or bad != '{"5": 500}' else "finite"):
            shaping_kwargs()
        monkeypatch.setenv(name, {"VIS_TOP_K": "40", "VIS_MIN_P": "0.05", "VIS_LOGIT_BIAS": "{}"}[name])
    assert shaping_kwargs() == {"top_k": 40, "min_p": 0.05, "logit_bias": {}}
