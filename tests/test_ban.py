"""no_repeat_ngram_size / bad_words / min_tokens without a GPU: the validators, ban.ban_ref against a brute-force restatement
of the three rules (and against transformers' processors where that package is importable), where the ban launch sits
among the pick stage's launches (the recorder technique of tests/test_stream.py on the stub engine of test_pick_stage.py),
the decode-graph key, the request scope, the client plumbing and the agents' environment switches."""
import os
import random
import threading

import numpy as np
import pytest
import torch

from test_pick_stage import COMBOS, GEMV_PICK, PICK, TRIPLE, Stub, _names, _same, _switch
from vision_inspection_system_amd import ban, hip
from vision_inspection_system_amd import client as CL
from vision_inspection_system_amd.ban import (BanRequest, bad_word_ids, ban_kwargs, ban_ref, check_bad_words, check_ban,
                                              check_min_tokens, check_ngram)
from vision_inspection_system_amd.json_mode import JsonBuffers, SchemaBuffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The buffer classes size their workspaces through the library's host-only queries."""
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    return hip.load()


class _Tok:
    """Bytes are ids; "hello" is id 300 and " hello" id 301 (a word with another spelling behind a space)."""

    def encode(self, text):
        out, i = [], 0
        b = text.encode()
        while i < len(b):
            if b[i:i + 6] == b" hello":
                out.append(301)
                i += 6
            elif b[i:i + 5] == b"hello":
                out.append(300)
                i += 5
            else:
                out.append(b[i])
                i += 1
        return out

    def token_bytes(self, t):
        return bytes([t]) if t < 256 else {300: b"hello", 301: b" hello"}.get(t, b"")


# ----------------------------------------------------------------------------- validators
def test_check_ngram():
    assert check_ngram(None) == 0 and check_ngram(0) == 0 and check_ngram(1) == 1 and check_ngram(np.int64(64)) == 64
    for bad in (-1, 65, 2.0, True, "3", [3]):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            check_ngram(bad)


def test_check_min_tokens():
    assert check_min_tokens(None) == 0 and check_min_tokens(0, 5) == 0 and check_min_tokens(5, 5) == 5
    assert check_min_tokens(10 ** 6) == 10 ** 6              # no max_tokens known here
    for bad in (-1, 1.0, True, "3", [3]):
        with pytest.raises(ValueError, match="min_tokens"):
            check_min_tokens(bad, 100)
    with pytest.raises(ValueError, match="exceeds max_tokens"):
        check_min_tokens(6, 5)


def test_check_bad_words():
    assert check_bad_words(None) is None and check_bad_words([]) is None
    assert check_bad_words(["a", "bc"]) == ("a", "bc") and check_bad_words(("x",) * 16) == ("x",) * 16
    for bad in ("abc", b"abc", 3, ["a", ""], ["a", 3], [None], ["x"] * 17):
        with pytest.raises(ValueError, match="bad_words"):
            check_bad_words(bad)


def test_bad_word_ids_both_spellings_and_the_table_limits():
    tok = _Tok()
    assert bad_word_ids(["ab"], tok) == [(97, 98)]                       # " ab" is one id longer: not another spelling
    assert bad_word_ids(["hello"], tok) == [(300,), (301,)]              # both spellings
    assert bad_word_ids([" hello"], tok) == [(301,)]
    assert bad_word_ids(["hello", "hello", "a"], tok) == [(300,), (301,), (97,)]
    assert bad_word_ids(None, tok) == [] and bad_word_ids(["12345678"], tok) == [tuple(b"12345678")]
    with pytest.raises(ValueError, match="9 token ids"):
        bad_word_ids(["123456789"], tok)
    assert len(bad_word_ids([f"hello{i}" for i in range(8)], tok)) == 16
    with pytest.raises(ValueError, match="exceed the table"):            # twice the words must fit the table
        bad_word_ids([f"hello{i}" for i in range(9)], tok)


def test_check_ban_per_request_off_values_and_json():
    assert check_ban(None, None, None, 3) is None and check_ban(0, [], 0, 2) is None
    assert check_ban([None, 0], None, [0, None], 2) is None
    assert check_ban(3, ["x"], 2, 2, 10) == BanRequest([(3, 2), (3, 2)], ("x",))
    assert check_ban([2, None], None, [None, 4], 2) == BanRequest([(2, 0), (0, 4)], None)
    assert check_ban(None, ["x"], None, 1) == BanRequest([(0, 0)], ("x",))
    for bad in (dict(no_repeat_ngram_size=[1]), dict(no_repeat_ngram_size=65), dict(min_tokens=[1, 2, 3]), dict(min_tokens=-1),
                dict(min_tokens=11), dict(min_tokens=[0, 11]), dict(bad_words="x"), dict(bad_words=[["x"], ["y"]])):
        with pytest.raises(ValueError):
            check_ban(**dict(dict(no_repeat_ngram_size=None, bad_words=None, min_tokens=None), **bad), n=2, max_tokens=10)
    for on in (dict(no_repeat_ngram_size=2), dict(bad_words=["x"]), dict(min_tokens=1)):
        kw = dict(dict(no_repeat_ngram_size=None, bad_words=None, min_tokens=None), **on)
        with pytest.raises(ValueError, match="JSON"):
            check_ban(**kw, n=1, json_mode=True)
        with pytest.raises(ValueError, match="JSON"):
            check_ban(**kw, n=1, json_schema=object())
    assert check_ban(None, None, 0, 1, json_mode=True) is None           # off: JSON mode is none of its business
    assert ban_kwargs(None) == {}
    assert ban_kwargs(BanRequest([(3, 2), (1, 1)], ("x",))) == {"no_repeat_ngram_size": 3, "min_tokens": 2, "bad_words": ["x"]}


# ----------------------------------------------------------------------------- ban_ref
def _brute(prompt, gen, n, words, min_tokens, eos):
    """The three rules as the issue words them, with loops."""
    h = list(prompt) + list(gen)
    L = len(h)
    out = set()
    if n >= 1:
        for i in range(L):
            if i + n - 1 < L and h[i:i + n - 1] == h[L - n + 1:L]:
                out.add(h[i + n - 1])
    for w in words:
        m = len(w)
        if m == 1 or (L >= m - 1 and h[L - m + 1:L] == list(w[:m - 1])):
            out.add(w[m - 1])
    if len(gen) < min_tokens:
        out.update(eos)
    return out


def _histories(n):
    """(prompt, generated) pairs over a 7-id alphabet with L in {0, n-1, n, n+1, 40}, the boundary at several places."""
    rng = random.Random(100 + n)
    for L in sorted({0, n - 1, n, n + 1, 40}):
        for trial in range(12):
            h = [rng.randrange(7) for _ in range(L)]
            if L == 40 and trial % 2:      # every other long history ends on a copy of an earlier n - 1 ids
                i = rng.randrange(L - 2 * n)
                h[L - n + 1:] = h[i:i + n - 1]
            for cut in sorted({0, L // 2, L}):
                yield h[:cut], h[cut:]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ban_ref_against_brute_force(n):
    rng = random.Random(n)
    some = 0
    for prompt, gen in _histories(n):
        words = [tuple(rng.randrange(7) for _ in range(rng.choice((1, 2, 2, 3, 8)))) for _ in range(rng.randrange(4))]
        mt = rng.choice((0, len(gen), len(gen) + 1))
        want = _brute(prompt, gen, n, words, mt, (5, 6))
        assert ban_ref(prompt, gen, n, words, mt, (5, 6)) == want, (prompt, gen, words, mt)
        assert ban_ref(prompt, gen, 0, (), 0, (5, 6)) == set()
        assert ban_ref(prompt, gen, n) == _brute(prompt, gen, n, (), 0, ())
        some += bool(_brute(prompt, gen, n, (), 0, ()))
    assert some > 10                                          # the alphabet is small enough for matches to be frequent


def test_ban_ref_hand_written():
    assert ban_ref([1, 2, 3], [1, 2], 3) == {3} and ban_ref([1, 2, 3, 1], [2], 3) == {3}      # across the boundary
    assert ban_ref([1, 2], [], 3) == set() and ban_ref([], [], 1) == set()                     # L < n
    assert ban_ref([4, 4], [4], 1) == {4} and ban_ref([1, 2], [1], 2) == {2}
    assert ban_ref([], [7, 8], 0, [(9,), (8, 5), (7, 8, 6), (1, 2)]) == {9, 5, 6}
    assert ban_ref([7], [8], 0, [(7, 8, 6)]) == {6} and ban_ref([7], [], 0, [(7, 8, 6)]) == set()
    assert ban_ref([1], [2, 3], 0, (), 3, (50, 51)) == {50, 51} and ban_ref([1], [2, 3], 0, (), 2, (50, 51)) == set()
    assert ban_ref([500, 2], [500], 2, [(900,)], vocab=500) == {2}                             # ids outside the vocabulary


def test_ban_ref_against_transformers():
    tf = pytest.importorskip("transformers")
    V = 7
    for n in (1, 2, 3, 4):
        rng = random.Random(n)
        proc = tf.NoRepeatNGramLogitsProcessor(n)
        for prompt, gen in _histories(n):
            h = prompt + gen
            if not h:
                continue                                      # the processors index the last column
            ids = torch.tensor([h], dtype=torch.long)
            out = proc(ids, torch.zeros((1, V)))
            assert set(torch.nonzero(torch.isinf(out[0])).flatten().tolist()) == ban_ref(prompt, gen, n), (n, h)
            # transformers skips a word that is longer than the whole context (m > L), where the rule here - and its own
            # earlier NoBadWordsLogitsProcessor - asks for the m - 1 ids in front only: compared where m <= L
            words = [[rng.randrange(V) for _ in range(rng.choice((1, 2, 3)))] for _ in range(3)]
            words = [w for w in words if len(w) <= len(h)] or [[3]]
            out = tf.NoBadWordsLogitsProcessor(words, eos_token_id=None)(ids, torch.zeros((1, V)))
            assert set(torch.nonzero(torch.isinf(out[0])).flatten().tolist()) == ban_ref(prompt, gen, 0, words), (words, h)


# ----------------------------------------------------------------------------- launch order
@pytest.fixture
def calls(monkeypatch):
    """Every launch the pick stage can issue, the ban launch included, as (name, args, kwargs) in issue order."""
    log = []

    def rec(name):
        def f(*a, **kw):
            log.append((name, a, kw))
        return f

    for name in ("argmax", "argmax_masked", "gemv", "gemv_argmax", "gemv_argmax_masked", "sample", "penalize",
                 "penalty_prompt", "logprobs", "shape_logits", "stop_scan", "ban"):
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


BAN = BanRequest([(3, 2)], ("ab", "hello"))
SHAPING = [(40, 0.05, ((7, -100.0),))]


def _banned(names, pen):
    """The launches of a pick with the ban launch behind the penalties and ahead of everything else."""
    return names[:1] + ["ban"] + names[1:] if pen else ["ban"] + names


@pytest.mark.parametrize("pen,smp,mask", COMBOS)
@pytest.mark.parametrize("B", [1, 2])
def test_pick_dispatch_with_ban(calls, pen, smp, mask, B):
    eng = Stub(_Tok())
    _switch(eng, pen, smp, mask)
    logits, tokens, cur, step = eng.logits_b[:B], eng.tokens_b[:B], eng.cur_b[:B], eng.step_b[:B]
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == PICK[(pen, smp, mask)] and "ban" not in _names(calls)      # off: the lists test_pick_stage.py pins
    eng._begin_ban(BanRequest(BAN.rows * B, BAN.words))
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == _banned(PICK[(pen, smp, mask)], pen)
    a = dict((c[0], c) for c in calls)["ban"][1]
    bn = eng._ban
    assert _same(a[0], eng._pen.out[:B] if pen else logits) and _same(a[12], bn.out[:B])       # the penalised rows when on
    assert _same(a[1], bn.prompt[:B]) and _same(a[2], bn.plen[:B]) and _same(a[3], tokens) and _same(a[4], bn.gen0[:B])
    assert _same(a[5], step) and _same(a[6], bn.ngram[:B]) and _same(a[7], bn.min_tokens[:B]) and _same(a[8], bn.words)
    assert a[9] == (2, 1, 1) and _same(a[10], bn.eos) and a[11] == 1
    assert bn.words[:3].tolist() == [[97, 98, 0, 0, 0, 0, 0, 0], [300] + [0] * 7, [301] + [0] * 7]
    assert bn.eos[0] == eng.cfg.eos_ids[0]
    assert _same(calls[-1][1][0], bn.out[:B])                 # the pick reads the banned rows
    # ... with shaping on as well: penalize, ban, mask, shape, pick
    eng._begin_shaping(SHAPING * B)
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    want = _banned(PICK[(pen, smp, mask)], pen)
    assert _names(calls) == want[:-1] + ["shape_logits", want[-1]]
    assert _same(dict((c[0], c) for c in calls)["shape_logits"][1][0], bn.out[:B])
    eng._end_shaping()
    eng._end_ban()
    del calls[:]
    eng._pick(logits, eng.ws_val, eng.ws_idx, tokens, cur, step, 0.7, 11)
    assert _names(calls) == PICK[(pen, smp, mask)]


def test_the_full_order_is_penalize_ban_mask_shape_pick(calls):
    eng = Stub(_Tok())
    _switch(eng, True, False, "json")
    eng._begin_ban(BAN)
    eng._begin_shaping(SHAPING)
    del calls[:]
    eng._pick(eng.logits_b[:1], eng.ws_val, eng.ws_idx, eng.tokens_b[:1], eng.cur_b[:1], eng.step_b[:1], 0.0, 0)
    assert _names(calls) == ["penalize", "ban", "json_mask", "shape_logits", "argmax_masked"]


@pytest.mark.parametrize("pen,smp,mask", COMBOS)
def test_gemv_pick_leaves_the_fused_path_when_on(calls, pen, smp, mask):
    eng = Stub(_Tok())
    _switch(eng, pen, smp, mask)
    x, w = torch.zeros(64, dtype=torch.bfloat16), torch.zeros((eng.cfg.vocab, 64), dtype=torch.bfloat16)

    def run():
        del calls[:]
        eng._gemv_pick(x, w, eng.logits_b[0], eng.ws_val, eng.ws_idx, eng.tokens_b[0], eng.cur_b[0:1], eng.step_b[0:1],
                       norm_w=None, eps=1e-5, temperature=0.7, seed=11)
        return _names(calls)

    assert run() == GEMV_PICK[(pen, smp, mask)]
    eng._begin_ban(BAN)
    names = run()
    assert names == ["gemv"] + _banned(PICK[(pen, smp, mask)], pen)
    assert "gemv_argmax" not in names and "gemv_argmax_masked" not in names
    assert _same(calls[0][1][2], eng.logits_b[0]) and _same(calls[-1][1][0], eng._ban.out[0])
    eng._end_ban()
    assert run() == GEMV_PICK[(pen, smp, mask)]


def test_prompt_pick_places_the_slot_parameters(calls):
    eng = Stub(_Tok())
    ids = torch.arange(5, dtype=torch.int32) + 20
    three = BanRequest([(3, 2), (0, 7), (1, 0)], None)
    with eng._pick_request(None, False, None, None, False, None, ban=three):
        assert eng.ban_on and eng._slot_ban == {}             # a batch's parameters are placed by its prompt passes
        eng._slot_ban[1], eng._slot_ban[2] = three.rows[1], three.rows[2]
        eng._ban.prompt[1, :7] = 55                           # stale entries of the slot's previous request
        eng.step_b.copy_(torch.tensor([4, 4, 9], dtype=torch.int32))
        del calls[:]
        for s in (1, 2, 0):
            eng._prompt_pick(s, ids, eng.logits_b[s], eng.tokens_b[s], eng.cur_b[s:s + 1], eng.step_b[s:s + 1])
        assert _names(calls) == ["ban", "argmax"] * 3
        bn = eng._ban
        assert bn.ngram.tolist() == [0, 0, 1] and bn.min_tokens.tolist() == [0, 7, 0]           # slot 0 had no entry: neutral
        assert bn.plen.tolist() == [5, 5, 5] and bn.gen0.tolist() == [4, 4, 9]
        assert bn.prompt[1, :7].tolist() == [20, 21, 22, 23, 24, 55, 55]
        assert bn.word_len == () and calls[0][1][9] == ()
    with eng._pick_request(None, False, None, None, False, None, ban=BAN):
        assert eng._slot_ban == {0: (3, 2)}                   # a single request runs in slot 0
        eng._prompt_pick(0, ids, eng.logits_b[0], eng.tokens_b[0], eng.cur_b[0:1], eng.step_b[0:1])
        assert eng._ban.ngram[0] == 3 and eng._ban.min_tokens[0] == 2 and eng._ban.word_len == (2, 1, 1)


# ----------------------------------------------------------------------------- keys and the request scope
def test_keys(calls):
    eng = Stub(_Tok())
    base = (None, False, False, None, False, False)
    assert eng._pick_key() == base and eng._ban_key() == (False,)
    with eng._pick_request(None, False, None, None, False, None, ban=BAN):
        assert eng._pick_key() == base and eng._shape_key() == (False,)
        on = eng._ban_key()
        assert on == (True, (2, 1, 1))                        # the words' lengths are launch arguments
    with eng._pick_request(None, False, None, None, False, None, ban=BanRequest([(1, 9)], ("xy", "hello"))):
        assert eng._ban_key() == on                           # n, min_tokens and the ids are read from device memory
    with eng._pick_request(None, False, None, None, False, None, ban=BanRequest([(1, 9)], None)):
        assert eng._ban_key() == (True, ())
    assert eng._ban_key() == (False,)


def test_switches_end_off(calls):
    eng = Stub(_Tok())
    with pytest.raises(RuntimeError, match="boom"):
        with eng._pick_request(3, False, None, 0.9, True, [TRIPLE], ban=BAN):
            assert eng.ban_on and eng._slot_ban == {0: (3, 2)}
            raise RuntimeError("boom")
    assert eng.ban_on is False and eng._slot_ban == {} and eng._ban_key() == (False,)
    assert eng.lp_k is None and not eng.smp_on and not eng.pen_on
    entered = []
    with pytest.raises(ValueError, match="9 token ids"):      # raised while switching on
        with eng._pick_request(None, False, None, None, False, None, ban=BanRequest([(0, 0)], ("123456789",))):
            entered.append(1)
    with pytest.raises(ValueError, match="JSON"):             # together with a grammar: refused before anything is on
        with eng._pick_request(None, True, None, None, False, None, ban=BAN):
            entered.append(1)
    with pytest.raises(ValueError, match="top_p"):            # another switch refuses: the bans never come on
        with eng._pick_request(None, False, None, 1.5, False, None, ban=BAN):
            entered.append(1)
    assert not entered and eng.ban_on is False and eng._slot_ban == {} and not eng.json_on
    with pytest.raises(ValueError, match="tokenizer"):        # bad_words need the vocabulary
        with Stub(None)._pick_request(None, False, None, None, False, None, ban=BAN):
            entered.append(1)
    del calls[:]
    eng._pick(eng.logits_b[:1], eng.ws_val, eng.ws_idx, eng.tokens_b[:1], eng.cur_b[:1], eng.step_b[:1], 0.0, 0)
    assert _names(calls) == ["argmax"]


@pytest.mark.parametrize("engine_mod,cls", [("engine", "Qwen2VLEngine"), ("mllama_engine", "MllamaEngine")])
def test_engines_check_ban_arguments_first(engine_mod, cls):
    import importlib
    E = getattr(importlib.import_module(f"vision_inspection_system_amd.{engine_mod}"), cls)
    eng = E.__new__(E)           # no device state: the checks run before anything touches the GPU or the model
    eng.max_batch = 4
    reqs = [([1, 2], None), ([3, 4], None)]
    for bad in (dict(no_repeat_ngram_size=65), dict(no_repeat_ngram_size=[1]), dict(min_tokens=-1), dict(min_tokens=[1, 2, 3]),
                dict(min_tokens=9, max_new_tokens=8), dict(bad_words="x"), dict(bad_words=["x"] * 17),
                dict(min_tokens=1, json_mode=True), dict(bad_words=["x"], json_schema=object())):
        with pytest.raises(ValueError):
            eng.generate_batch(reqs, **bad)
    for bad in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(min_tokens=9, max_new_tokens=8),
                dict(bad_words=[""]), dict(no_repeat_ngram_size=2, json_mode=True)):
        with pytest.raises(ValueError):
            eng.generate([1, 2], **bad)


# ----------------------------------------------------------------------------- the clients
class _HostOnlyEngine:
    """Stands where the engine stands and records the keywords of every call."""
    host_only = True

    def __init__(self, max_batch):
        self.max_batch, self.device, self.lock = max_batch, "cpu", threading.Lock()
        self.calls, self.last_timing, self.last_logprobs, self.last_finish = [], {}, None, None

    def generate_batch(self, requests, **kw):
        ids = [r()[0] for r in requests]
        self.calls.append(kw)
        self.last_finish = [("length", None) for _ in ids]
        return [[65, 66] for _ in ids]


def test_client_hands_the_keywords_to_the_engine_and_checks_them_first():
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    cfg = Qwen2VLConfig.tiny()
    tok = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    eng = _HostOnlyEngine(4)
    CL.register_model("host-only:ban", "cpu", CL.LoadedModel(eng, tok, cfg, "host-only:ban"))
    try:
        c = CL.LocalVLMClient(device="cpu")
        msgs = [{"role": "user", "content": "x"}]
        c.chat.completions.create(model="host-only:ban", messages=msgs, max_tokens=8, no_repeat_ngram_size=3,
                                  bad_words=["```", "As an AI"], min_tokens=5)
        kw = eng.calls[-1]
        assert kw["no_repeat_ngram_size"] == 3 and kw["bad_words"] == ["```", "As an AI"] and kw["min_tokens"] == 5
        c.complete_many("host-only:ban", [msgs, msgs], max_tokens=8, min_tokens=2)
        assert eng.calls[-1]["min_tokens"] == 2 and "bad_words" not in eng.calls[-1]
        c.chat.completions.create(model="host-only:ban", messages=msgs, no_repeat_ngram_size=0, bad_words=[], min_tokens=0)
        assert not {"no_repeat_ngram_size", "bad_words", "min_tokens"} & set(eng.calls[-1])     # off: the call of before
        n = len(eng.calls)
        for bad in (dict(no_repeat_ngram_size=65), dict(min_tokens=9, max_tokens=8), dict(min_tokens=513), dict(bad_words="x"),
                    dict(bad_words=["x"] * 17), dict(min_tokens=1, response_format={"type": "json_object"}),
                    dict(no_repeat_ngram_size=2, stream=True, response_format={"type": "json_object"})):
            with pytest.raises(ValueError):
                c.chat.completions.create(model="host-only:ban", messages=msgs, **bad)
        assert len(eng.calls) == n                            # refused before the engine saw anything
    finally:
        CL.unregister_model("host-only:ban", "cpu")


def test_mock_client_validates_the_same_way():
    c = CL.CannedResponseClient("OK")
    c.chat.completions.create(model="m", messages=[], no_repeat_ngram_size=3, bad_words=["x"], min_tokens=5)
    c.chat.completions.create(model="m", messages=[])
    assert c.calls[0]["no_repeat_ngram_size"] == 3 and c.calls[0]["bad_words"] == ["x"] and c.calls[0]["min_tokens"] == 5
    assert not {"no_repeat_ngram_size", "bad_words", "min_tokens"} & set(c.calls[1])           # only the keywords given
    for bad in (dict(no_repeat_ngram_size=65), dict(min_tokens=9, max_tokens=8), dict(bad_words=["x", ""]),
                dict(min_tokens=1, response_format={"type": "json_object"})):
        with pytest.raises(ValueError):
            c.chat.completions.create(model="m", messages=[], **bad)
    assert len(c.calls) == 2


# ----------------------------------------------------------------------------- the agents' switches
def test_ban_kwargs_env(monkeypatch):
    from vision_inspection_system_amd.agents import ban_kwargs as env_kwargs
    for name in ("VIS_NO_REPEAT_NGRAM", "VIS_BAD_WORDS", "VIS_MIN_TOKENS"):
        monkeypatch.delenv(name, raising=False)
    assert env_kwargs() == {}
    monkeypatch.setenv("VIS_NO_REPEAT_NGRAM", " 3 ")
    assert env_kwargs() == {"no_repeat_ngram_size": 3}
    monkeypatch.setenv("VIS_BAD_WORDS", '["```", "As an AI"]')
    monkeypatch.setenv("VIS_MIN_TOKENS", "5")
    assert env_kwargs() == {"no_repeat_ngram_size": 3, "bad_words": ["```", "As an AI"], "min_tokens": 5}
    for name, bad in (("VIS_NO_REPEAT_NGRAM", "65"), ("VIS_NO_REPEAT_NGRAM", "2.5"), ("VIS_NO_REPEAT_NGRAM", "many"),
                      ("VIS_BAD_WORDS", '"x"'), ("VIS_BAD_WORDS", "[x]"), ("VIS_BAD_WORDS", '[""]'), ("VIS_MIN_TOKENS", "-1"),
                      ("VIS_MIN_TOKENS", "few")):
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError, match=name):
            env_kwargs()
        monkeypatch.setenv(name, {"VIS_NO_REPEAT_NGRAM": "3", "VIS_BAD_WORDS": "[]", "VIS_MIN_TOKENS": "0"}[name])
    assert env_kwargs() == {"no_repeat_ngram_size": 3, "bad_words": [], "min_tokens": 0}
