"""Stop strings without a GPU: the argument check, the automaton and its Python walk (stop.scan, the reference of the GPU
tests) against plain bytes.find, the mock client's record, and where PickStage issues the stop_scan launch."""
import os
import random

import pytest
import torch

from vision_inspection_system_amd import hip, stop
from vision_inspection_system_amd.client import CannedResponseClient
from vision_inspection_system_amd.pick import PickStage
from vision_inspection_system_amd.stop import EOS, OPEN, STOP, check_stop, compile_stop, find_oracle, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- check_stop
def test_check_stop_accepts():
    assert check_stop(None) is None
    assert check_stop("```") == (b"```",)
    assert check_stop(["a", b"b", "€"]) == (b"a", b"b", b"\xe2\x82\xac")
    assert check_stop(("x", "y", "z", "w")) == (b"x", b"y", b"z", b"w")
    assert check_stop(["ab", "ab", b"ab", "c"]) == (b"ab", b"c")            # duplicates collapse, the order stays
    assert check_stop(["a" * 64]) == (b"a" * 64,)
    assert check_stop(["€" * 21]) == (("€" * 21).encode(),)        # 63 bytes


@pytest.mark.parametrize("bad", [[], ["a", "b", "c", "d", "e"], [""], ["ok", ""], ["a" * 65], ["€" * 22], [1], ["a", None],
                                 3, b"raw", {"a"}, [["a"]]])
def test_check_stop_refuses(bad):
    with pytest.raises(ValueError) as e:
        check_stop(bad)
    text = str(e.value).lower()
    assert not any(w in text for w in ("429", "rate", "413", "payload"))    # what the agents' retry logic keys on


# ----------------------------------------------------------------------------- scan against bytes.find
def _same(a: dict, b: dict):
    assert {k: a[k] for k in ("reason", "n_tokens", "cut", "which")} == b, (a, b)


def test_scan_against_find_random_sweep():
    rng = random.Random(20240607)
    seen = {OPEN: 0, EOS: 0, STOP: 0}
    for _ in range(4000):
        stops = [bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 4))]
        stream = bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 40)))
        toks, i = [], 0
        while i < len(stream):
            n = rng.randint(0, 5)
            toks.append(stream[i:i + n])
            i += n
        eos = [rng.random() < 0.04 for _ in toks]
        got, want = scan(stops, toks, eos), find_oracle(stops, toks, eos)
        _same(got, want)
        seen[got["reason"]] += 1
        if got["reason"] == STOP:           # the text in front of the cut holds no stop string; the match sits at the cut
            s = check_stop(stops)[got["which"]]
            kept = b"".join(toks[:got["n_tokens"]])
            assert kept[got["cut"]:got["cut"] + len(s)] == s
            assert all(t not in kept[:got["cut"] + len(s) - 1] for t in check_stop(stops))
    assert all(v > 100 for v in seen.values()), seen


NAMED = [
    # name, stops, tokens, eos flags, (reason, n_tokens, cut, which)
    ("failure link: aab in aaab", ["aab"], [b"a", b"a", b"a", b"b", b"c"], None, (STOP, 4, 1, 0)),
    ("suffix of another: the shorter ends first", ["xabc", "bc"], [b"ab", b"c", b"d"], None, (STOP, 2, 1, 1)),
    ("suffix of another: same end, the longer wins", ["xabc", "bc"], [b"xa", b"bc"], None, (STOP, 2, 0, 0)),
    ("tie at one end offset: the longest wins", ["c", "bc", "abc"], [b"zab", b"cd"], None, (STOP, 2, 1, 2)),
    ("inside one token, trailing bytes", ["```"], [b"{}", b"x```yz", b"more"], None, (STOP, 2, 3, 0)),
    ("spanning three tokens", ["hello"], [b"ohe", b"ll", b"o!"], None, (STOP, 3, 1, 0)),
    ("3-byte UTF-8 over three one-byte tokens", ["€"], [b"a", b"\xe2", b"\x82", b"\xac", b"b"], None, (STOP, 4, 1, 0)),
    ("EOS one token before a would-be match", ["ab"], [b"xa", b"", b"b"], [False, True, False], (EOS, 1, 2, 0)),
    ("match in the first token", ["ab"], [b"abc", b"d"], None, (STOP, 1, 0, 0)),
    ("empty tokens contribute nothing", ["ab"], [b"a", b"", b"", b"b"], None, (STOP, 4, 0, 0)),
    ("nothing matches", ["zz"], [b"ab", b"z"], None, (OPEN, 2, 0, 0)),
]


@pytest.mark.parametrize("name,stops,toks,eos,want", NAMED, ids=[c[0] for c in NAMED])
def test_scan_named_cases(name, stops, toks, eos, want):
    want = dict(zip(("reason", "n_tokens", "cut", "which"), want))
    _same(scan(stops, toks, eos), want)
    _same(dict(find_oracle(stops, toks, eos)), want)


def test_dfa_bounds_for_the_maximal_input():
    stops = [bytes(64 * i + j for j in range(64)) for i in range(4)]        # 4 x 64 bytes, every byte value occurs
    d = compile_stop(stops)
    assert d.trans.dtype.name == "uint16" and d.trans.shape == (257, 256) == (stop.MAX_STATES, stop.MAX_CLASSES)
    assert int(d.trans.max()) < 257 and d.byte_class.shape == (256,) and int(d.byte_class.max()) < 256
    assert d.hit_len.shape == d.hit_id.shape == (257,) and int(d.hit_len.max()) == 64 and int(d.hit_id.max()) == 3
    small = compile_stop(["```", "END"])
    assert small.trans.shape == (7, 5)                                              # `, E, N, D and "other"
    assert len({int(small.byte_class[b]) for b in range(256) if bytes([b]) not in (b"`", b"E", b"N", b"D")}) == 1
    assert sorted(small.hit_len.tolist()) == [0, 0, 0, 0, 0, 3, 3]


# ----------------------------------------------------------------------------- the mock client
def test_canned_client_records_stop_only_when_given():
    c = CannedResponseClient("fine")
    c.chat.completions.create(model="m", messages=[], stop=["```"])
    assert c.calls[-1]["stop"] == ["```"]
    c.chat.completions.create(model="m", messages=[])
    assert "stop" not in c.calls[-1]


def test_agents_vis_stop(monkeypatch):
    from vision_inspection_system_amd import agents
    monkeypatch.delenv("VIS_STOP", raising=False)
    assert agents.stop_kwargs() == {}
    monkeypatch.setenv("VIS_STOP", '["```", "END"]')
    assert agents.stop_kwargs() == {"stop": ["```", "END"]}
    monkeypatch.setenv("VIS_STOP", '"```"')
    assert agents.stop_kwargs() == {"stop": "```"}
    for bad in ("```", "[]", "3", '[""]'):
        monkeypatch.setenv("VIS_STOP", bad)
        with pytest.raises(ValueError):
            agents.stop_kwargs()


# ----------------------------------------------------------------------------- PickStage
V, T, SLOTS, K = 320, 16, 3, 64


@pytest.fixture(scope="module", autouse=True)
def lib():
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
    def __init__(self, tokenizer=None):
        dev = torch.device("cpu")
        self.cfg, self.max_batch, self.device = _Cfg(), SLOTS, dev
        self.tokens_b = torch.zeros((SLOTS, T), dtype=torch.int32, device=dev)
        self.logits_b = torch.zeros((SLOTS, V), dtype=torch.float32, device=dev)
        self.step_b = torch.zeros(SLOTS, dtype=torch.int32, device=dev)
        self.cur_b = torch.zeros(SLOTS, dtype=torch.int32, device=dev)
        self.ws_val = torch.zeros(2048, dtype=torch.float32, device=dev)
        self.ws_idx = torch.zeros(2048, dtype=torch.int32, device=dev)
        self.temperature, self.seed = 0.0, 0
        self.tokenizer = tokenizer
        self._init_pick_stage()


@pytest.fixture
def calls(monkeypatch):
    log = []

    def rec(name):
        def f(*a, **kw):
            log.append((name, a, kw))
        return f

    for name in ("argmax", "argmax_masked", "gemv", "gemv_argmax", "gemv_argmax_masked", "sample", "penalize",
                 "penalty_prompt", "logprobs", "stop_scan"):
        monkeypatch.setattr(hip, name, rec(name))
    return log


def _names(log):
    return [c[0] for c in log]


def _three_picks(eng, B=2):
    """The three pick entry points the way the engines call them: the pick, then the launches that follow a pick."""
    eng._pick(eng.logits_b[:B], eng.ws_val, eng.ws_idx, eng.tokens_b[:B], eng.cur_b[:B], eng.step_b[:B], 0.0, 0)
    eng._logprobs_after_pick(B)
    eng._stop_after_pick(B)
    x, w = torch.zeros(K, dtype=torch.bfloat16), torch.zeros((V, K), dtype=torch.bfloat16)
    eng._gemv_pick(x, w, eng.logits_b[0], eng.ws_val, eng.ws_idx, eng.tokens_b[0], eng.cur_b[0:1], eng.step_b[0:1])
    eng._logprobs_after_pick(1)
    eng._stop_after_pick(1)
    eng._prompt_pick(2, torch.arange(5, dtype=torch.int32), eng.logits_b[2], eng.tokens_b[2], eng.cur_b[2:3], eng.step_b[2:3])


def test_stop_scan_follows_every_pick_when_on(calls):
    eng = Stub(_Tokenizer())
    with eng._pick_request(None, False, None, None, False, None, stop=["ab", "c"]):
        assert eng.stop_on and eng._stop.stops == (b"ab", b"c")
        eng._stop.state[2] = 7                              # stale record of the slot's previous request
        _three_picks(eng)
        assert _names(calls) == ["argmax", "stop_scan", "gemv_argmax", "stop_scan", "argmax", "stop_scan"]
        rows = [c[1][0] for c in calls if c[0] == "stop_scan"]
        st = eng._stop.state
        assert [(r.data_ptr(), r.shape[0]) for r in rows] == [(st.data_ptr(), 2), (st.data_ptr(), 1), (st[2].data_ptr(), 1)]
        assert st[2].tolist() == [0] * stop.STATE_INTS      # the prompt pass's pick starts from a fresh record
        toks = [c[1][1] for c in calls if c[0] == "stop_scan"]
        assert toks[2].data_ptr() == eng.tokens_b[2].data_ptr() and toks[0].shape == (2, T)
        assert calls[1][1][-1] is True                      # EOS ends a row unless the engine runs with ignore_eos
        eng.stop_eos = False
        eng._stop_after_pick(1)
        assert calls[-1][1][-1] is False
    assert not eng.stop_on and eng.stop_eos is True


def test_no_stop_scan_when_off(calls):
    eng = Stub(_Tokenizer())
    for kw in ({}, {"stop": None}):
        with eng._pick_request(None, False, None, None, False, None, **kw):
            _three_picks(eng)
    assert _names(calls) == ["argmax", "gemv_argmax", "argmax"] * 2
    assert eng._stop is None                                # no buffers, no token table, nothing on the device


def test_stop_key_and_pick_key(calls):
    eng = Stub(_Tokenizer())
    base = (None, False, False, None, False, False)
    off = eng._stop_key()
    assert eng._pick_key() == base
    with eng._pick_request(None, False, None, None, False, None, stop="x"):
        assert eng._pick_key() == base                      # the six entries, whatever stop is
        on = eng._stop_key()
        eng.stop_eos = False
        assert eng._stop_key() not in (on, off)             # eos_on is a kernel argument baked into a captured step
    assert on != off and eng._stop_key() == off
    with eng._pick_request(None, False, None, None, False, None, stop=["y", "zz"]):
        assert eng._stop_key() == on                        # the strings live in device tables: one graph serves every set


def test_scope_is_clean_after_a_bad_stop(calls):
    eng = Stub(_Tokenizer())
    entered = []
    for bad in ([], [""], ["a"] * 2 + ["b", "c", "d", "e"], [3]):
        with pytest.raises(ValueError, match="stop"):
            with eng._pick_request(3, False, None, 0.9, True, None, stop=bad):
                entered.append(1)
    with pytest.raises(ValueError, match="tokenizer"):
        with Stub(None)._pick_request(None, False, None, None, False, None, stop="a"):
            entered.append(1)
    assert not entered and not eng.stop_on and eng.lp_k is None and not eng.smp_on and _names(calls) == []


def test_token_table_is_shared_with_the_masks(calls):
    eng = Stub(_Tokenizer())
    with eng._pick_request(None, False, None, None, False, None, stop="a"):
        pass
    with eng._pick_request(None, True, None, None, False, None, stop="a"):
        assert eng._json.off is eng._stop.off and eng._json.table is eng._stop.table


def test_finish_records(calls):
    eng = Stub(_Tokenizer())
    eos = _Cfg.eos_ids
    # stop off: the host's own view, as before
    assert eng._finish([(0, [5, 6, V - 1, 7]), None, (1, [5, 6])], eos, False) == [[5, 6], None, [5, 6]]
    assert eng.last_finish == [("eos", None), None, ("length", None)]
    assert eng._finish([(0, [5, V - 1, 7])], eos, True) == [[5, V - 1, 7]] and eng.last_finish == [("length", None)]
    assert eng._finish([(0, [5, V - 1, 7])], eos, False, keep_eos=True) == [[5, V - 1]]
    with eng._pick_request(None, False, None, None, False, None, stop="a"):
        assert eng.last_finish is None
        st = eng._stop.state
        st[0, stop.REASON], st[0, stop.N_TOKENS], st[0, stop.CUT] = STOP, 2, 3
        st[1, stop.REASON], st[1, stop.N_TOKENS], st[1, stop.CUT] = EOS, 1, 9
        assert eng._finish([(1, [5, 6, 7]), (0, [5, 6, 7]), (2, [5, 6, 7])], eos, False) == [[5], [5, 6], [5, 6, 7]]
        assert eng.last_finish == [("eos", None), ("stop", 3), ("length", None)]
        assert eng._finish([(1, [5, 6, 7])], eos, False, keep_eos=True) == [[5, 6]]
        assert eng._stop_done([0, 1]) and not eng._stop_done([0, 1, 2])


def test_launcher_rejects_bad_arguments_without_gpu(lib):
    P = 4096                                                # never dereferenced: every call below fails a check first

    def call(state=P, tokens=P, max_tokens=16, V=320, cap_states=257, cap_classes=256, eos_on=1, batch=1, hits=P):
        return lib.vis_stop_scan(state, tokens, max_tokens, P, P, P, P, V, P, P, P, hits, cap_states, cap_classes, eos_on, batch, None)

    for kw in (dict(state=None), dict(tokens=None), dict(hits=None), dict(max_tokens=0), dict(V=0), dict(V=262145),
               dict(cap_states=258), dict(cap_states=0), dict(cap_classes=257), dict(eos_on=2), dict(batch=0), dict(batch=65),
               dict(state=P + 8)):
        assert call(**kw) == 1, kw
