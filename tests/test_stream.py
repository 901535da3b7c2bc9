"""Streaming without a GPU: stream.publish_ref (the kernel's restatement) against stop.find_oracle on random byte streams,
the reader's text against the one-shot decode, the client's chunk sequence, the argument checks, and - on a stub PickStage
in the style of tests/test_pick_stage.py - which launches the switch adds and what it leaves alone."""
import os
import random

import numpy as np
import pytest
import torch

from vision_inspection_system_amd import hip, stop, stream
from vision_inspection_system_amd.pick import PickStage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP_SETS = [("ab", "abc", "bca"), ("q" * 64,), ("xy", "xyz"), ("a",), ("ab", "b" * 64, "ba"), None]


@pytest.fixture(scope="module", autouse=True)
def lib():
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    return hip.load()


class _Tok:
    """A byte vocabulary plus multi-byte tokens; id 300 is EOS and has no bytes."""
    EXTRA = [b"ab", b"bc", b"abc", b"bca", b"xyz", b"qqqq", "é".encode(), "日本".encode(), b"\xf0\x9f", b"\x98\x80", b"zab"]

    def token_bytes(self, t: int) -> bytes:
        if t < 256:
            return bytes([t])
        return self.EXTRA[t - 256] if t - 256 < len(self.EXTRA) else b""

    def decode(self, ids):
        return b"".join(self.token_bytes(t) for t in ids).decode("utf-8", errors="replace")


EOS_ID = 300


class _FakeBuffers:
    """StreamBuffers' host side in numpy: what the reader reads."""

    def __init__(self, slots=2, T=256):
        self.T = T
        self.records = np.zeros((slots, T, 4), dtype=np.int32)
        self.count = np.zeros(slots, dtype=np.int32)
        self.start = np.zeros(slots, dtype=np.int32)

    def reset(self, slot):
        self.count[slot] = 0
        self.start[slot] = 0

    def publish(self, slot, pos, tok, rec):
        """What the kernel does for one pick: the record, then the count."""
        if self.count[slot] == 0:
            self.start[slot] = pos
        self.records[slot, pos] = (tok, rec[0], rec[1], rec[2])
        self.count[slot] = pos + 1


def _random_reply(rng, stops):
    alphabet = b"abcqxyz" + (b"".join(s.encode() for s in stops) if stops else b"")
    toks = []
    for _ in range(rng.randint(1, 60)):
        r = rng.random()
        if r < 0.03:
            toks.append(EOS_ID)
        elif r < 0.3:
            toks.append(256 + rng.randrange(len(_Tok.EXTRA)))
        elif stops and r < 0.4:
            toks.extend(rng.choice(stops).encode()[:rng.randint(1, 64)])       # most of a stop string, byte by byte
        else:
            toks.append(rng.choice(alphabet))
    return toks


@pytest.mark.parametrize("stops", STOP_SETS)
def test_publish_ref_against_the_oracle_and_the_reader(stops):
    tok = _Tok()
    rng = random.Random(7)
    for trial in range(120):
        toks = _random_reply(rng, stops)
        tb = [tok.token_bytes(t) for t in toks]
        flags = [t == EOS_ID for t in toks]
        ref = stream.publish_ref(stops, tb, flags)
        if stops:
            oracle = stop.find_oracle(stops, tb, flags)
        else:
            n_eos = flags.index(True) if True in flags else None
            oracle = dict(reason=stop.EOS, n_tokens=n_eos, cut=sum(map(len, tb[:n_eos]))) if n_eos is not None else \
                dict(reason=stop.OPEN, n_tokens=len(toks), cut=0)
        # the last record is the oracle's verdict; an open reply has one record per token
        assert ref[-1][1] == oracle["reason"]
        assert len(ref) == (oracle["n_tokens"] + (1 if oracle["reason"] == stop.EOS else 0))
        stream_bytes = b"".join(tb[:oracle["n_tokens"]])
        final_cut = oracle["cut"] if oracle["reason"] != stop.OPEN else len(stream_bytes)
        safes = [r[0] for r in ref]
        assert all(a <= b for a, b in zip(safes, safes[1:])), (trial, safes)           # never decreases
        assert all(s <= final_cut for s in safes)                                      # never beyond the final cut
        if oracle["reason"] != stop.OPEN:
            assert safes[-1] == final_cut and ref[-1][2] == final_cut                  # ... and equal to it at the end
        assert all(r[1] == stop.OPEN and r[2] == 0 for r in ref[:-1])
        # the reader over the same records, polled after every pick: always a prefix of the final text, equal at the end
        final_text = stream_bytes[:final_cut].decode("utf-8", errors="replace")
        buf = _FakeBuffers()
        reader = stream.StreamReader(tok)
        reader._attach(buf)
        reader._reset(0)
        reader._bind(0, 0, 0)
        text = ""
        for i, rec in enumerate(ref):
            buf.publish(0, 9 + i, toks[i], rec)
            text += "".join(e.text for e in reader.poll())
            assert final_text.startswith(text), (trial, i, text, final_text)
        reader._end_group()
        text += "".join(e.text for e in reader.poll())
        assert text == final_text, (trial, stops, toks)


def _read(tok, toks, stops=None, poll_each=True):
    tb = [tok.token_bytes(t) for t in toks]
    ref = stream.publish_ref(stops, tb, [t == EOS_ID for t in toks])
    buf, reader = _FakeBuffers(), stream.StreamReader(tok)
    reader._attach(buf)
    reader._reset(0)
    reader._bind(0, 0, 0)
    pieces = []
    for i, rec in enumerate(ref):
        buf.publish(0, 3 + i, toks[i], rec)
        if poll_each:
            pieces += [e.text for e in reader.poll()]
    reader._end_group()
    pieces += [e.text for e in reader.poll()]
    return pieces


def test_reader_a_character_split_over_three_tokens_comes_out_once():
    tok = _Tok()
    toks = [ord("a"), 256 + 8, 0x98, 0x80, ord("b")]          # a, F0 9F | 98 | 80 (U+1F600), b
    pieces = _read(tok, toks)
    assert "".join(pieces) == "a\U0001F600b"
    assert sum("\U0001F600" in p for p in pieces) == 1 and not any("�" in p for p in pieces)
    assert pieces[0] == "a"                                    # nothing of the character before its last byte


def test_reader_invalid_bytes_as_the_one_shot_decode():
    tok = _Tok()
    for toks in ([ord("a"), 0xFF, ord("b")], [0xE6, 0x97, ord("x")], [ord("k"), 256 + 8], [0x80, 0x80, 256 + 6]):
        want = b"".join(tok.token_bytes(t) for t in toks).decode("utf-8", errors="replace")
        assert "�" in want
        assert "".join(_read(tok, toks)) == want
        assert "".join(_read(tok, toks, poll_each=False)) == want


def test_reader_drops_what_it_held_back_when_a_stop_string_completes_inside_a_token():
    tok = _Tok()
    toks = [ord("h"), ord("i"), ord("z"), ord("a"), 256 + 1, ord("k")]          # "hiza" + "bc": "ab" completes inside a token
    pieces = _read(tok, toks, stops=("ab", "zac"))
    assert "".join(pieces) == "hiz"
    # "za" was held back as the possible start of "zac" / "ab": "z" is released when "ab" wins, "a" never
    toks = [ord("h"), ord("a"), ord("x")]
    assert _read(tok, toks, stops=("ab",))[:2] == ["h", "ax"]                    # held back, then released with the next pick
    toks = [ord("h"), ord("a")]
    assert "".join(_read(tok, toks, stops=("ab",))) == "ha"                      # a length limit flushes what was held back
    toks = [ord("h"), ord("a"), EOS_ID, ord("b")]
    assert "".join(_read(tok, toks, stops=("ab",))) == "ha"                      # so does EOS


def test_reader_continues_behind_a_request_served_again():
    tok = _Tok()
    toks = [ord(c) for c in "hello"]
    ref = stream.publish_ref(None, [tok.token_bytes(t) for t in toks])
    buf, reader = _FakeBuffers(), stream.StreamReader(tok)
    reader._attach(buf)
    reader._bind(0, 0, 0)
    reader._reset(0)
    out = []
    for i in range(3):
        buf.publish(0, 4 + i, toks[i], ref[i])
    out += [e.text for e in reader.poll()]
    assert "".join(out) == "hel"
    reader._reset(0)                                           # the request is served again from the start
    assert reader.poll() == [] and buf.count[0] == 0
    for i in range(5):
        buf.publish(0, 4 + i, toks[i], ref[i])
        out += [e.text for e in reader.poll()]
    reader._end_group()
    out += [e.text for e in reader.poll()]
    assert "".join(out) == "hello"                             # nothing twice
    # other bytes the second time are an error, not text
    buf, reader = _FakeBuffers(), stream.StreamReader(tok)
    reader._attach(buf)
    reader._bind(0, 0, 0)
    reader._reset(0)
    buf.publish(0, 4, ord("h"), ref[0])
    assert [e.text for e in reader.poll()] == ["h"]
    reader._reset(0)
    buf.publish(0, 4, ord("j"), ref[0])
    with pytest.raises(RuntimeError):
        reader.poll()


def test_reader_cancel_flag():
    r = stream.StreamReader(_Tok())
    assert r.cancelled is False and r.poll() == []
    r.cancel()
    assert r.cancelled is True


# ----------------------------------------------------------------------------- the client
def test_canned_client_chunk_sequence_and_usage():
    """The reference's chat panel loop, unmodified, against the mock provider."""
    from vision_inspection_system_amd.client import ChatCompletion, ChatCompletionChunk, make_client
    client = make_client("mock", reply="two defects")
    s = client.chat.completions.create(model="m", messages=[{"role": "user", "content": "hi"}], temperature=0.3, stream=True)
    assert not isinstance(s, ChatCompletion)
    seen = ""
    for chunk in s:
        if chunk.choices[0].delta.content:
            seen += chunk.choices[0].delta.content
    assert seen == "two defects"
    chunks = list(client.chat.completions.create(model="m", messages=[], stream=True, stream_options={"include_usage": True}))
    assert all(isinstance(c, ChatCompletionChunk) and c.object == "chat.completion.chunk" and c.model == "m" for c in chunks)
    role, content, fin, usage = chunks
    assert (role.choices[0].delta.role, role.choices[0].delta.content, role.choices[0].finish_reason) == ("assistant", "", None)
    assert (content.choices[0].delta.role, content.choices[0].delta.content, content.choices[0].index) == (None, "two defects", 0)
    assert (fin.choices[0].delta.role, fin.choices[0].delta.content, fin.choices[0].finish_reason) == (None, None, "stop")
    assert usage.choices == [] and set(usage.usage) == {"prompt_tokens", "completion_tokens", "total_tokens"}
    assert all(c.usage is None for c in chunks[:3])
    two = list(client.chat.completions.create(model="m", messages=[], stream=True, n=2))
    assert [c.choices[0].index for c in two] == [0, 0, 0, 1, 1, 1]
    for off in (None, False):      # today's call
        assert isinstance(client.chat.completions.create(model="m", messages=[], stream=off), ChatCompletion)
        assert "stream" not in client.calls[-1]


def test_stream_with_logprobs_is_refused():
    from vision_inspection_system_amd.client import LocalVLMClient, make_client
    for client in (make_client("mock"), LocalVLMClient()):
        with pytest.raises(ValueError, match="stream=True together with logprobs=True"):
            client.chat.completions.create(model="synthetic:tiny", messages=[], stream=True, logprobs=True)
    with pytest.raises(ValueError, match="stream=True together with logprobs=True"):
        LocalVLMClient().complete_many("synthetic:tiny", [[]], stream=True, logprobs=True)
    with pytest.raises(ValueError, match="stream_options"):
        make_client("mock").chat.completions.create(model="m", messages=[], stream_options={"include_usage": True})
    with pytest.raises(ValueError, match="stream_options"):
        make_client("mock").chat.completions.create(model="m", messages=[], stream=True, stream_options={"usage": True})


def test_check_stream_refuses_non_bools():
    assert stream.check_stream(None) is False and stream.check_stream(False) is False and stream.check_stream(True) is True
    for bad in (1, 0, "true", "yes", [], 1.0):
        with pytest.raises(ValueError):
            stream.check_stream(bad)
    from vision_inspection_system_amd.client import make_client
    with pytest.raises(ValueError):
        make_client("mock").chat.completions.create(model="m", messages=[], stream=1)


def test_depths_are_the_longest_suffix_that_starts_a_stop_string():
    rng = random.Random(3)
    for stops in [s for s in STOP_SETS if s]:
        dfa = stop.compile_stop(stops)
        depth = stop.depths(dfa)
        bs = [s.encode() for s in stops]
        for _ in range(40):
            text = bytes(rng.choice(b"abcqxyz") for _ in range(rng.randint(0, 12)))
            if rng.random() < 0.5:
                text += rng.choice(bs)[:rng.randint(0, 63)]
            st = 0
            for b in text:
                st = int(dfa.trans[st, dfa.byte_class[b]])
            want = max(k for k in range(len(text) + 1) if any(s.startswith(text[len(text) - k:]) for s in bs))
            assert int(depth[st]) == want, (stops, text)
    assert stop.depths(stop.empty_dfa()).tolist() == [0]


# ----------------------------------------------------------------------------- the switch on a stub PickStage
V, T, SLOTS = 320, 16, 3


class _Cfg:
    vocab, eos_ids = V, (V - 1,)


class _ByteTok:
    def token_bytes(self, t: int) -> bytes:
        return bytes([t]) if t < 256 else b""


class Stub(PickStage):
    def __init__(self):
        dev = torch.device("cpu")
        self.cfg, self.max_batch, self.device = _Cfg(), SLOTS, dev
        self.tokens_b = torch.zeros((SLOTS, T), dtype=torch.int32)
        self.logits_b = torch.zeros((SLOTS, V), dtype=torch.float32)
        self.step_b = torch.zeros(SLOTS, dtype=torch.int32)
        self.cur_b = torch.zeros(SLOTS, dtype=torch.int32)
        self.ws_val = torch.zeros(2048, dtype=torch.float32)
        self.ws_idx = torch.zeros(2048, dtype=torch.int32)
        self.temperature, self.seed = 0.7, 11
        self.tokenizer = _ByteTok()
        self._init_pick_stage()

    def step(self, B):
        """What DecodeStage's steps end with."""
        self._pick(self.logits_b[:B], self.ws_val, self.ws_idx, self.tokens_b[:B], self.cur_b[:B], self.step_b[:B],
                   self.temperature, self.seed)
        self._logprobs_after_pick(B)
        self._stop_after_pick(B)
        self._stream_after_pick(B)


class _FakeHost:
    """hip.HostCoherent without a device: ordinary memory."""

    def __init__(self, nbytes):
        self._mem = np.zeros(nbytes // 4, dtype=np.int32)
        self.nbytes, self.host_ptr, self.dev_ptr = nbytes, self._mem.ctypes.data, self._mem.ctypes.data

    def array(self, offset, shape, dtype="int32"):
        return self._mem[offset // 4: offset // 4 + int(np.prod(shape))].reshape(shape)


@pytest.fixture
def calls(monkeypatch):
    log = []
    for name in ("argmax", "argmax_masked", "gemv", "gemv_argmax", "sample", "penalize", "logprobs", "stop_scan",
                 "stream_publish"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **kw: log.append((_n, a, kw)))
    monkeypatch.setattr(hip, "HostCoherent", _FakeHost)
    return log


def _names(log):
    return [c[0] for c in log]


def _prompt_pick(eng, slot):
    eng._prompt_pick(slot, torch.zeros(4, dtype=torch.int32), eng.logits_b[slot], eng.tokens_b[slot],
                     eng.cur_b[slot:slot + 1], eng.step_b[slot:slot + 1])


def test_stream_off_issues_the_launches_of_before(calls):
    eng = Stub()
    keys = (eng._pick_key(), eng._stop_key(), eng._shape_key())
    with eng._pick_request(None, False, None, None, False, None):
        assert eng.stream_on is False and eng._stream_key() == (False,)
        assert (eng._pick_key(), eng._stop_key(), eng._shape_key()) == keys
        _prompt_pick(eng, 0)
        eng.step(2)
    assert _names(calls) == ["argmax", "argmax"]
    del calls[:]
    with eng._pick_request(None, False, None, None, False, None, stop=["ab"]):
        _prompt_pick(eng, 1)
        eng.step(3)
    assert _names(calls) == ["argmax", "stop_scan", "argmax", "stop_scan"]
    assert eng._stream is None


def test_stream_on_adds_one_launch_behind_the_stop_scan(calls):
    eng = Stub()
    off = (eng._pick_key(), eng._stop_key(), eng._shape_key())
    reader = stream.StreamReader(eng.tokenizer)
    with eng._pick_request(None, False, None, None, False, None, on_stream=reader):
        assert eng.stream_on and eng.stop_on and eng._stream_key() == (True,)
        assert eng._pick_key() == off[0] and eng._shape_key() == off[2] and eng._stop_key() == (True, True)
        assert eng._stop.dfa.stops == () and eng._stop.header.tolist() == [1, 1, 0, 0]       # the start state alone
        _prompt_pick(eng, 1)
        eng.step(3)
    assert _names(calls) == ["argmax", "stop_scan", "stream_publish", "argmax", "stop_scan", "stream_publish"]
    first, second = calls[2][1], calls[5][1]
    assert first[0].data_ptr() == eng._stop.state[1:2].data_ptr() and first[1].shape == (1, T)      # the slot's rows
    assert second[0].data_ptr() == eng._stop.state.data_ptr() and second[1].shape == (3, T) and second[2].numel() == 3
    assert first[5] == second[5] + 1 * T * 16 and first[6] == T                                       # records of slot 1
    assert (eng.stream_on, eng.stop_on, eng._reader) == (False, False, None)
    assert eng._stream_key() == (False,) and (eng._pick_key(), eng._stop_key(), eng._shape_key()) == off
    del calls[:]
    eng._stream.count[:] = 9           # what a request leaves behind is not there when the next one begins
    # with the request's own stop strings the scan runs on their automaton and the depth table is theirs
    with eng._pick_request(None, False, None, None, False, None, stop=["abc", "b"], on_stream=stream.StreamReader(eng.tokenizer)):
        assert eng._stop.dfa.stops == (b"abc", b"b")
        assert eng._stream.depth[:5].tolist() == stop.depths(eng._stop.dfa).tolist()
        assert eng._stream.count.tolist() == [0] * SLOTS
        eng.step(1)
    assert _names(calls) == ["argmax", "stop_scan", "stream_publish"]
    # the switch is off again however the request ends
    with pytest.raises(RuntimeError):
        with eng._pick_request(None, False, None, None, False, None, on_stream=stream.StreamReader(eng.tokenizer)):
            raise RuntimeError("boom")
    assert (eng.stream_on, eng.stop_on) == (False, False)
    with pytest.raises(ValueError, match="logprobs"):
        with eng._pick_request(3, False, None, None, False, None, on_stream=stream.StreamReader(eng.tokenizer)):
            pass
    with pytest.raises(ValueError):
        with eng._pick_request(None, False, None, None, False, None, on_stream=object()):
            pass


def test_wrapper_refusals_need_no_gpu(lib):
    P = 4096        # never dereferenced: every call below fails a check first
    ok = [P, P, 16, P, P, 257, P, P, 16, P, P, 3, None]
    for i, bad in [(0, None), (1, None), (3, None), (4, None), (6, None), (7, None), (9, None), (10, None), (0, P + 8),
                   (7, P + 8), (1, P + 2), (9, P + 2), (11, 0), (11, 65), (8, 15), (2, 0), (5, 0), (5, 258)]:
        args = list(ok)
        args[i] = bad
        assert lib.vis_stream_publish(*args) == 1, (i, bad)
    assert lib.vis_host_free(None) == 1
