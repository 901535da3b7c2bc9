"""Streaming on MI355X: vis_stream_publish against its Python restatement (stream.publish_ref) record for record and count
for count, and the engines / the client streamed against the same call not streamed - text, finish reasons and usage equal
under every request switch, eager and graph-replayed, the switch off again afterwards, cancellation, and the one liveness
condition the kernel exists for: text is handed out while the decode loop is still running."""
import os
import threading

import numpy as np
import pytest
import torch

from vision_inspection_system_amd import hip, stop, stream
from vision_inspection_system_amd import json_grammar as G

pytestmark = pytest.mark.gpu
V, T = 320, 16
GUARD = 0x5A5A5A5A
STOPS = ("ab", "abc", "bca")


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


# ----------------------------------------------------------------------------- 1. the kernel
class _Vocab:
    """ids 0..255 the single bytes, then multi-byte pieces, the last id EOS."""
    PIECES = [b"ab", b"bc", b"ca", b"abc", b"xa", b"bca", "é".encode(), "日本".encode(), b"\xf0\x9f", b"\x98\x80", b"", b"cab"]

    def token_bytes(self, t: int) -> bytes:
        return bytes([t]) if t < 256 else self.PIECES[(t - 256) % len(self.PIECES)]


class _Share:
    def __init__(self, table):
        d = "cuda:0"
        self.table = table
        self.off, self.data = torch.from_numpy(table.off).to(d), torch.from_numpy(table.data).to(d)
        self.flags, self.eos = torch.from_numpy(table.flags).to(d), torch.from_numpy(table.eos_ids).to(d)


@pytest.fixture(scope="module")
def table(device):
    return G.build_token_table(_Vocab(), V, [V - 1])


class _Host:
    """records [B, T, 4] | guard | count [B] | start [B] | guard in one coherent allocation."""
    G_INTS = 64

    def __init__(self, B):
        rec = B * T * 16
        self.mem = hip.HostCoherent(rec + 2 * self.G_INTS * 4 + 2 * B * 4)
        self.records = self.mem.array(0, (B, T, 4))
        self.g1 = self.mem.array(rec, (self.G_INTS,))
        self.count_off = rec + self.G_INTS * 4
        self.count = self.mem.array(self.count_off, (B,))
        self.start_off = self.count_off + B * 4
        self.start = self.mem.array(self.start_off, (B,))
        self.g2 = self.mem.array(self.start_off + B * 4, (self.G_INTS,))
        self.g1[:] = GUARD
        self.g2[:] = GUARD

    def snapshot(self):
        return self.records.copy(), self.count.copy(), self.start.copy()

    def guards_intact(self):
        return bool((self.g1 == GUARD).all() and (self.g2 == GUARD).all())


def _rows(B, N, eos):
    """Row 0 ends on a stop string that two tokens spell, row 1 on EOS, the others stay open or end by chance: they draw
    from letters that walk the automaton up and down and from the multi-byte pieces."""
    rng = np.random.default_rng(B)
    rows = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        if b % 4 == 2:
            rows[b] = rng.choice([ord("a"), ord("c"), ord("x"), ord("f"), 256 + 4, 256 + 6, 256 + 7, 256 + 8], N)      # no b: never matches
        else:
            rows[b] = rng.choice([ord("a"), ord("b"), ord("c"), ord("x"), 256, 257, 258, 260, 261, 262, 266, 267], N) \
                if b >= 3 else rng.choice([ord("c"), ord("x"), ord("y")], N)
    rows[0, 3:6] = [ord("x"), ord("a"), ord("b")]
    if B > 1:
        rows[1, 4] = eos
    return rows


@pytest.mark.parametrize("B", [1, 3, 64])
def test_kernel_against_publish_ref(table, B):
    P0, N = 5, T - 5                                    # the last pick lands on the row's last position: step == T
    dev = stop.StopBuffers(None, V, table.eos_ids, B, "cuda:0", share=_Share(table))
    dfa = dev.load(STOPS)
    depth = torch.zeros(stop.MAX_STATES, dtype=torch.uint8)
    depth[:len(stop.depths(dfa))] = torch.from_numpy(stop.depths(dfa))
    depth = depth.cuda()
    pub = torch.zeros(B, dtype=torch.int32, device="cuda")
    host = _Host(B)
    rows = _rows(B, N, int(table.eos_ids[0]))
    tokens = torch.full((B, T), 7, dtype=torch.int32)
    tokens[:, P0:] = torch.from_numpy(rows)
    tokens = tokens.cuda()
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    d = host.mem.dev_ptr

    def launch():
        dev.scan(tokens, step, 0, True)
        hip.stream_publish(dev.state, tokens, step, depth, pub, d, T, d + host.count_off, d + host.start_off)
        torch.cuda.synchronize()

    def want(n):
        recs, count = np.zeros((B, T, 4), dtype=np.int32), np.zeros(B, dtype=np.int32)
        for b in range(B):
            toks = [int(t) for t in rows[b, :n]]
            ref = stream.publish_ref(dfa, [table.tokens[t] for t in toks], [bool(table.flags[t] & G.FLAG_EOS) for t in toks])
            for i, (safe, status, cut) in enumerate(ref):
                recs[b, P0 + i] = (toks[i], safe, status, cut)
            count[b] = P0 + len(ref)
        return recs, count

    ended = set()
    for n in range(1, N + 2):                           # the last one: step == T + 1, nothing may be written
        step.fill_(P0 + n)
        launch()
        got = host.snapshot()
        launch()                                        # the same step again (a graph's warm-up): nothing changes
        again = host.snapshot()
        assert all(np.array_equal(x, y) for x, y in zip(got, again)), ("relaunch", n)
        recs, count = want(min(n, N))
        assert np.array_equal(got[0], recs), (n, np.argwhere(got[0] != recs)[:4])
        assert np.array_equal(got[1], count), (n, got[1], count)
        assert (got[2] == P0).all()
        assert host.guards_intact()
        ended |= {b for b in range(B) if recs[b, count[b] - 1, stream.STATUS] != stream.OPEN}
    final = host.snapshot()
    assert 0 in ended and final[0][0, final[1][0] - 1, stream.STATUS] == stream.STOP
    assert final[1][0] == P0 + 6 and final[0][0, P0 + 5, stream.CUT] == final[0][0, P0 + 5, stream.SAFE]      # "ab" over two tokens
    if B > 1:
        assert final[1][1] == P0 + 5 and final[0][1, P0 + 4, stream.STATUS] == stream.EOS
    if B > 2:
        assert final[1][2] == T and final[0][2, T - 1, stream.STATUS] == stream.OPEN                        # open to the last position
    # an ended row launched again, many steps later, stays as it is: covered by every later n above (count frozen)
    assert pub.cpu().tolist() == final[1].tolist()
    host.mem.free()


def test_wrapper_refusals(device):
    lib = hip.load()
    P = 4096        # never dereferenced: every call below fails a check first

    def call(stop_state=P, tokens=P, max_tokens=16, step=P, depth=P, n_states=257, pub=P, records=P, capacity=16, count=P,
             start=P, batch=3):
        return lib.vis_stream_publish(stop_state, tokens, max_tokens, step, depth, n_states, pub, records, capacity, count,
                                      start, batch, None)

    for name in ("stop_state", "tokens", "step", "depth", "pub", "records", "count", "start"):
        assert call(**{name: None}) == 1, name
    assert call(stop_state=P + 8) == 1 and call(records=P + 8) == 1                 # 16-byte alignment
    for name in ("tokens", "step", "pub", "count", "start"):
        assert call(**{name: P + 2}) == 1, name
    assert call(batch=0) == 1 and call(batch=65) == 1
    assert call(capacity=15) == 1 and call(max_tokens=0) == 1
    assert call(n_states=0) == 1 and call(n_states=258) == 1
    import ctypes
    h, dv = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.vis_host_coherent_alloc(None, ctypes.addressof(dv), 64) == 1
    assert lib.vis_host_coherent_alloc(ctypes.addressof(h), ctypes.addressof(dv), 0) == 1
    assert lib.vis_host_free(None) == 1


# ----------------------------------------------------------------------------- 2. engines and client
def _msgs(tmp_path, seed):
    from PIL import Image
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    p = tmp_path / f"img{seed}.png"
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    url = encode_image_optimized(str(p), 256)
    return [{"role": "user", "content": [{"type": "text", "text": "Inspect this part and describe every defect you find. " * 3},
                                         {"type": "image_url", "image_url": {"url": url}}]}]


def _drain(chunks):
    """A chunk sequence -> {(request, choice): (text, finish_reason)}, {request: usage}; the order per choice is checked."""
    state, text, fin, usage = {}, {}, {}, {}
    for ch in chunks:
        assert ch.object == "chat.completion.chunk"
        if not ch.choices:
            usage[ch.request_index] = ch.usage
            continue
        (c,) = ch.choices
        key = (ch.request_index, c.index)
        if c.delta.role is not None:
            assert key not in state and c.delta.role == "assistant" and c.delta.content == ""
            state[key] = "open"
        elif c.finish_reason is not None:
            assert state.get(key) == "open" and c.delta.content is None
            state[key], fin[key] = "done", c.finish_reason
        else:
            assert state.get(key) == "open" and c.delta.content
            text[key] = text.get(key, "") + c.delta.content
    assert set(state.values()) <= {"done"}
    return {k: (text.get(k, ""), fin[k]) for k in state}, usage


MODELS = ["synthetic:tiny", "synthetic:mllama-tiny"]
CONFIGS = {
    "greedy": {},
    "sampled": dict(temperature=0.8, seed=3),
    "stop": dict(temperature=0.8, seed=3),          # + stop=, two bytes from the middle of the reply
    "json": dict(temperature=0.8, seed=3, response_format={"type": "json_object"}),
    "n3": dict(temperature=0.8, seed=3, n=3),
}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_streamed_equals_not_streamed(device, tmp_path, model, config):
    from vision_inspection_system_amd.client import ChatCompletion, LocalVLMClient, get_model
    c = LocalVLMClient()
    m = _msgs(tmp_path, 1)
    kw = dict(max_tokens=24, **CONFIGS[config])
    if config == "stop":
        plain = c.chat.completions.create(model=model, messages=m, logprobs=True, **kw)
        raw = b"".join(bytes(e.bytes) for e in plain.choices[0].logprobs.content)      # the reply's bytes, token by token
        assert len(raw) >= 8
        kw["stop"] = [raw[5:7]]                          # two tokens of the byte vocabulary spell it
        sizes = np.cumsum([len(e.bytes) for e in plain.choices[0].logprobs.content])
        through = int(np.searchsorted(sizes, 7)) + 1     # the token that brings the reply to 7 bytes completes it at the latest
    want = c.chat.completions.create(model=model, messages=m, **kw)
    assert isinstance(want, ChatCompletion)
    got, usage = _drain(c.chat.completions.create(model=model, messages=m, stream=True,
                                                  stream_options={"include_usage": True}, **kw))
    assert got == {(0, ch.index): (ch.message.content, ch.finish_reason) for ch in want.choices}
    assert usage == {0: want.usage}
    if config == "stop":
        assert want.choices[0].finish_reason == "stop" and want.usage["completion_tokens"] <= through
        assert len(want.choices[0].message.content.encode("utf-8")) < len(raw.decode("utf-8", errors="replace").encode("utf-8"))
    eng = get_model(model).engine
    assert eng.stream_on is False and eng.stop_on is False
    # the same request not streamed afterwards: the switch went off and the graphs are keyed apart
    after = c.chat.completions.create(model=model, messages=m, **kw)
    assert after.choices == want.choices and after.usage == want.usage


@pytest.mark.parametrize("model", MODELS)
def test_complete_many_streams_every_request(device, tmp_path, model):
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    batch = [_msgs(tmp_path, s) for s in range(5)]
    kw = dict(temperature=0.8, seed=3, max_tokens=16)
    want = c.complete_many(model, batch, **kw)
    got, usage = _drain(c.complete_many(model, batch, stream=True, stream_options={"include_usage": True}, **kw))
    assert got == {(j, 0): (r.choices[0].message.content, r.choices[0].finish_reason) for j, r in enumerate(want)}
    assert usage == {j: r.usage for j, r in enumerate(want)}


def _text_ids(lm):
    from vision_inspection_system_amd.tokenizer import build_chat_ids
    return build_chat_ids(lm.tokenizer, [{"role": "user", "content": "Describe the part."}], [])


def test_eager_and_graph_replayed(device):
    from vision_inspection_system_amd.client import get_model
    lm = get_model("synthetic:tiny")
    eng, ids = lm.engine, _text_ids(lm)
    with eng.lock:
        want = eng.generate(ids, (), max_new_tokens=24, temperature=0.8, seed=5)
        fin = eng.last_finish
        for use_graph in (False, True):
            reader = stream.StreamReader(lm.tokenizer)
            toks = eng.generate(ids, (), max_new_tokens=24, temperature=0.8, seed=5, use_graph=use_graph, on_stream=reader)
            assert toks == want and eng.last_finish == fin
            events = reader.poll()                       # the run is over: everything is in the queue
            assert all((e.request, e.choice) == (0, 0) for e in events)
            assert "".join(e.text for e in events) == lm.tokenizer.decode(want)
            assert reader.poll() == []
            assert eng.stream_on is False and eng.stop_on is False
        assert eng.generate(ids, (), max_new_tokens=24, temperature=0.8, seed=5) == want
        with pytest.raises(ValueError, match="logprobs"):
            eng.generate(ids, (), max_new_tokens=4, logprobs=2, on_stream=stream.StreamReader(lm.tokenizer))
        assert eng.stream_on is False


def test_cancel_ends_the_call_and_leaves_the_engine_usable(device, tmp_path, monkeypatch):
    from vision_inspection_system_amd.client import LocalVLMClient, get_model
    monkeypatch.setenv("VIS_IGNORE_EOS", "1")
    c = LocalVLMClient()
    m = _msgs(tmp_path, 2)
    want = c.chat.completions.create(model="synthetic:tiny", messages=m, max_tokens=24)
    s = c.chat.completions.create(model="synthetic:tiny", messages=m, max_tokens=900, stream=True)
    for ch in s:
        if ch.choices[0].delta.content:
            break
    s.close()                                            # joins the worker: nothing is left running
    assert s.worker_done.is_set()
    eng = get_model("synthetic:tiny").engine
    steps = eng.last_timing["decode_steps"]
    print(f"cancelled after {steps} of 899 decode steps")
    assert steps < 899 and eng.last_finish == [("length", None)]
    assert eng.stream_on is False and eng.stop_on is False
    again = c.chat.completions.create(model="synthetic:tiny", messages=m, max_tokens=24)
    assert again.choices == want.choices


def test_text_is_handed_out_while_the_loop_runs(device):
    """256 tokens with check_every=256: after the prompt pass the loop launches 255 steps and then blocks on one D2H.  The
    first text must be in the reader's hands before the engine call has returned - it fails only if what the kernel publishes
    is not visible to the host while the loop runs."""
    from vision_inspection_system_amd.client import get_model
    lm = get_model("synthetic:tiny")
    eng, ids = lm.engine, _text_ids(lm)
    reader = stream.StreamReader(lm.tokenizer)
    returned = threading.Event()
    box = {}

    def work():
        try:
            with eng.lock:
                box["toks"] = eng.generate(ids, (), max_new_tokens=256, ignore_eos=True, check_every=256, on_stream=reader)
        finally:
            returned.set()

    th = threading.Thread(target=work)
    th.start()
    first_before_return = None
    text = ""
    while True:
        over = returned.is_set()
        events = reader.poll()
        if events and first_before_return is None:
            first_before_return = not over
        text += "".join(e.text for e in events)
        if over:
            break
        if not events:
            returned.wait(0.0005)
    th.join()
    assert len(box["toks"]) == 256
    assert text == lm.tokenizer.decode(box["toks"])
    assert first_before_return is True
