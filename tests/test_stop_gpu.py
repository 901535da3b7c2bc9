"""Stop strings on MI355X: vis_stop_scan against its Python restatement (stop.scan) pick by pick, the engines' replies cut
where scan says - single, batched, eager, graph-replayed - and the client's text, usage and finish_reason."""
import os
import random

import numpy as np
import pytest
import torch

from helpers import load_golden
from vision_inspection_system_amd import hip, stop
from vision_inspection_system_amd import json_grammar as G
from vision_inspection_system_amd.stop import EOS, OPEN, STOP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HF = os.path.join(HERE, "golden", "hf_dirs")
MARK = b"\x02\x03\x04"          # spelled by three single-byte tokens no other token of the synthetic vocabulary contains


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


class _Vocab:
    """The synthetic vocabulary of test_json_mode_gpu.py: ids 0..255 the single bytes, then random JSON-heavy byte strings
    of 1..40 bytes, a few ids without bytes."""

    def __init__(self, V: int, seed: int):
        rng = random.Random(seed)
        pieces = [b"{", b"}", b"[", b"]", b'"', b":", b",", b" ", b"\n", b"  ", b"\\", b"\\n", b"\\u00e9", b"0", b"1", b"9",
                  b"-", b".", b"e", b"E+", b"true", b"false", b"null", b"abc", b"key", b"_x", "é".encode(), "日本".encode(),
                  "😀".encode(), b"\xe6", b"\x97", b"\xa5", b"\xf0\x9f", b"\x98\x80", b"\x01", b"\xff", b"\t", b"/"]
        self.toks = [bytes([b]) for b in range(256)]
        while len(self.toks) < V:
            self.toks.append(b"".join(rng.choice(pieces) for _ in range(rng.randint(1, 12)))[:rng.randint(1, 40)])
        for t in range(300, V, 997):
            self.toks[t] = b""

    def token_bytes(self, t: int) -> bytes:
        return self.toks[t]


class _Dev:
    """The device side of one stop set over one token table, as StopBuffers lays it out."""

    def __init__(self, table, stops, B):
        self.buf = stop.StopBuffers(None, table.vocab, table.eos_ids, B, "cuda:0", share=_Share(table))
        self.dfa = self.buf.load(stops)
        self.table = table

    def launch(self, tokens, step, eos_on=True):
        self.buf.scan(tokens, step, 0, eos_on)

    def records(self):
        return self.buf.state.cpu().numpy().copy()


class _Share:
    def __init__(self, table):
        d = "cuda:0"
        self.table = table
        self.off, self.data = torch.from_numpy(table.off).to(d), torch.from_numpy(table.data).to(d)
        self.flags, self.eos = torch.from_numpy(table.flags).to(d), torch.from_numpy(table.eos_ids).to(d)


def _want(dfa, table, row, n, eos_on=True):
    toks = [int(t) for t in row[:n]]
    flags = [bool(table.flags[t] & G.FLAG_EOS) and eos_on for t in toks]
    return stop.scan(dfa, [table.tokens[t] for t in toks], flags)


def _check(rec, want, what):
    got = dict(reason=int(rec[stop.REASON]), n_tokens=int(rec[stop.N_TOKENS]), cut=int(rec[stop.CUT]),
               which=int(rec[stop.WHICH]), bytes_so_far=int(rec[stop.BYTES]), state=int(rec[stop.STATE]))
    assert got == want, (what, got, want)
    assert int(rec[stop.ANCHOR]) == 1


def _step_through(dev, rows, P0, T, eos_on=True, stride=1):
    """Rows of generated tokens laid at positions P0.. of [B, T]; one launch per ``stride`` picks; the records against scan
    after every launch, a relaunch at the same step bit-identical.  Returns the records per launch."""
    B, N = rows.shape
    tokens = torch.full((B, T), 7, dtype=torch.int32)
    tokens[:, P0:P0 + N] = torch.from_numpy(rows)
    tokens = tokens.cuda()
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    dev.buf.state.zero_()
    history = []
    done_at = {}
    for n in list(range(1, N + 1, stride)) + ([N] if (N - 1) % stride else []):
        step.fill_(P0 + n)
        dev.launch(tokens, step, eos_on)
        recs = dev.records()
        dev.launch(tokens, step, eos_on)                       # the engines replay a step while they warm a graph up
        assert np.array_equal(dev.records(), recs), ("relaunch", n)
        for b in range(B):
            if b in done_at:                                   # a finished row keeps its record while the others go on
                assert np.array_equal(recs[b], history[-1][b]), (b, n)
                continue
            want = _want(dev.dfa, dev.table, rows[b], n, eos_on)
            _check(recs[b], want, (b, n))
            if want["reason"] != OPEN:
                done_at[b] = n
        history.append(recs)
    return history, done_at


@pytest.fixture(scope="module")
def big(device):
    V = 152064
    return G.build_token_table(_Vocab(V, seed=11), V, [V - 3, V - 1])


def _crafted_rows(table, B, N, seed):
    """Row b: random tokens with MARK spelled so that it ends at token position 15 + b % 3 (the poll's edge at 16).  The first
    six rows draw from letters only (nothing else matches first); the others from the whole vocabulary, EOS ids included."""
    rng = np.random.default_rng(seed)
    V = table.vocab
    rows = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        if b < 6:
            rows[b] = rng.integers(ord("f"), ord("z"), N)
        else:
            ids = rng.integers(5, V, N)
            if b % 5 == 0:
                ids[rng.integers(0, N)] = table.eos_ids[b % len(table.eos_ids)]
            rows[b] = ids
        end = 15 + b % 3
        rows[b, end - 2:end + 1] = list(MARK)
    return rows


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("stops", [[MARK], [MARK, b"null,", "日本".encode(), b"E+E+"]], ids=["1stop", "4stops"])
def test_kernel_follows_scan_synthetic_vocab(big, B, stops):
    dev = _Dev(big, stops, B)
    rows = _crafted_rows(big, B, 40, seed=B)
    history, done_at = _step_through(dev, rows, P0=3, T=64)
    final = history[-1]
    ends = {int(final[b][stop.N_TOKENS]) for b in range(min(B, 6))}
    assert ends == ({16, 17, 18} if B > 1 else {16})           # the match ends at token positions 15, 16, 17
    for b in range(min(B, 6)):
        assert final[b][stop.REASON] == STOP and final[b][stop.WHICH] == 0 and final[b][stop.CUT] == 13 + b % 3
    assert len(done_at) == B                                   # every row ended, by MARK at the latest
    if B > 1:
        assert len(set(done_at.values())) > 4                  # rows finish at different steps
        reasons = {int(final[b][stop.REASON]) for b in range(B)}
        assert reasons == {EOS, STOP}
        if len(stops) > 1:
            assert {int(final[b][stop.WHICH]) for b in range(B) if final[b][stop.REASON] == STOP} >= {0, 1}
    # several picks folded by one launch give the same records
    again, _ = _step_through(dev, rows, P0=3, T=64, stride=3)
    assert np.array_equal(again[-1][:, [stop.REASON, stop.N_TOKENS, stop.CUT, stop.WHICH]],
                          final[:, [stop.REASON, stop.N_TOKENS, stop.CUT, stop.WHICH]])
    # EOS ids folded as tokens without bytes (an ignore_eos run): no row ends on EOS, MARK still ends every row
    quiet, _ = _step_through(dev, rows, P0=3, T=64, eos_on=False)
    assert all(int(r[stop.REASON]) == STOP for r in quiet[-1])


@pytest.mark.parametrize("name,V", [("qwen2vl_tiny", 520), ("mllama_tiny", 513)])
@pytest.mark.parametrize("B", [1, 64])
def test_kernel_follows_scan_golden_tokenizers(name, V, B):
    pytest.importorskip("tokenizers")
    from vision_inspection_system_amd.tokenizer import HFTokenizer, LlamaHFTokenizer
    tok = HFTokenizer(os.path.join(HF, name), 500, 501, 502, [503, 505]) if name == "qwen2vl_tiny" else \
        LlamaHFTokenizer(os.path.join(HF, name), 510, [501])
    eos = [503, 505] if name == "qwen2vl_tiny" else list(tok.eos_ids)
    table = G.build_token_table(tok, V, eos)
    rng = np.random.default_rng(7)
    rows = rng.integers(0, V, (B, 40)).astype(np.int32)
    rows[:, :12][np.isin(rows[:, :12], eos)] = 65              # no EOS before the strings below can match
    stream = b"".join(table.tokens[int(t)] for t in rows[0])
    ends = np.cumsum([len(table.tokens[int(t)]) for t in rows[0]])
    # out of row 0's own bytes: one string across the boundary behind token 15, one across 16 | 17, one that is nowhere
    stops = [stream[ends[15] - 2:ends[15] + 1], stream[ends[16] - 1:ends[16] + 2], b"\x00nowhere\x00"]
    assert all(len(s) == 3 for s in stops[:2])
    dev = _Dev(table, stops, B)
    history, done_at = _step_through(dev, rows, P0=5, T=64)
    assert history[-1][0][stop.REASON] == STOP and 0 in done_at
    if B > 1:
        assert len({int(r[stop.REASON]) for r in history[-1]}) > 1


# ----------------------------------------------------------------------------- engines
def _qwen_engine(device, **kw):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, **kw)
    eng.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    return cfg, eng


def _mllama_engine(device, **kw):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, **kw)
    eng.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
    return cfg, eng


N_NEW = 48
ABSENT = b"\x00\x00never\x00"


def _bytes_of(eng, toks, eos_ids):
    return [b"" if t in eos_ids else eng.tokenizer.token_bytes(t) for t in toks]


def _pick_stops(eng, toks, eos_ids, around):
    """Out of one reply's bytes: a string that spans a token boundary (the bytes of the first three tokens that have any,
    from token ``around`` on) and one inside a token (the bytes of one later token); both exist, asserted."""
    tb = _bytes_of(eng, toks, eos_ids)
    print("reply bytes per token:", tb)
    have = [i for i in range(around, len(tb)) if tb[i]]
    assert len(have) >= 4, "no boundary-spanning stop string in this reply"
    span = tb[have[0]] + tb[have[1]] + tb[have[2]]
    assert len(span) > max(len(tb[i]) for i in have[:3])
    return span, tb[have[-1]]


def _spread_stops(eng, firsts, eos_ids, windows):
    """One boundary-spanning string out of each reply (row b's from a token in ``windows[b]``) such that under the whole set
    every row ends on a stop string and no two rows end at the same step; exists, asserted."""
    import itertools
    tbs = [_bytes_of(eng, f, eos_ids) for f in firsts]
    cands = []
    for tb, win in zip(tbs, windows):
        have = [i for i in range(len(tb)) if tb[i]]
        cands.append([tb[have[k]] + tb[have[k + 1]] + tb[have[k + 2]] for k in range(len(have) - 2) if have[k] in win])
    for combo in itertools.product(*cands):
        if len(set(combo)) < len(combo):
            continue
        ends = [stop.scan(list(combo), tb) for tb in tbs]
        if all(e["reason"] == STOP for e in ends) and len({e["n_tokens"] for e in ends}) == len(ends):
            return list(combo)
    raise AssertionError("no stop set that ends the rows at different steps in these replies")


def _expect(eng, first, eos_ids, stops, honour_eos, keep_eos=False):
    """What a rerun of ``first`` (the tokens of a run without stop strings) must return under ``stops``."""
    flags = [honour_eos and t in eos_ids for t in first]
    want = stop.scan(list(stops), _bytes_of(eng, first, eos_ids), flags)
    n = want["n_tokens"] + (1 if keep_eos and want["reason"] == EOS else 0)
    toks = first[:n] if want["reason"] != OPEN else list(first)
    return toks, (stop.REASONS[want["reason"]], want["cut"] if want["reason"] == STOP else None), want


def test_qwen_engine_single(device):
    cfg, eng = _qwen_engine(device, decode_splits=4)
    eos = set(cfg.eos_ids)
    g = load_golden()
    ids, fr = g["ids_a"].tolist(), [torch.from_numpy(g["frame_a"]).to(device)]
    first = eng.generate(ids, fr, max_new_tokens=N_NEW, ignore_eos=True)
    assert len(first) == N_NEW and eng.last_finish == [("length", None)]
    span, inner = _pick_stops(eng, first, eos, around=13)
    for stops in ([span], [inner], [span, inner, ABSENT], [ABSENT]):
        for use_graph in (False, True):
            for ignore_eos in (True, False):
                toks, fin, want = _expect(eng, first, eos, stops, not ignore_eos)
                got = eng.generate(ids, fr, max_new_tokens=N_NEW, ignore_eos=ignore_eos, use_graph=use_graph, stop=stops)
                assert got == toks, (stops, use_graph, ignore_eos)
                assert eng.last_finish == [fin]
                assert not eng.stop_on
    toks, fin, want = _expect(eng, first, eos, [span], False)
    assert fin[0] == "stop" and want["n_tokens"] < N_NEW and b"".join(_bytes_of(eng, toks, eos))[want["cut"]:] == span
    toks, fin, _ = _expect(eng, first, eos, [ABSENT], False)
    assert toks == first and fin == ("length", None)
    # logprobs cover exactly the returned tokens
    toks, _, _ = _expect(eng, first, eos, [span], False)
    assert eng.generate(ids, fr, max_new_tokens=N_NEW, ignore_eos=True, stop=[span], logprobs=2) == toks
    assert len(eng.last_logprobs[0].token_logprobs) == len(toks)
    # afterwards the engine launches what it launched before
    assert eng.generate(ids, fr, max_new_tokens=N_NEW, ignore_eos=True) == first and eng.last_finish == [("length", None)]
    # a reply max_new_tokens cut off says so; so does one that ended on EOS (host-derived, stop off)
    short = eng.generate(ids, fr, max_new_tokens=4)
    assert eng.last_finish == [("eos", None) if len(short) < 4 else ("length", None)]


def test_qwen_engine_batched(device):
    cfg, eng = _qwen_engine(device, max_batch=4)
    eos = set(cfg.eos_ids)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fa), ([256, 72, 105, 33, 90, 41], []), (g["ids_a"].tolist()[:-1] + [77, 10], fa)]
    first = eng.generate_batch(reqs, max_new_tokens=N_NEW, ignore_eos=True)
    assert eng.last_finish == [("length", None)] * 3
    s0, s1, s2 = _spread_stops(eng, first, eos, [range(2, 14), range(16, 28), range(30, 42)])
    for stops in ([s0, s1, s2], [s1, ABSENT], [ABSENT]):
        exp = [_expect(eng, f, eos, stops, False) for f in first]
        for use_graph in (False, True):
            got = eng.generate_batch(reqs, max_new_tokens=N_NEW, ignore_eos=True, use_graph=use_graph, stop=stops)
            assert got == [e[0] for e in exp], (stops, use_graph)
            assert eng.last_finish == [e[1] for e in exp]
    exp = [_expect(eng, f, eos, [s0, s1, s2], False) for f in first]
    assert all(e[1][0] == "stop" for e in exp) and len({e[2]["n_tokens"] for e in exp}) == 3, "rows must finish at different steps"
    exp = [_expect(eng, f, eos, [s0, s1, s2], True) for f in first]
    assert eng.generate_batch(reqs, max_new_tokens=N_NEW, stop=[s0, s1, s2]) == [e[0] for e in exp]
    assert eng.last_finish == [e[1] for e in exp]
    assert eng.generate_batch(reqs, max_new_tokens=N_NEW, ignore_eos=True) == first


def test_mllama_engine(device):
    cfg, eng = _mllama_engine(device, max_batch=4)
    eos = set(cfg.eos_ids)
    gm = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    ids, frame = gm["a_ids"].tolist(), torch.from_numpy(gm["a_image"]).to(device)
    first = eng.generate(ids, frame, max_new_tokens=N_NEW, stop_on_eos=False)
    assert len(first) == N_NEW and eng.last_finish == [("length", None)]
    span, inner = _pick_stops(eng, first, eos, around=13)
    for stops in ([span], [inner, ABSENT], [ABSENT]):
        for use_graph in (False, True):
            for on_eos in (False, True):
                toks, fin, _ = _expect(eng, first, eos, stops, on_eos, keep_eos=True)
                got = eng.generate(ids, frame, max_new_tokens=N_NEW, stop_on_eos=on_eos, use_graph=use_graph, stop=stops)
                assert got == toks and eng.last_finish == [fin], (stops, use_graph, on_eos)
    toks, fin, _ = _expect(eng, first, eos, [ABSENT], False)
    assert toks == first and fin == ("length", None)
    reqs = [(ids, frame), (gm["b_ids"].tolist(), torch.from_numpy(gm["b_image"]).to(device))]
    firsts = eng.generate_batch(reqs, max_new_tokens=N_NEW, stop_on_eos=False)
    s0, s1 = _spread_stops(eng, firsts, eos, [range(2, 16), range(20, 40)])
    for stops in ([s0, s1], [ABSENT]):
        exp = [_expect(eng, f, eos, stops, False) for f in firsts]
        for use_graph in (False, True):
            got = eng.generate_batch(reqs, max_new_tokens=N_NEW, stop_on_eos=False, use_graph=use_graph, stop=stops)
            assert got == [e[0] for e in exp] and eng.last_finish == [e[1] for e in exp], (stops, use_graph)
    exp = [_expect(eng, f, eos, [s0, s1], False) for f in firsts]
    assert len({e[2]["n_tokens"] for e in exp}) == 2 and all(e[1][0] == "stop" for e in exp)
    assert eng.generate_batch(reqs, max_new_tokens=N_NEW, stop_on_eos=False) == firsts


# ----------------------------------------------------------------------------- client
@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_stop_and_finish_reason(device, tmp_path, monkeypatch, model):
    from PIL import Image
    from vision_inspection_system_amd.client import LocalVLMClient
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    monkeypatch.setenv("VIS_IGNORE_EOS", "1")               # random weights may pick EOS at once: replies of full length
    p = tmp_path / "img.png"
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    url = encode_image_optimized(str(p), 256)
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": [{"type": "text", "text": "Inspect."},
                                         {"type": "image_url", "image_url": {"url": url}}]}]

    def create(**kw):
        return c.chat.completions.create(model=model, messages=msgs, max_tokens=32, logprobs=True, **kw)

    def tokens_of(r):
        return [bytes(e.bytes) for e in r.choices[0].logprobs.content]

    cut4 = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=4)
    assert cut4.choices[0].finish_reason == "length" and cut4.usage["completion_tokens"] == 4
    for kw in (dict(temperature=0.0), dict(temperature=0.0, response_format={"type": "json_object"}),
               dict(temperature=0.9, top_p=0.8, seed=5), dict(temperature=0.0, repetition_penalty=1.3, frequency_penalty=0.5)):
        base = create(**kw)
        assert base.choices[0].finish_reason == "length"
        tb = tokens_of(base)
        data = b"".join(tb)
        print(kw, "reply bytes:", data)
        assert len(tb) == 32 and len(data) >= 2, (kw, data)
        s = data[len(data) // 2:len(data) // 2 + 2]
        want = stop.find_oracle([s], tb)
        assert want["reason"] == STOP
        r = create(stop=[s], **kw)
        ch = r.choices[0]
        assert ch.finish_reason == "stop", kw
        assert tokens_of(r) == tb[:want["n_tokens"]], kw                         # the same reply up to the cut
        assert r.usage["completion_tokens"] == want["n_tokens"] == len(ch.logprobs.content)
        assert ch.message.content == data[:want["cut"]].decode("utf-8", errors="replace")
        assert s not in data[:want["cut"]]
        # a string that is not in the reply changes nothing but the poll
        r = create(stop=["\x00never\x00"], **kw)
        assert tokens_of(r) == tb and r.choices[0].finish_reason == "length"
        assert r.choices[0].message.content == base.choices[0].message.content
    many = c.complete_many(model, [msgs, msgs], temperature=0.0, max_tokens=32, stop="\x00never\x00")
    assert [m.choices[0].finish_reason for m in many] == ["length", "length"]
    for bad in ([], ["a"] * 5, [""], [3]):
        with pytest.raises(ValueError):
            c.chat.completions.create(model="no-such-model", messages=msgs, stop=bad)
