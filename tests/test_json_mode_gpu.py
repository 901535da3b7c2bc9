"""JSON mode on MI355X: vis_json_mask against the Python grammar (json_grammar) bit for bit, the masked picks against the
unmasked ones, and the engines' / client's JSON-mode replies replayed through the grammar token by token."""
import json
import os
import random

import numpy as np
import pytest
import torch

from helpers import load_golden
from vision_inspection_system_amd import hip
from vision_inspection_system_amd import json_grammar as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HF = os.path.join(HERE, "golden", "hf_dirs")

# byte prefixes that reach the grammar's states (value start, after a key, in a string, inside a UTF-8 sequence, numbers,
# literals, \u escapes, DONE, and an error: ']' where a key must come)
PREFIXES = [b"", b' {"a": ', b'{"key"', b'{"k": "abc', b'{"k": "\xe6\x97', b'{"k": [1, -0.5e', b'{"k": [tr',
            b'{"k": {"x": 1}}', b'{"k": "\\u1', b'{"k": 12', b'{"a":[{"b":null}, ', b"{]"]


class _Vocab:
    """token_bytes of a synthetic vocabulary: ids 0..255 the single bytes, then random JSON-heavy byte strings of 1..40
    bytes (structure, digits, literals, escapes, whole and partial UTF-8 characters), a few specials without bytes."""

    def __init__(self, V: int, seed: int):
        rng = random.Random(seed)
        pieces = [b"{", b"}", b"[", b"]", b'"', b":", b",", b" ", b"\n", b"  ", b"\\", b"\\n", b"\\u00e9", b"0", b"1", b"9",
                  b"-", b".", b"e", b"E+", b"true", b"false", b"null", b"abc", b"key", b"_x", "é".encode(), "日本".encode(),
                  "😀".encode(), b"\xe6", b"\x97", b"\xa5", b"\xf0\x9f", b"\x98\x80", b"\x01", b"\xff", b"\t", b"/"]
        self.toks = [bytes([b]) for b in range(256)]
        while len(self.toks) < V:
            t = b"".join(rng.choice(pieces) for _ in range(rng.randint(1, 12)))[:rng.randint(1, 40)]
            self.toks.append(t)
        for t in range(300, V, 997):
            self.toks[t] = b""

    def token_bytes(self, t: int) -> bytes:
        return self.toks[t]


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


@pytest.fixture(scope="module")
def big(device):
    V = 152064
    tok = _Vocab(V, seed=11)
    table = G.build_token_table(tok, V, [V - 3, V - 1])
    return table, _dev_table(table)


def _dev_table(table):
    d = "cuda:0"
    return (torch.from_numpy(table.off).to(d), torch.from_numpy(table.data).to(d), torch.from_numpy(table.flags).to(d),
            torch.from_numpy(table.eos_ids).to(d))


def _prefix_state(p: bytes, table):
    st = G.initial_state()
    for b in p:
        G.advance(st, b, table)
    return st


def _run_mask(prefixes, table, dt, T: int = 64):
    """One launch for len(prefixes) rows; row r folds the single-byte tokens of prefixes[r] (anchored at position 0)."""
    B = len(prefixes)
    V = table.vocab
    tokens = torch.zeros((B, T), dtype=torch.int32)
    state = torch.zeros((B, G.STATE_INTS), dtype=torch.int32)
    step = torch.zeros(B, dtype=torch.int32)
    for r, p in enumerate(prefixes):
        tokens[r, :len(p)] = torch.tensor(list(p), dtype=torch.int32)
        step[r] = len(p)
        rd = (len(p) & 1) * G.SLOT_INTS
        state[r, rd + G.ANCHOR] = 1
        state[r, rd + G.POS] = 0
    tokens, state, step = tokens.cuda(), state.cuda(), step.cuda()
    allow = torch.full((B, (V + 63) // 64 + 3), -1, dtype=torch.int64, device="cuda")
    hip.json_mask(state, tokens, step, *dt, allow)
    torch.cuda.synchronize()
    return state.cpu(), allow.cpu()


def _check_rows(prefixes, table, state, allow, cache):
    nw = (table.vocab + 63) // 64
    for r, p in enumerate(prefixes):
        if p not in cache:
            st = _prefix_state(p, table)
            ok, err = G.allowed(st, table)
            if err:
                st[G.ERR] = 1
            cache[p] = (st, G.mask_words(ok))
        st, words = cache[p]
        wr = ((len(p) + 1) & 1) * G.SLOT_INTS
        got = state[r, wr:wr + G.SLOT_INTS].tolist()
        assert got[:G.LEX_WORDS] == st[:G.LEX_WORDS], (p, got, st)
        assert got[G.POS] == len(p) and got[G.ANCHOR] == 1
        assert state[r, G.COUNT_WORD] == 0 and state[r, G.TICKET_WORD] == 0
        assert np.array_equal(allow[r, :nw].numpy(), words), p
        assert (allow[r, nw:] == -1).all(), "wrote past the row's words"


def test_mask_equals_reference_synthetic_vocab(big):
    table, dt = big
    cache = {}
    for p in PREFIXES:                      # B = 1
        state, allow = _run_mask([p], table, dt)
        _check_rows([p], table, state, allow, cache)
    rows = [PREFIXES[r % len(PREFIXES)] for r in range(64)]
    state, allow = _run_mask(rows, table, dt)   # B = 64, every state in several slots
    _check_rows(rows, table, state, allow, cache)
    # the in-string state allows most of the vocabulary, the error row only the EOS ids
    assert sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in cache[b'{"k": "abc'][1]) > 30000
    assert G.mask_words(np.isin(np.arange(table.vocab), table.eos_ids)).tolist() == cache[b"{]"][1].tolist()
    assert cache[b"{]"][0][G.ERR] == 1


@pytest.mark.parametrize("name,V", [("qwen2vl_tiny", 520), ("mllama_tiny", 513)])
def test_mask_and_fold_follow_the_reference_step_by_step(name, V):
    """Random logits, the masked Gumbel-max pick, the next launch folds it: state and mask equal the reference each step."""
    pytest.importorskip("tokenizers")
    from vision_inspection_system_amd.tokenizer import HFTokenizer, LlamaHFTokenizer
    tok = HFTokenizer(os.path.join(HF, name), 500, 501, 502, [503, 505]) if name == "qwen2vl_tiny" else \
        LlamaHFTokenizer(os.path.join(HF, name), 510, [501])
    eos = [503, 505] if name == "qwen2vl_tiny" else list(tok.eos_ids)
    table = G.build_token_table(tok, V, eos)
    dt = _dev_table(table)
    B, T, P0 = 4, 128, 3
    state = torch.zeros((B, G.STATE_INTS), dtype=torch.int32, device="cuda")
    tokens = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    step = torch.full((B,), P0, dtype=torch.int32, device="cuda")
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    allow = torch.zeros((B, (V + 63) // 64), dtype=torch.int64, device="cuda")
    wv = torch.empty(256 * B, dtype=torch.float32, device="cuda")
    wi = torch.empty(256 * B, dtype=torch.int32, device="cuda")
    ref = [G.initial_state() for _ in range(B)]
    g = torch.Generator(device="cuda").manual_seed(3)
    for it in range(60):
        hip.json_mask(state, tokens, step, *dt, allow)
        st = state.cpu()
        al = allow.cpu().numpy()
        n = P0 + it
        for b in range(B):
            ok, err = G.allowed(ref[b], table)
            if err:
                ref[b][G.ERR] = 1
            wr = ((n + 1) & 1) * G.SLOT_INTS
            assert st[b, wr:wr + G.LEX_WORDS].tolist() == ref[b][:G.LEX_WORDS], (it, b)
            assert np.array_equal(al[b], G.mask_words(ok)), (it, b)
        logits = torch.randn((B, V), generator=g, device="cuda") * 3
        hip.argmax_masked(logits, wv, wi, tokens, cur, step, allow, temperature=0.9, seed=it)
        picked = tokens[:, n].cpu().tolist()
        for b in range(B):
            ok, _ = G.allowed(ref[b], table)
            assert ok[picked[b]], (it, b, picked[b])
            G.advance(ref[b], picked[b], table)
            assert not ref[b][G.ERR]


def _masks(V: int, B: int, kind: str, seed: int) -> torch.Tensor:
    nw = (V + 63) // 64
    if kind == "ones":
        m = torch.full((B, nw), -1, dtype=torch.int64)
        if V % 64:
            m[:, -1] = (1 << (V % 64)) - 1
        return m.cuda()
    rng = np.random.default_rng(seed)
    bits = rng.random((B, nw * 64)) < 0.1
    bits[:, V:] = False
    return torch.from_numpy(np.packbits(bits.reshape(B, -1, 8), axis=2, bitorder="little").reshape(B, -1)
                            .view("<u8").view(np.int64).copy()).cuda()


def _allowed_bits(m: torch.Tensor, V: int) -> np.ndarray:
    a = m.cpu().numpy().view(np.uint8)
    return np.unpackbits(a.reshape(a.shape[0], -1), axis=1, bitorder="little")[:, :V].astype(bool)


def _pick(fn, x, B, T=8, **kw):
    tokens = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    step = torch.arange(B, dtype=torch.int32, device="cuda") % 5
    cur = torch.zeros(B, dtype=torch.int32, device="cuda")
    wv = torch.empty(max(256 * B, 2048), dtype=torch.float32, device="cuda")
    wi = torch.empty(max(256 * B, 2048), dtype=torch.int32, device="cuda")
    fn(x, wv, wi, tokens if B > 1 else tokens[0], cur, step, **kw)
    return tokens.cpu(), cur.cpu(), step.cpu()


@pytest.mark.parametrize("V", [152064, 128256, 513])
def test_masked_argmax(V):
    g = torch.Generator(device="cuda").manual_seed(V)
    for B in (1, 64):
        x = (torch.randn((B, V), generator=g, device="cuda") * 4).contiguous()
        x[:, 7] = x.max() + 1                   # ties at the top: the lower index wins in both forms
        x[:, 9] = x[:, 7]
        xs = x if B > 1 else x[0]
        for temp in (0.0, 0.7):
            a = _pick(hip.argmax, xs, B, temperature=temp, seed=5)
            ones = _masks(V, B, "ones", 0)
            b = _pick(lambda *args, **kw: hip.argmax_masked(*args[:6], ones if B > 1 else ones[0], **kw), xs, B,
                      temperature=temp, seed=5)
            for u, v in zip(a, b):
                assert torch.equal(u, v), (V, B, temp)
            m = _masks(V, B, "sparse", B)
            allowed = _allowed_bits(m, V)
            t, cur, _ = _pick(lambda *args, **kw: hip.argmax_masked(*args[:6], m if B > 1 else m[0], **kw), xs, B,
                              temperature=temp, seed=5)
            for r in range(B):
                assert allowed[r, int(cur[r])], (V, B, temp, r)
                if temp == 0.0:
                    xr = x[r].cpu().numpy().copy()
                    xr[~allowed[r]] = -np.inf
                    assert int(cur[r]) == int(np.argmax(xr))
            one = torch.zeros_like(m)
            ids = [(r * 7919 + 3) % V for r in range(B)]
            for r, i in enumerate(ids):
                one[r, i // 64] = torch.tensor(np.array([1 << (i % 64)], dtype=np.uint64).view(np.int64)[0])
            _, cur, _ = _pick(lambda *args, **kw: hip.argmax_masked(*args[:6], one if B > 1 else one[0], **kw), xs, B,
                              temperature=temp, seed=5)
            assert cur.tolist() == ids


@pytest.mark.parametrize("N,K", [(152064, 3584), (128256, 4096), (513, 64)])
def test_masked_gemv_argmax(N, K):
    """The fused lm_head + masked pick (7B / 11B lm_head shapes): all-ones equals the unmasked fused pick bit for bit; a
    grammar mask gives the pick of gemv + the masked two-stage argmax."""
    g = torch.Generator(device="cuda").manual_seed(N)
    w = (torch.randn((N, K), generator=g, device="cuda") * 0.05).to(torch.bfloat16)
    x = torch.randn(K, generator=g, device="cuda").to(torch.bfloat16)
    nw_ = torch.rand(K, generator=g, device="cuda").to(torch.bfloat16) + 0.5

    def fused(masked, allow, temp):
        logits = torch.empty(N, dtype=torch.float32, device="cuda")
        tokens = torch.full((16,), -1, dtype=torch.int32, device="cuda")
        cur = torch.zeros(1, dtype=torch.int32, device="cuda")
        step = torch.full((1,), 3, dtype=torch.int32, device="cuda")
        wv = torch.empty(2048, dtype=torch.float32, device="cuda")
        wi = torch.empty(2048, dtype=torch.int32, device="cuda")
        if masked:
            hip.gemv_argmax_masked(x, w, logits, wv, wi, tokens, cur, step, allow, norm_w=nw_, temperature=temp, seed=9)
        else:
            hip.gemv_argmax(x, w, logits, wv, wi, tokens, cur, step, norm_w=nw_, temperature=temp, seed=9)
        return logits, tokens.cpu(), cur.cpu(), step.cpu()

    for temp in (0.0, 0.8):
        ref = fused(False, None, temp)
        got = fused(True, _masks(N, 1, "ones", 0)[0], temp)
        assert torch.equal(ref[0].view(torch.int32), got[0].view(torch.int32))
        for u, v in zip(ref[1:], got[1:]):
            assert torch.equal(u, v)
        m = _masks(N, 1, "sparse", 1)
        lg, _, cur, _ = fused(True, m[0], temp)
        tokens = torch.full((16,), -1, dtype=torch.int32, device="cuda")
        c2 = torch.zeros(1, dtype=torch.int32, device="cuda")
        s2 = torch.full((1,), 3, dtype=torch.int32, device="cuda")
        hip.argmax_masked(lg, torch.empty(256, device="cuda"), torch.empty(256, dtype=torch.int32, device="cuda"), tokens,
                          c2, s2, m[0], temperature=temp, seed=9)
        assert int(c2) == int(cur) and _allowed_bits(m, N)[0, int(cur)]


# ----------------------------------------------------------------------------- engines
def _replay(table, toks, eos_ids, what=""):
    """Every token allowed by the reference grammar at its position; the bytes a JSON-object prefix; parsed when DONE."""
    st = G.initial_state()
    for i, t in enumerate(toks):
        ok, err = G.allowed(st, table)
        assert not err and ok[t], (what, i, t, toks)
        G.advance(st, t, table)
        if t in eos_ids:
            assert i == len(toks) - 1, (what, "tokens after EOS")
    data = b"".join(table.tokens[t] for t in toks)
    assert G.feed(data)[0] in ("progress", "done"), (what, data)
    assert data[:1] in (b"", b"{", b" ", b"\t", b"\n", b"\r")
    if st[G.LEX] == G.DONE:
        assert isinstance(json.loads(data.decode("utf-8")), dict), (what, data)
    return st[G.LEX] == G.DONE


def _qwen_engine(device, **kw):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    eng = Qwen2VLEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, **kw)
    eng.tokenizer = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    return cfg, eng


def test_qwen_single_sequence_paths(device, monkeypatch):
    cfg, eng = _qwen_engine(device, decode_splits=4)
    g = load_golden()
    ids = g["ids_a"].tolist()
    fr = [torch.from_numpy(g["frame_a"]).to(device)]
    off = eng.generate(ids, fr, max_new_tokens=40, ignore_eos=True)
    assert eng.generate(ids, fr, max_new_tokens=40, ignore_eos=True, json_mode=False) == off
    assert eng.chain_sync is not None
    outs = {}
    for temp, seed in ((0.0, 0), (0.9, 1), (1.5, 2)):
        for use_graph in (False, True):
            toks = eng.generate(ids, fr, max_new_tokens=60, temperature=temp, seed=seed, use_graph=use_graph, json_mode=True)
            assert eng._json is not None and eng.json_on is False
            outs[(temp, use_graph)] = toks
            _replay(eng._json.table, toks, set(cfg.eos_ids), (temp, use_graph))
        assert outs[(temp, False)] == outs[(temp, True)], temp
    assert outs[(0.0, True)] != off[:len(outs[(0.0, True)])]       # random weights do not write JSON on their own
    # unchained layer head and the fp8 single-sequence step
    monkeypatch.setenv("VIS_DECODE_CHAIN", "0")
    _, plain = _qwen_engine(device, decode_splits=4)
    assert plain.chain_sync is None
    for temp, seed in ((0.0, 0), (0.9, 1)):
        assert plain.generate(ids, fr, max_new_tokens=60, temperature=temp, seed=seed, json_mode=True) == outs[(temp, True)]
    _, f8 = _qwen_engine(device, decode_splits=4, decode_weights="fp8")
    for temp in (0.0, 0.9):
        toks = f8.generate(ids, fr, max_new_tokens=60, temperature=temp, seed=1, json_mode=True)
        _replay(f8._json.table, toks, set(cfg.eos_ids), ("fp8", temp))
    # after a JSON-mode request the engine is back to the unmasked kernels
    assert eng.generate(ids, fr, max_new_tokens=40, ignore_eos=True) == off


@pytest.mark.parametrize("form,weights", [("plain", "bf16"), ("plain", "fp8"), ("fused", "bf16"), ("rows", "bf16")])
def test_qwen_batched_forms(device, monkeypatch, form, weights):
    monkeypatch.setenv("VIS_DECODE_FUSED", "1" if form == "fused" else "0")
    monkeypatch.setenv("VIS_ROWS_GEMV", "2" if form == "rows" else "0")
    cfg, eng = _qwen_engine(device, max_batch=17, decode_weights=weights)
    g = load_golden()
    fa = [torch.from_numpy(g["frame_a"]).to(device)]
    reqs = [(g["ids_a"].tolist(), fa), ([256, 72, 105, 33, 90, 41], [])]
    n_big = 2 if form == "rows" else 17
    big = [reqs[0]] * n_big
    eos = set(cfg.eos_ids)
    for temp in (0.0, 0.9):
        res = {}
        for use_graph in (False, True):
            out = eng.generate_batch(reqs, max_new_tokens=50, temperature=temp, seed=4, use_graph=use_graph, json_mode=True)
            for i, t in enumerate(out):
                _replay(eng._json.table, t, eos, (form, temp, i))
            res[use_graph] = out
        assert res[False] == res[True]
        outs = eng.generate_batch(big, max_new_tokens=50, temperature=temp, seed=4, json_mode=True)
        for i, t in enumerate(outs):
            _replay(eng._json.table, t, eos, (form, temp, "big", i))
        if temp == 0.0:     # the same request in every slot: the same tokens in every slot (greedy)
            assert all(t == outs[0] for t in outs)
        single = eng.generate(*reqs[0], max_new_tokens=50, temperature=temp, seed=4, json_mode=True)
        assert single[:1] == outs[0][:1] == res[True][0][:1]        # the prompt pass's pick: the same arithmetic
        if form == "rows":                                           # the rows GEMV is the single-sequence arithmetic
            assert res[True][0] == single and outs[0] == single


def test_qwen_json_failure_is_reported(device):
    """A vocabulary that cannot continue the object (no '"', no '}'): the request fails instead of returning non-JSON."""
    from vision_inspection_system_amd.json_mode import JsonModeError
    cfg, eng = _qwen_engine(device, max_batch=2)

    class NoQuote:
        def token_bytes(self, t):
            return b"" if t in (ord('"'), ord("}")) or t > 255 else bytes([t])

    eng.tokenizer = NoQuote()
    g = load_golden()
    req = (g["ids_a"].tolist(), [torch.from_numpy(g["frame_a"]).to(device)])
    # at most 16 whitespace bytes, '{', 16 more: the 34th pick at the latest finds nothing allowed
    with pytest.raises(JsonModeError):
        eng.generate(*req, max_new_tokens=60, json_mode=True)
    out = eng.generate_batch([req, req], max_new_tokens=60, json_mode=True)
    assert all(isinstance(o, JsonModeError) for o in out)


def test_mllama_json_mode(device):
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    from vision_inspection_system_amd.mllama_weights import MllamaConfig, pack_device_weights, synth_state_dict
    from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
    cfg = MllamaConfig.tiny()
    eng = MllamaEngine(cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device), device, max_ctx=256, max_batch=17)
    eng.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
    gm = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
    frame = torch.from_numpy(gm["a_image"]).to(device)
    ids = gm["a_ids"].tolist()
    eos = set(cfg.eos_ids)
    off = eng.generate(ids, frame, max_new_tokens=30, stop_on_eos=False)
    assert eng.generate(ids, frame, max_new_tokens=30, stop_on_eos=False, json_mode=False) == off
    for temp in (0.0, 0.9):
        a = eng.generate(ids, frame, max_new_tokens=50, temperature=temp, seed=3, use_graph=False, json_mode=True)
        b = eng.generate(ids, frame, max_new_tokens=50, temperature=temp, seed=3, json_mode=True)
        assert a == b
        _replay(eng._json.table, b, eos, ("mllama", temp))
        reqs = [(ids, frame), (gm["b_ids"].tolist(), torch.from_numpy(gm["b_image"]).to(device))] * 8 + [(ids, frame)]
        outs = eng.generate_batch(reqs, max_new_tokens=40, temperature=temp, seed=3, json_mode=True)
        assert len(outs) == 17
        for i, t in enumerate(outs):
            _replay(eng._json.table, t, eos, ("mllama batch", temp, i))
        assert outs[0][:1] == b[:1]
    assert eng.generate(ids, frame, max_new_tokens=30, stop_on_eos=False) == off


# ----------------------------------------------------------------------------- client
@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_response_format(device, tmp_path, model):
    from PIL import Image
    from vision_inspection_system_amd.client import LocalVLMClient, get_model
    from vision_inspection_system_amd.image_processing import encode_image_optimized
    p = tmp_path / "img.png"
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (120, 90, 3), dtype=np.uint8)).save(p)
    url = encode_image_optimized(str(p), 256)
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": [{"type": "text", "text": "Inspect."},
                                         {"type": "image_url", "image_url": {"url": url}}]}]
    plain = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=24)
    text = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=24,
                                     response_format={"type": "text"})
    assert text.choices[0].message.content == plain.choices[0].message.content
    assert text.usage == plain.usage
    r = c.chat.completions.create(model=model, messages=msgs, temperature=0.0, max_tokens=24,
                                  response_format={"type": "json_object"}, logprobs=True)
    body = r.choices[0].message.content
    assert body != plain.choices[0].message.content
    assert get_model(model).engine._json.table.vocab == get_model(model).cfg.vocab
    # the generated tokens' bytes (logprobs.content) are a JSON-object prefix; logprobs keep their raw-logit meaning
    data = bytes(b for e in r.choices[0].logprobs.content for b in e.bytes)
    assert G.feed(data)[0] in ("progress", "done"), data
    assert len(r.choices[0].logprobs.content) == r.usage["completion_tokens"]
    many = c.complete_many(model, [msgs, msgs], temperature=0.0, max_tokens=24, response_format={"type": "json_object"},
                           logprobs=True)
    for m in many:
        d = bytes(b for e in m.choices[0].logprobs.content for b in e.bytes)
        assert G.feed(d)[0] in ("progress", "done"), d
