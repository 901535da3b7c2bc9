"""Token log-probabilities, the parts that need no GPU: the vis_logprobs_f32 argument checks (before any HIP call), the
tokenizers' per-token bytes, and the client's argument validation (before any model is loaded)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HF = os.path.join(ROOT, "tests", "golden", "hf_dirs")
RETRY_SUBSTRINGS = ("429", "rate", "413", "payload")
TEXT = "Hello, wörld! 日本語 ✓ — café\n{\"overall_condition\": \"damaged\", \"overall_confidence\": 0.93} 😀  end"


@pytest.fixture(scope="module")
def lib():
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    from vision_inspection_system_amd import hip
    return hip.load()


def test_logprobs_entry_point_rejects_bad_arguments_without_gpu(lib):
    from vision_inspection_system_amd import hip
    assert "vis_logprobs_f32" in hip.exported_symbols() and "vis_logprobs_ws_bytes" in hip.exported_symbols()
    V, T, B = 152064, 64, 4
    ws = int(lib.vis_logprobs_ws_bytes(V, B))
    assert ws == B * 38 * 64 * 4
    p = 4096     # any non-null address: nothing is launched when an argument is refused

    def call(logits=p, V=V, ld=V, tokens=p, T=T, step=p, k=5, lp=p, ids=p, wsp=p, wsb=ws, batch=B):
        return lib.vis_logprobs_f32(logits, V, ld, tokens, T, step, k, lp, ids, wsp, wsb, batch, None)

    for bad in (dict(k=-1), dict(k=21), dict(V=0), dict(V=-5), dict(batch=0), dict(batch=65), dict(ld=V - 1),
                dict(logits=None), dict(tokens=None), dict(step=None), dict(lp=None), dict(ids=None), dict(wsp=None),
                dict(wsb=ws - 4), dict(T=0), dict(V=262145, ld=262145), dict(V=8, ld=8, k=9)):
        assert call(**bad) == 1, bad
    assert lib.vis_logprobs_ws_bytes(0, 1) == 0 and lib.vis_logprobs_ws_bytes(512, 65) == 0
    assert lib.vis_logprobs_ws_bytes(512, 1) == 256 and lib.vis_logprobs_ws_bytes(513, 1) == 256


def _check_tokenizer(tok, special_ids):
    ids = tok.encode(TEXT)
    joined = b"".join(tok.token_bytes(i) for i in ids)
    assert joined.decode("utf-8") == tok.decode(ids) == TEXT
    # the per-token text is those bytes with errors="replace": multi-byte characters split over tokens give U+FFFD
    for i in ids:
        assert tok.token_text(i) == tok.token_bytes(i).decode("utf-8", errors="replace")
    for s in special_ids:
        assert tok.token_bytes(s) == b""
        assert tok.token_text(s).startswith("<|") and tok.token_text(s).endswith("|>")
    # specials inside the generated ids do not change the invariant (decode skips them, their bytes are empty)
    mixed = ids[:5] + [special_ids[0]] + ids[5:]
    assert b"".join(tok.token_bytes(i) for i in mixed).decode("utf-8") == tok.decode(mixed)


def test_token_bytes_byte_level_bpe_qwen():
    pytest.importorskip("tokenizers")
    from vision_inspection_system_amd.tokenizer import HFTokenizer
    tok = HFTokenizer(os.path.join(HF, "qwen2vl_tiny"), 500, 501, 502, [503, 505])
    _check_tokenizer(tok, [503, 504, 500])


def test_token_bytes_byte_level_bpe_llama():
    pytest.importorskip("tokenizers")
    from vision_inspection_system_amd.tokenizer import LlamaHFTokenizer
    tok = LlamaHFTokenizer(os.path.join(HF, "mllama_tiny"), 510, [501])
    _check_tokenizer(tok, [tok.eot_id, tok.start_header_id, tok.bos_id])


def test_token_bytes_byte_tokenizers():
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.mllama_weights import MllamaConfig
    from vision_inspection_system_amd.tokenizer import ByteTokenizer, LlamaByteTokenizer
    cfg = Qwen2VLConfig.tiny()
    bt = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    _check_tokenizer(bt, [bt.im_end_id, bt.im_start_id, bt.image_token_id])
    assert bt.token_bytes(65) == b"A" and bt.token_bytes(300) == b""
    mc = MllamaConfig.tiny()
    lt = LlamaByteTokenizer(mc.vocab, mc.image_token_id, mc.eos_ids)
    _check_tokenizer(lt, [lt.eot_id, lt.bos_id, lt.image_token_id])


@pytest.mark.parametrize("kw", [dict(top_logprobs=3), dict(logprobs=False, top_logprobs=0),
                                dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1),
                                dict(logprobs=True, top_logprobs=2.0), dict(logprobs=True, top_logprobs="5"),
                                dict(logprobs=True, top_logprobs=True)])
def test_client_rejects_bad_logprobs_arguments_before_loading(kw, monkeypatch):
    from vision_inspection_system_amd import client as C

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(C, "get_model", no_load)
    c = C.LocalVLMClient()
    with pytest.raises(ValueError) as e:
        c.chat.completions.create(model="synthetic:tiny", messages=[{"role": "user", "content": "hi"}], max_tokens=4, **kw)
    msg = str(e.value).lower()
    assert not any(s in msg for s in RETRY_SUBSTRINGS), msg


def test_client_logprobs_argument_mapping():
    from vision_inspection_system_amd.client import CannedResponseClient, _Choice, _Message, logprobs_k
    assert logprobs_k(False, None) is None and logprobs_k(None, None) is None
    assert logprobs_k(True, None) == 0 and logprobs_k(True, 20) == 20 and logprobs_k(True, 0) == 0
    assert _Choice(_Message("x")).logprobs is None
    # the canned client keeps ignoring every extra argument
    r = CannedResponseClient("OK").chat.completions.create(model="m", messages=[], logprobs=True, top_logprobs=99)
    assert r.choices[0].message.content == "OK" and r.choices[0].logprobs is None


def test_engine_logprobs_argument_check():
    from vision_inspection_system_amd.logprobs import check_k
    assert check_k(None) is None and check_k(0) == 0 and check_k(20) == 20
    for bad in (-1, 21, 1.0, True, "3"):
        with pytest.raises(ValueError):
            check_k(bad)
