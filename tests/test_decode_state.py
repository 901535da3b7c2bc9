"""DecodeStage._init_decode_state on the CPU: which attributes exist in which configuration, the shapes that follow from the
arguments, the one rule of ``b_part``; and quantize_decode_weights' zero-padded down projection.  No GPU: a bare subclass
instance with the tiny configuration on device "cpu", the chain switched off (its context limit asks the device)."""
import types

import pytest
import torch

from vision_inspection_system_amd import decode_stage, hip
from vision_inspection_system_amd.config import Qwen2VLConfig
from vision_inspection_system_amd.decode_stage import DecodeStage, quantize_decode_weights

CFG = Qwen2VLConfig.tiny()      # hidden 256, 2 q heads / 1 kv head of 128, intermediate 704 (kpad 768), vocab 512
H, I, NQ, HQD, T = CFG.hidden, CFG.intermediate, (CFG.heads + 2 * CFG.kv_heads) * CFG.head_dim, CFG.heads * CFG.head_dim, 256
ROWS = ("b_x", "b_x2", "b_qkv", "b_attn", "b_act", "b_xn", "b_xn2")
FP8 = ("b_xq", "b_x2q", "b_actq", "b_sx")
FP8_FUSED = ("b_xqs", "b_x2qs", "b_actqs")
FUSED = ("b_xw", "b_x2w", "b_ssq1", "b_ssq2", "b_proj_ws")


class Bare(DecodeStage):
    pass


def make(monkeypatch, max_batch, n_self=2, fused_env=False, **kw):
    monkeypatch.setenv("VIS_DECODE_CHAIN", "0")
    monkeypatch.setenv("VIS_DECODE_FUSED", "1" if fused_env else "0")
    monkeypatch.delenv("VIS_QKV_FOLD", raising=False)
    st = Bare.__new__(Bare)
    st.cfg, st.device, st.max_ctx = CFG, torch.device("cpu"), T
    st._init_decode_state(max_batch, n_self, **kw)
    return st


def has(st, names):
    return [n for n in names if hasattr(st, n)]


def part_numel(bm):
    return 16 * hip.part_rows(bm) * max(NQ, H, 2 * I)


def test_bf16_single_sequence(monkeypatch):
    st = make(monkeypatch, 1)
    assert st.max_batch == 1 and st.decode_weights == "bf16" and st.mxfp4_gemm_from is None
    assert st.nsplit == max(1, -(-T // hip.DECODE_KEYS_PER_SPLIT))
    assert st.kcache_b.shape == st.vcache_b.shape == (1, 2, CFG.kv_heads, T, CFG.head_dim)
    assert st.kcache.shape == (2, CFG.kv_heads, T, CFG.head_dim)
    for view, base in ((st.kcache, st.kcache_b), (st.vcache, st.vcache_b), (st.step, st.step_b), (st.cur_token, st.cur_b),
                       (st.tokens, st.tokens_b), (st.logits, st.logits_b)):
        assert view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() and view.storage_offset() == 0
    assert st.step.shape == st.cur_token.shape == (1,) and st.tokens.shape == (T,) and st.logits.shape == (CFG.vocab,)
    assert st.ws_val.numel() == st.ws_idx.numel() == 2048
    assert (st.d_x.shape, st.d_x2.shape, st.d_qkv.shape, st.d_attn.shape, st.d_act.shape) == \
        ((1, H), (1, H), (NQ,), (HQD,), (I,))
    assert st.part_o.numel() == CFG.heads * st.nsplit * CFG.head_dim and st.part_ml.numel() == CFG.heads * st.nsplit * 2
    assert has(st, ROWS + FP8 + FP8_FUSED + FUSED) == []
    assert not st.streamk_part and not hasattr(st, "b_part") and st.kpad is None and st.chain_ws is None and st.chain_sync is None
    assert (st.fused_proj, st.fold_qkv, st.fp8_batched, st.chain_ctx_limit, st._chain_launches) == (False, True, False, 0, 0)
    assert (st.slot_prompt_len, st.prompt_len, st._decoded, st.decode_limit, st.temperature, st.seed, st.last_timing,
            st._prefill_streams) == ([0], 0, 0, 0, 0.0, 0, {}, [])
    for t in (st.kcache_b, st.vcache_b, st.step_b, st.cur_b, st.tokens_b):
        assert not t.any()


def test_bf16_batched(monkeypatch):
    st = make(monkeypatch, 3, n_self=3, decode_splits=5)
    assert st.nsplit == 5 and st.kcache_b.shape[:2] == (3, 3) and st.slot_prompt_len == [0, 0, 0]
    assert st.ws_val.numel() == 2048 and st.logits_b.shape == (3, CFG.vocab)
    assert has(st, ROWS) == list(ROWS) and has(st, FP8 + FP8_FUSED + FUSED) == []
    assert [tuple(getattr(st, n).shape) for n in ROWS] == [(3, H), (3, H), (3, NQ), (3, HQD), (3, I), (3, H), (3, H)]
    assert all(getattr(st, n).dtype == torch.bfloat16 for n in ROWS)
    assert st.part_o.numel() == 3 * CFG.heads * 5 * CFG.head_dim and st.part_ml.numel() == 3 * CFG.heads * 5 * 2
    assert st.streamk_part and st.b_part.numel() == part_numel(3) and st.b_part.dtype == torch.float32
    assert st.kpad is None and not st.fp8_batched and not st.fused_proj


def test_pick_workspace_grows_with_the_batch(monkeypatch):
    assert make(monkeypatch, 9).ws_val.numel() == 256 * 9


def test_qkv_fold_switch(monkeypatch):
    monkeypatch.setenv("VIS_DECODE_CHAIN", "0")
    monkeypatch.setenv("VIS_QKV_FOLD", "0")
    st = Bare.__new__(Bare)
    st.cfg, st.device, st.max_ctx = CFG, torch.device("cpu"), T
    st._init_decode_state(1, 2)
    assert st.fold_qkv is False


def test_fp8_batched(monkeypatch):
    st = make(monkeypatch, 3, decode_weights="fp8")
    assert st.fp8_batched and not st.fused_proj and st.kpad == 768
    assert has(st, ROWS + FP8) == list(ROWS + FP8) and has(st, FP8_FUSED + FUSED) == []
    assert [tuple(getattr(st, n).shape) for n in FP8] == [(3, H), (3, H), (3, 768), (3, 3)]
    assert all(getattr(st, n).dtype == torch.uint8 for n in FP8[:3]) and st.b_sx.dtype == torch.float32
    assert not any(getattr(st, n).any() for n in FP8)
    assert st.b_part.numel() == part_numel(3)      # the stream-K step reads it


def test_fp8_single_sequence_has_no_batched_state(monkeypatch):
    st = make(monkeypatch, 1, decode_weights="fp8")
    assert not st.fp8_batched and st.kpad is None and not st.streamk_part and has(st, ROWS + FP8 + ("b_part",)) == []
    assert make(monkeypatch, 1, decode_weights="fp8", prefill_fp8=True).kpad == 768


@pytest.fixture
def ws_bytes(monkeypatch):
    """vis_decode_proj_ws_bytes of the built library where it answers without a device, else a stand-in; the calls made."""
    calls = []
    try:
        real = hip.load().vis_decode_proj_ws_bytes
        real(3, 512, 256, 0)
    except Exception:
        real = None

    def ws(bm, n, k, f8):
        calls.append((bm, n, k, f8))
        got = int(real(bm, n, k, f8)) if real is not None else 0
        return got if got > 0 else 64 * n
    monkeypatch.setattr(decode_stage.hip, "load", lambda: types.SimpleNamespace(vis_decode_proj_ws_bytes=ws))
    return calls


def test_fp8_fused(monkeypatch, ws_bytes):
    st = make(monkeypatch, 3, fused_env=True, decode_weights="fp8")
    assert st.fp8_batched and st.fused_proj
    assert has(st, ROWS + FP8 + FP8_FUSED + FUSED) == list(ROWS + FP8 + FP8_FUSED + FUSED)
    assert [tuple(getattr(st, n).shape) for n in FP8_FUSED] == [(3, H // 32), (3, H // 32), (3, 768 // 32)]      # MX scale widths
    assert st.b_ssq1.shape == st.b_ssq2.shape == (H // hip.SSQ_UNIT, hip.SSQ_LD)
    assert not any(getattr(st, n).any() for n in FP8_FUSED + ("b_ssq1", "b_ssq2", "b_proj_ws"))
    assert ws_bytes == [(3, NQ, H, 1), (3, H, HQD, 0), (3, 2 * I, H, 1), (3, H, 768, 1), (3, CFG.vocab, H, 1)]
    assert st.b_proj_ws.dtype == torch.uint8 and st.b_proj_ws.numel() > 0
    assert not st.streamk_part and not hasattr(st, "b_part")      # every projection of the fused fp8 step is one launch


def test_bf16_fused_keeps_the_slabs(monkeypatch, ws_bytes):
    st = make(monkeypatch, 3, fused_env=True)
    assert st.fused_proj and has(st, FUSED) == list(FUSED) and has(st, FP8 + FP8_FUSED) == []
    assert ws_bytes == [(3, NQ, H, 0), (3, H, HQD, 0), (3, 2 * I, H, 0), (3, H, I, 0), (3, CFG.vocab, H, 0)]
    assert st.b_part.numel() == part_numel(3)      # the long-K down projection at many sequences
    assert not make(monkeypatch, 1, fused_env=True).fused_proj


def test_fused_step_for_bf16_weights_only(monkeypatch, ws_bytes):
    """fused_quantised=False (Mllama): the switch holds for bf16 weights alone; a quantised engine keeps the stream-K step."""
    st = make(monkeypatch, 3, fused_env=True, decode_weights="fp8", fused_quantised=False)
    assert not st.fused_proj and st.fp8_batched and has(st, FUSED + FP8_FUSED) == [] and st.b_part.numel() == part_numel(3)
    assert make(monkeypatch, 3, fused_env=True, fused_quantised=False).fused_proj


def test_mxfp4(monkeypatch):
    st = make(monkeypatch, 3, decode_weights="mxfp4")
    assert has(st, ROWS) == list(ROWS) and has(st, FP8 + FP8_FUSED + FUSED) == [] and st.kpad is None
    assert not st.streamk_part and not hasattr(st, "b_part")      # every batch size is the rows step's
    st = make(monkeypatch, 6, decode_weights="mxfp4", mxfp4_gemm_from=5)
    assert st.mxfp4_gemm_from == 5 and st.b_part.numel() == part_numel(6)
    assert make(monkeypatch, 33, decode_weights="mxfp4", mxfp4_gemm_from=5).b_part.numel() == 16 * 64 * max(NQ, H, 2 * I)


def test_cross_split_count_sizes_the_attention_workspace(monkeypatch):
    st = make(monkeypatch, 3, decode_splits=2, cross_splits=7)
    assert st.nsplit == 2
    assert st.part_o.numel() == 3 * CFG.heads * 7 * CFG.head_dim and st.part_ml.numel() == 3 * CFG.heads * 7 * 2
    st = make(monkeypatch, 3, decode_splits=4, cross_splits=2)
    assert st.part_o.numel() == 3 * CFG.heads * 4 * CFG.head_dim


def test_max_batch_bounds(monkeypatch):
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_batch must be in 1..64"):
            make(monkeypatch, bad)


def test_checks_are_the_stage_s(monkeypatch):
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    for cls in (Qwen2VLEngine, MllamaEngine):
        assert cls.check_decode_weights is DecodeStage.check_decode_weights
        assert cls.check_mxfp4_gemm_from is DecodeStage.check_mxfp4_gemm_from
    with pytest.raises(ValueError, match="decode_weights must be"):
        DecodeStage.check_decode_weights(CFG, "int4")
    with pytest.raises(ValueError, match="needs decode_weights='mxfp4'"):
        DecodeStage.check_mxfp4_gemm_from(CFG, "bf16", 5)


# ----------------------------------------------------------------------------- quantize_decode_weights
def _stand_ins(monkeypatch):
    """Quantisers that are easy to tell apart: codes = the weight's integer part + 1 (never 0), scales = the row index."""
    def q8(w):
        return (w.to(torch.uint8) + 1).contiguous(), torch.arange(w.shape[0], dtype=torch.float32)

    def q4(w):
        return (w[:, ::2].to(torch.uint8) + 1).contiguous(), torch.full((w.shape[0], w.shape[1] // 32), 127, dtype=torch.uint8)
    monkeypatch.setattr(decode_stage.hip, "quantize_fp8_rows", q8)
    monkeypatch.setattr(decode_stage.hip, "quantize_mxfp4_rows", q4)


def _layers(n, k_down):
    g = torch.Generator().manual_seed(0)
    mk = lambda r, c: torch.randint(0, 100, (r, c), generator=g).float()      # noqa: E731
    return [types.SimpleNamespace(qkv_w=mk(12, 64), o_w=mk(8, 64), gateup_w=mk(16, 64), down_w=mk(8, k_down))
            for _ in range(n)], mk(20, 64)


def test_quantize_pads_down_with_zero_columns_under_the_unpadded_scales(monkeypatch):
    _stand_ins(monkeypatch)
    layers, head = _layers(2, 704)
    q8, q4, h8, h4 = quantize_decode_weights(layers, head, True, False, pad_down=True)
    assert q4 == [] and h4 is None and len(q8) == 2 and h8[0].shape == (20, 64)
    for lw, q in zip(layers, q8):
        assert sorted(q) == ["down_w", "down_w_pad", "gateup_w", "o_w", "qkv_w"]
        codes, scales = q["down_w"]
        pad, pad_scales = q["down_w_pad"]
        assert codes.shape == (8, 704) and pad.shape == (8, 768) and pad.dtype == torch.uint8 and pad.is_contiguous()
        assert torch.equal(pad[:, :704], codes) and codes.all() and not pad[:, 704:].any()
        assert pad_scales is scales and torch.equal(scales, torch.arange(8, dtype=torch.float32))
        assert torch.equal(codes, lw.down_w.to(torch.uint8) + 1)


def test_quantize_pads_only_where_asked_and_needed(monkeypatch):
    _stand_ins(monkeypatch)
    layers, head = _layers(1, 704)
    assert "down_w_pad" not in quantize_decode_weights(layers, head, True, False)[0][0]
    layers, head = _layers(1, 768)
    assert "down_w_pad" not in quantize_decode_weights(layers, head, True, False, pad_down=True)[0][0]


def test_quantize_formats(monkeypatch):
    _stand_ins(monkeypatch)
    layers, head = _layers(2, 64)
    assert quantize_decode_weights(layers, head, False, False) == ([], [], None, None)
    q8, q4, h8, h4 = quantize_decode_weights(layers, head, False, True, pad_down=False)
    assert q8 == [] and h8 is None and len(q4) == 2 and sorted(q4[0]) == ["down_w", "gateup_w", "o_w", "qkv_w"]
    assert q4[1]["qkv_w"][0].shape == (12, 32) and q4[1]["qkv_w"][1].shape == (12, 2) and h4[0].shape == (20, 32)
