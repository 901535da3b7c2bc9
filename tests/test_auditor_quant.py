"""Quantised Auditor decode, the parts that need no GPU: the shape and name checks of MllamaEngine, the VIS_AUDITOR_*
variables on their way to the constructor, and the restatements of tests/cross_kv_ref.py (row quantiser, fp8 cross
attention, derived slack) checked against themselves."""
import dataclasses

import numpy as np
import pytest
import torch

import cross_kv_ref as X


def _cfg(**kw):
    from vision_inspection_system_amd.mllama_weights import MllamaConfig
    return dataclasses.replace(MllamaConfig.tiny(), **kw)


def test_check_decode_weights_names_and_shapes():
    from vision_inspection_system_amd.mllama_engine import MllamaEngine as E
    cfg = _cfg()
    for fmt in ("bf16", "fp8", "mxfp4"):
        E.check_decode_weights(cfg, fmt)
    for bad in ("int8", "", "FP8", None):
        with pytest.raises(ValueError):
            E.check_decode_weights(cfg, bad)
    odd = _cfg(intermediate=720)                       # a multiple of 16, not of 32
    E.check_decode_weights(odd, "fp8")
    with pytest.raises(ValueError, match="multiples of 32"):
        E.check_decode_weights(odd, "mxfp4")


def test_check_mxfp4_gemm_from():
    from vision_inspection_system_amd.mllama_engine import MllamaEngine as E
    cfg = _cfg()
    E.check_mxfp4_gemm_from(cfg, "bf16", None)
    E.check_mxfp4_gemm_from(cfg, "mxfp4", 5)
    E.check_mxfp4_gemm_from(cfg, "mxfp4", 64)
    for fmt in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="needs decode_weights='mxfp4'"):
            E.check_mxfp4_gemm_from(cfg, fmt, 5)
    for bad in (4, 65, True, 5.0, "5"):
        with pytest.raises(ValueError):
            E.check_mxfp4_gemm_from(cfg, "mxfp4", bad)
    with pytest.raises(ValueError, match="multiples of 64"):
        E.check_mxfp4_gemm_from(_cfg(intermediate=736), "mxfp4", 5)     # a multiple of 32, not of 64


def test_constructor_refuses_before_it_touches_the_device():
    """Bad names and shapes are ValueErrors raised before the library is loaded or a tensor is made: weights None, device 'cpu'."""
    from vision_inspection_system_amd.mllama_engine import MllamaEngine as E
    cfg = _cfg()
    for kw in (dict(cross_kv="int8"), dict(cross_kv="FP8"), dict(cross_kv=None), dict(decode_weights="nf4"),
               dict(decode_weights="fp8", mxfp4_gemm_from=5), dict(decode_weights="mxfp4", mxfp4_gemm_from=3)):
        with pytest.raises(ValueError):
            E(cfg, None, "cpu", **kw)
    E.check_cross_kv("bf16")
    E.check_cross_kv("fp8")


class _FakeEngine:
    calls = []

    def __init__(self, *a, **kw):
        type(self).calls.append((a, kw))
        self.tokenizer = None


@pytest.fixture()
def loader(monkeypatch):
    from vision_inspection_system_amd import client, mllama_engine
    from vision_inspection_system_amd import mllama_weights as MW
    monkeypatch.setattr(mllama_engine, "MllamaEngine", _FakeEngine)
    monkeypatch.setattr(MW, "pack_device_weights", lambda cfg, sd, device: "weights")
    monkeypatch.setattr(MW, "synth_state_dict", lambda cfg, seed: {})
    for v in ("VIS_AUDITOR_DECODE_WEIGHTS", "VIS_AUDITOR_MXFP4_GEMM_FROM", "VIS_AUDITOR_CROSS_KV", "VIS_DECODE_WEIGHTS",
              "VIS_MXFP4_GEMM_FROM"):
        monkeypatch.delenv(v, raising=False)
    _FakeEngine.calls = []
    return client


def test_unset_variables_make_todays_constructor_call(loader, monkeypatch):
    monkeypatch.setenv("VIS_DECODE_WEIGHTS", "fp8")          # the Inspector's switch is not the Auditor's
    monkeypatch.setenv("VIS_MXFP4_GEMM_FROM", "8")
    lm = loader._load_mllama("synthetic:mllama-tiny", "cpu", 256, 3)
    (args, kw), = _FakeEngine.calls
    assert args[1:] == ("weights", "cpu") and kw == dict(max_ctx=256, max_batch=3)
    assert lm.family == "mllama"
    assert loader._auditor_settings() == ("bf16", None, "bf16")


def test_auditor_variables_reach_the_constructor(loader, monkeypatch):
    monkeypatch.setenv("VIS_AUDITOR_DECODE_WEIGHTS", "mxfp4")
    monkeypatch.setenv("VIS_AUDITOR_MXFP4_GEMM_FROM", "5")
    monkeypatch.setenv("VIS_AUDITOR_CROSS_KV", "fp8")
    loader._load_mllama("synthetic:mllama-tiny", "cpu", 256, 2)
    (_, kw), = _FakeEngine.calls
    assert kw == dict(max_ctx=256, max_batch=2, decode_weights="mxfp4", mxfp4_gemm_from=5, cross_kv="fp8")
    assert loader._auditor_settings() == ("mxfp4", 5, "fp8")
    monkeypatch.setenv("VIS_AUDITOR_MXFP4_GEMM_FROM", "five")
    with pytest.raises(ValueError):
        loader._load_mllama("synthetic:mllama-tiny", "cpu", 256, 2)


def test_engine_cache_key_carries_the_auditor_settings(loader, monkeypatch):
    loader.drop_models()
    try:
        monkeypatch.setenv("VIS_AUDITOR_DECODE_WEIGHTS", "fp8")
        monkeypatch.setenv("VIS_AUDITOR_CROSS_KV", "fp8")
        a = loader.get_model("synthetic:mllama-tiny", "cpu")
        assert loader.get_model("synthetic:mllama-tiny", "cpu") is a
        monkeypatch.delenv("VIS_AUDITOR_DECODE_WEIGHTS")
        monkeypatch.delenv("VIS_AUDITOR_CROSS_KV")
        b = loader.get_model("synthetic:mllama-tiny", "cpu")
        assert b is not a and b.engine is not a.engine
        assert [kw.get("cross_kv") for _, kw in _FakeEngine.calls] == ["fp8", None]
        assert loader.get_model("synthetic:mllama-tiny") is b           # no device named: the entry of the current settings
    finally:
        loader.drop_models()


# ----------------------------------------------------------------------------- the restatements
def test_scale_constant_is_exact():
    assert np.float32(X.SCALE) * X.LOG2E_F32 == np.float32(0.125)


def test_e4m3_table_and_encoder_agree_with_torch():
    codes = torch.arange(256, dtype=torch.uint8)
    ref = codes.view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(ref), np.isnan(X.E4M3))
    assert np.array_equal(ref[~np.isnan(ref)], X.E4M3[~np.isnan(ref)])
    fin = X.FINITE_CODES
    back = X.e4m3_encode(X.E4M3[fin].astype(np.float32))
    assert np.array_equal(back[fin != 0x80], fin[fin != 0x80])
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(20000) * 100, rng.standard_normal(20000) * 0.02, rng.standard_normal(2000) * 1e-3,
                        [448.0, -448.0, 447.9, 464.0, 500.0, -1e9, 0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6]]
                       ).astype(np.float32)
    want = torch.from_numpy(x).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = X.e4m3_encode(x)
    assert np.array_equal(got & 0x7F, want & 0x7F) and np.array_equal((got >> 7)[x != 0], (want >> 7)[x != 0])


def edge_rows():
    """bf16-valued rows of 128 (float32) that sit on the quantiser's edges; shared with the GPU comparison."""
    rng = np.random.default_rng(7)
    bf = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()
    rows = [np.zeros(128)]                                              # all-zero row: scale 1e-12, codes 0
    for k in (-3, 0, 5):                                                # amax exactly 448 * 2^k: scale a power of two
        r = rng.standard_normal(128) * 100 * 2.0 ** k
        r[5] = 448.0 * 2.0 ** k
        rows.append(r)
    r = np.full(128, 1.0); r[0] = 1.96875 * 8; r[1:9] = [0.96875 * 8, 1.9375, 1.96875, 0.124, 0.1245, 15.5, 15.75, 7.75]
    rows.append(r)                                                      # values that round up to the next binade
    r = rng.standard_normal(128); r[3], r[4] = 3.0, -3.0
    rows.append(r)                                                      # +-max both present
    r = rng.standard_normal(128) * 2.0 ** -12; r[0] = 7.0
    rows.append(r)                                                      # most values in e4m3's denormal range after scaling
    rows.append(rng.standard_normal(128) * 1e-30)                       # amax / 448 below the floor of 1e-12
    rows.append(np.full(128, -2.0 ** -100))
    for s in (1e-3, 1.0, 300.0):
        rows.append(rng.standard_normal(128) * s)
    return bf(np.stack(rows))


def test_row_quantiser_restatement_on_the_edge_rows():
    x = edge_rows()
    codes, sc = X.quantize_rows(x)
    assert sc[0] == np.float32(1e-12) and not codes[0].any()
    assert [float(s) for s in sc[1:4]] == [2.0 ** -3, 1.0, 32.0] and all(codes[i][5] == 0x7E for i in (1, 2, 3))
    assert (codes[5] == 0x7E).any() and (codes[5] == 0xFE).any()
    assert ((codes[6] & 0x78) == 0).sum() > 64                          # denormal codes
    assert sc[7] == np.float32(1e-12) and not (codes[7] & 0x7F).any()
    # against torch's float8 cast on the same f32 products
    inv = (np.float32(1.0) / sc).astype(np.float32)
    want = torch.from_numpy((x * inv[:, None]).astype(np.float32)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(codes & 0x7F, want & 0x7F)
    deq = X.E4M3[codes] * sc[:, None].astype(np.float64)
    live = sc > np.float32(1e-12)                                       # (a row on the scale floor dequantises to zeros)
    assert np.all(np.abs(deq - x)[live] <= np.abs(x).max(axis=1, keepdims=True)[live] * 2.0 ** -4)


BOUND_SHAPES = ((2, 1), (32, 8))
TK = 256                                                                # four splits of 64
BOUND_NKEYS = (1, 63, 64, 65, 127, 128, 129, 256)


@pytest.mark.parametrize("Hq,Hkv", BOUND_SHAPES)
def test_float32_emulation_stays_inside_the_derived_slack(Hq, Hkv):
    """The fault-free kernel's order of operations in float32 lands inside [lo, hi] for every element of the chosen inputs -
    no element is excluded - and the interval is tight enough to mean something: a weight error of 2^-12 on one key's
    share shows."""
    q, w, kq, ksc, vq, vsc = X.bound_inputs(Hq, Hkv, TK, 0)
    qn = X.q_norm(q, w, 1e-5)
    assert np.array_equal(qn, q.astype(np.float64) * w)                 # the exact q_norm the inputs were made for
    for nkeys in BOUND_NKEYS:
        o, a, smax = X.attention(qn, kq, ksc, vq, vsc, nkeys)
        lo, hi = X.interval(o, a, smax, nkeys)
        got = X.attention_f32(qn, kq, ksc, vq, vsc, nkeys)
        assert np.all((got >= lo) & (got <= hi)), (nkeys, float(np.abs(got - o).max()))
        assert X.rel_slack(smax, -(-nkeys // 64)) < 2.0 ** -14          # far below bf16's half-ulp 2^-9
        assert float((lo != hi).mean()) <= 0.05
    bad_vsc = vsc.copy()
    bad_vsc[:, 0] *= np.float32(1.0 + 2.0 ** -3)
    o, a, smax = X.attention(qn, kq, ksc, vq, vsc, 64)
    lo, hi = X.interval(o, a, smax, 64)
    wrong = X.attention_f32(qn, kq, ksc, vq, bad_vsc, 64)
    assert not np.all((wrong >= lo) & (wrong <= hi))


@pytest.mark.parametrize("Hq,Hkv", BOUND_SHAPES)
def test_general_k_codes_slack_is_still_far_below_a_bf16_ulp(Hq, Hkv):
    """Arbitrary finite K codes: the emulation (one rounding of the exact dot product) is inside the widened interval, the
    widening stays below a quarter of bf16's half-ulp, and a K code decoded one step wrong on one key shows."""
    q, w, kq, ksc, vq, vsc = X.general_inputs(Hq, Hkv, TK, 0)
    qn = X.q_norm(q, w, 1e-5)
    assert len(np.unique(kq)) == len(X.FINITE_CODES)
    for nkeys in (65, 256):
        o, a, smax = X.attention(qn, kq, ksc, vq, vsc, nkeys)
        sabs = X.dot_abs(qn, kq, ksc, nkeys)
        lo, hi = X.interval(o, a, smax, nkeys, sabs)
        got = X.attention_f32(qn, kq, ksc, vq, vsc, nkeys)
        assert np.all((got >= lo) & (got <= hi))
        assert X.rel_slack(smax, 4) + 360 * sabs * X.U < 2.0 ** -11
    bad = kq.copy()
    bad[:, :64] = np.where((bad[:, :64] & 0x7F) < 0x7E, bad[:, :64] + 1, bad[:, :64])      # every code of a split one step up
    wrong = X.attention_f32(qn, bad, ksc, vq, vsc, 65)
    o, a, smax = X.attention(qn, kq, ksc, vq, vsc, 65)
    lo, hi = X.interval(o, a, smax, 65, X.dot_abs(qn, kq, ksc, 65))
    assert not np.all((wrong >= lo) & (wrong <= hi))


def test_malformed_auditor_variable_does_not_fail_another_models_lookup(loader, monkeypatch):
    """The variables are read only where an mllama model is loaded or cached: a registered non-mllama model is served."""
    loader.drop_models()
    try:
        monkeypatch.setenv("VIS_AUDITOR_MXFP4_GEMM_FROM", "five")
        lm = object()
        loader.register_model("some-inspector", "cpu", lm)
        assert loader.get_model("some-inspector", "cpu") is lm and loader.get_model("some-inspector") is lm
        with pytest.raises(ValueError):
            loader.get_model("synthetic:mllama-tiny", "cpu")
    finally:
        loader.drop_models()
