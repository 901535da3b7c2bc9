"""The MFMA batched-decode projection on MXFP4 weights, host side (no GPU): the engine's static check of
``mxfp4_gemm_from``, the slot geometry query vis_gemm_decode_mxfp4_ksplit, and the argument errors of
vis_gemm_decode_mxfp4, all of which are decided before any HIP call."""
import dataclasses

import pytest

from vision_inspection_system_amd import hip
from vision_inspection_system_amd.config import Qwen2VLConfig
from vision_inspection_system_amd.engine import Qwen2VLEngine

SHAPES_7B = [(4608, 3584), (3584, 3584), (37888, 3584), (3584, 18944), (152064, 3584)]


# ----------------------------------------------------------------------------- the switch
def test_threshold_accepts_none_and_5_to_64():
    cfg = Qwen2VLConfig.tiny()
    for dw in ("bf16", "fp8", "mxfp4"):
        Qwen2VLEngine.check_mxfp4_gemm_from(cfg, dw, None)
    for v in (5, 6, 16, 33, 64):
        Qwen2VLEngine.check_mxfp4_gemm_from(cfg, "mxfp4", v)


@pytest.mark.parametrize("bad", [4, 65, "x", 0, -5, 5.0, True])
def test_threshold_bad_value_raises(bad):
    with pytest.raises(ValueError):
        Qwen2VLEngine.check_mxfp4_gemm_from(Qwen2VLConfig.tiny(), "mxfp4", bad)


@pytest.mark.parametrize("dw", ["bf16", "fp8"])
def test_threshold_needs_mxfp4_weights(dw):
    with pytest.raises(ValueError, match="mxfp4"):
        Qwen2VLEngine.check_mxfp4_gemm_from(Qwen2VLConfig.tiny(), dw, 5)


@pytest.mark.parametrize("field", ["hidden", "intermediate"])
def test_threshold_needs_dimensions_in_64s(field):
    """A dimension that holds whole MX blocks (a multiple of 32) but no whole 64-input K-step: fine for the GEMV form,
    refused for the MFMA form."""
    cfg = Qwen2VLConfig.tiny()
    bad = dataclasses.replace(cfg, **{field: getattr(cfg, field) + 32})
    assert getattr(bad, field) % 32 == 0 and getattr(bad, field) % 64 != 0
    with pytest.raises(ValueError, match=field):
        Qwen2VLEngine.check_mxfp4_gemm_from(bad, "mxfp4", 5)
    Qwen2VLEngine.check_mxfp4_gemm_from(bad, "mxfp4", None)


def test_constructor_checks_before_touching_the_gpu():
    """The constructor runs the static check first, so a bad value raises ValueError with or without a GPU."""
    cfg = Qwen2VLConfig.tiny()
    with pytest.raises(ValueError):
        Qwen2VLEngine(cfg, None, "cpu", decode_weights="mxfp4", mxfp4_gemm_from=4)
    with pytest.raises(ValueError):
        Qwen2VLEngine(cfg, None, "cpu", decode_weights="bf16", mxfp4_gemm_from=8)


def test_client_reads_the_environment_switch(monkeypatch):
    from vision_inspection_system_amd import client
    monkeypatch.delenv("VIS_MXFP4_GEMM_FROM", raising=False)
    assert client._env_int_or_none("VIS_MXFP4_GEMM_FROM") is None
    monkeypatch.setenv("VIS_MXFP4_GEMM_FROM", "")
    assert client._env_int_or_none("VIS_MXFP4_GEMM_FROM") is None
    monkeypatch.setenv("VIS_MXFP4_GEMM_FROM", "12")
    assert client._env_int_or_none("VIS_MXFP4_GEMM_FROM") == 12
    monkeypatch.setenv("VIS_MXFP4_GEMM_FROM", "x")
    with pytest.raises(ValueError):
        client._env_int_or_none("VIS_MXFP4_GEMM_FROM")


# ----------------------------------------------------------------------------- the slot geometry
def test_ksplit_query():
    lib = hip.load()
    q = lib.vis_gemm_decode_mxfp4_ksplit
    for N, K in [(0, 64), (-4, 3584), (128, 0), (128, 32), (128, 63)]:
        assert q(N, K) == 0, (N, K)
    for N, K in SHAPES_7B + [(128, 64), (1000, 704), (260, 2112), (132, 18944)]:
        s = q(N, K)
        assert 1 <= s <= 16, (N, K, s)
        assert hip.decode_gemm_mxfp4_ksplit(N, K) == s
        assert q(N, K) == s                      # nothing but (N, K) goes in: asked again, the same answer
    assert q(3584, 18944) > 1                    # a long K on few tiles is cut


# ----------------------------------------------------------------------------- argument errors, no launch
def _call(lib, A=256, Wq=512, Ws=768, part=1024, C=None, B=8, N=128, K=256, lda=None, ldq=None, lds=None, ldc=0, ksplit=0,
          out_f32=0):
    """Fake (never dereferenced) 16-byte aligned addresses: every call here must be refused by the host checks."""
    lda = K if lda is None else lda
    ldq = K // 2 if ldq is None else ldq
    lds = K // 32 if lds is None else lds
    return lib.vis_gemm_decode_mxfp4(A, Wq, Ws, part, C, B, N, K, lda, ldq, lds, ldc, ksplit, out_f32, None)


def test_argument_errors_without_gpu():
    lib = hip.load()
    ERR = 1   # VIS_ERR_ARG
    assert _call(lib, A=None) == ERR and _call(lib, Wq=None) == ERR and _call(lib, Ws=None) == ERR
    assert _call(lib, part=None, C=None) == ERR, "neither part nor C"
    assert _call(lib, A=256 + 8) == ERR and _call(lib, Wq=512 + 4) == ERR and _call(lib, part=1024 + 8) == ERR
    assert _call(lib, part=None, C=2048 + 2, ldc=128) == ERR, "misaligned C"
    assert _call(lib, B=4) == ERR and _call(lib, B=65) == ERR and _call(lib, B=0) == ERR
    assert _call(lib, K=96) == ERR, "K % 64 != 0"
    assert _call(lib, K=0) == ERR and _call(lib, N=0) == ERR and _call(lib, N=130) == ERR
    assert _call(lib, lda=252) == ERR and _call(lib, lda=128) == ERR, "lda % 8, lda < K"
    assert _call(lib, ldq=136) == ERR and _call(lib, ldq=112) == ERR, "ldq % 16, ldq < K/2"
    assert _call(lib, lds=7) == ERR, "lds < K/32"
    assert _call(lib, part=None, C=2048, ldc=130) == ERR and _call(lib, part=None, C=2048, ldc=64) == ERR
    need = lib.vis_gemm_decode_mxfp4_ksplit(3584, 18944)
    assert need > 1
    assert _call(lib, N=3584, K=18944, ksplit=need - 1) == ERR, "fewer slots than the geometry needs"
    assert _call(lib, N=3584, K=18944, ksplit=17) == ERR, "more slots than the layout holds"


def test_binding_checks_shapes():
    import torch
    x = torch.zeros((8, 256), dtype=torch.bfloat16)
    wq = torch.zeros((128, 128), dtype=torch.uint8)
    ws = torch.zeros((128, 8), dtype=torch.uint8)
    part = torch.zeros(16 * 16 * 128, dtype=torch.float32)
    with pytest.raises(hip.HipLibraryError):
        hip.decode_gemm_mxfp4(x, wq, ws)                                    # neither part nor out
    with pytest.raises(hip.HipLibraryError):
        hip.decode_gemm_mxfp4(x, wq, ws, part=part, out=part)               # both
    with pytest.raises(hip.HipLibraryError):
        hip.decode_gemm_mxfp4(x.float(), wq, ws, part=part)                 # x not bf16
    with pytest.raises(hip.HipLibraryError):
        hip.decode_gemm_mxfp4(x, wq, ws[:, :7], part=part)                  # too few scale bytes
    with pytest.raises(hip.HipLibraryError):
        hip.decode_gemm_mxfp4(x[:, :128], wq, ws, part=part)                # K mismatch
    with pytest.raises(hip.HipLibraryError):
        hip.decode_gemm_mxfp4(x, wq, ws, part=part[:100])                   # workspace too small
