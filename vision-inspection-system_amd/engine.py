"""Qwen2-VL inference engine on MI355X: image frames + token ids -> generated token ids.

This is the local replacement of what the reference's remote endpoint does for one
``chat.completions.create`` call (src/agents/vlm_inspector.py:105-111).  The control flow is
Python; every arithmetic op is a gfx950 HIP kernel reached through ``hip.py`` (C ABI in
include/vis_hip.h).  PyTorch only allocates device memory, provides the HIP stream and
captures the per-token decode step into a hipGraph (``torch.cuda.CUDAGraph``).

Stages (kernel ids as in SURVEY.md section 8a):
  vision : K1 patchify+GEMM, then 32 x [K5 LN, K2 qkv GEMM, K4 2-D rope/split, K6 varlen attention,
           K2 proj(+res), K5 LN, K2 fc1(+QuickGELU), K2 fc2(+res)], merger (K5, K2+GELU, K2)
  prefill: K12 embed gather + image scatter, 28 x [K3, K2 qkv(+bias), K4 M-RoPE/split/KV write,
           K7 causal GQA attention, K2 o(+res), K3, K2 gate/up(+SwiGLU), K2 down(+res)], K10 lm_head, K12 argmax
  decode : per token, one hipGraph replay of 28 x [K10 qkv(+RMSNorm,+bias), K4 rope+KV append,
           K11 attention, K10 o(+res), K10 gate/up(+RMSNorm,+SwiGLU), K10 down(+res)], K10 lm_head, K12 argmax
"""
from __future__ import annotations

import collections
import logging
import os
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip, spec_batch
from .decode_stage import DecodeLayer, quantize_decode_weights
from .generation import Generation
from .request import Switches
from .config import Qwen2VLConfig
from .weights import DeviceWeights, PATCH_K_PAD, pad_cols


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- host-side position math
def vision_pos_hw(grids: Sequence[Tuple[int, int, int]], merge: int) -> np.ndarray:
    """(h, w) index of every patch, 2x2-merge-block order (TF vision_utils.get_vision_position_ids)."""
    out = []
    for (t, h, w) in grids:
        hp = np.broadcast_to(np.arange(h)[:, None], (h, w))
        wp = np.broadcast_to(np.arange(w)[None, :], (h, w))
        shape = (h // merge, merge, w // merge, merge)
        hp = hp.reshape(shape).transpose(0, 2, 1, 3).reshape(-1)
        wp = wp.reshape(shape).transpose(0, 2, 1, 3).reshape(-1)
        out.append(np.tile(np.stack([hp, wp], axis=-1), (t, 1)))
    return np.concatenate(out, axis=0)


def vision_cos_sin(cfg: Qwen2VLConfig, grids) -> Tuple[np.ndarray, np.ndarray]:
    """cos/sin rows [N, 80] f32 of the ViT 2-D rotary embedding (TF modeling_qwen2_vl.py:239-248,:719-722)."""
    dim = cfg.v_head_dim // 2
    inv_freq = (1.0 / (10000.0 ** (np.arange(0, dim, 2, dtype=np.float32) / np.float32(dim)))).astype(np.float32)
    pos = vision_pos_hw(grids, cfg.merge).astype(np.float32)
    freqs = (pos[:, :, None] * inv_freq[None, None, :]).reshape(pos.shape[0], -1)
    emb = np.concatenate([freqs, freqs], axis=-1)
    return np.cos(emb).astype(np.float32), np.sin(emb).astype(np.float32)


def vision_window_order(cfg: Qwen2VLConfig, grid: Tuple[int, int, int]) -> Tuple[np.ndarray, List[int]]:
    """Qwen2.5-VL window layout of ONE image (TF vision_utils.get_vision_window_index): the permutation of its 2x2 merge
    units into window order and the cumulative window boundaries in patch rows.  Windows are v_window pixels square
    (v_window / merge / patch merged tokens per side); the right / bottom windows of a grid are ragged."""
    t, h, w = grid
    win = cfg.v_window // cfg.merge // cfg.patch
    unit = cfg.merge ** 2
    lh, lw = h // cfg.merge, w // cfg.merge
    idx = np.arange(t * lh * lw).reshape(t, lh, lw)
    ph, pw = win - lh % win, win - lw % win               # the reference pads a whole window when already divisible
    nh, nw = (lh + ph) // win, (lw + pw) // win
    pad = np.pad(idx, ((0, 0), (0, ph), (0, pw)), constant_values=-100)
    pad = pad.reshape(t, nh, win, nw, win).transpose(0, 1, 3, 2, 4).reshape(t, nh * nw, win * win)
    seqlens = (pad != -100).sum(axis=2).reshape(-1)
    flat = pad.reshape(-1)
    cu = [0]
    for n in seqlens.tolist():
        if n:                                             # all-padding windows vanish (unique_consecutive)
            cu.append(cu[-1] + n * unit)
    return flat[flat != -100].astype(np.int64), cu


def rope_index(cfg: Qwen2VLConfig, input_ids: Sequence[int], grids) -> Tuple[np.ndarray, int]:
    """M-RoPE position ids [3, S] of one sequence and the next text position
    (TF modeling_qwen2_vl.py:914-1016: text runs count up on all 3 axes, an image block uses
    (t, h, w) over the merged grid and advances the text position by max(h, w) / merge)."""
    ids = np.asarray(list(input_ids))
    is_img = ids == cfg.image_token_id
    pos: List[np.ndarray] = []
    cur, i, g, n = 0, 0, 0, len(ids)
    while i < n:
        if is_img[i]:
            if g >= len(grids):
                raise ValueError("more image-token runs than images")
            t, h, w = grids[g]
            g += 1
            lh, lw = h // cfg.merge, w // cfg.merge
            cnt = t * lh * lw
            if i + cnt > n or not is_img[i:i + cnt].all():
                raise ValueError("image-token run does not match the image grid")
            tt = np.repeat(np.arange(t), lh * lw)
            hh = np.tile(np.repeat(np.arange(lh), lw), t)
            ww = np.tile(np.arange(lw), t * lh)
            pos.append(np.stack([tt, hh, ww]) + cur)
            cur += max(h, w) // cfg.merge
            i += cnt
        else:
            j = i
            while j < n and not is_img[j]:
                j += 1
            pos.append(np.broadcast_to(np.arange(j - i)[None, :], (3, j - i)) + cur)
            cur += j - i
            i = j
    if g != len(grids):
        raise ValueError("fewer image-token runs than images")
    p = np.concatenate(pos, axis=1).astype(np.int64)
    return p, int(p.max()) + 1


def mrope_cos_sin(cfg: Qwen2VLConfig, pos3: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """pos3 [3, S] -> cos/sin rows [S, head_dim] f32 with the (t,h,w) sections already selected per
    channel (TF modeling_qwen2_vl.py:156-170 + the cos.split(mrope_section*2) selection of :212-217)."""
    D = cfg.head_dim
    inv_freq = (1.0 / (np.float32(cfg.rope_theta) ** (np.arange(0, D, 2, dtype=np.float32) / np.float32(D))))
    inv_freq = inv_freq.astype(np.float32)
    axis = np.concatenate([np.full(s, i % 3) for i, s in enumerate(cfg.mrope_section)])  # [D/2]
    sel = pos3.astype(np.float32)[axis, :].T                                             # [S, D/2]
    freqs = sel * inv_freq[None, :]
    emb = np.concatenate([freqs, freqs], axis=-1)
    return np.cos(emb).astype(np.float32), np.sin(emb).astype(np.float32)


_LOG = logging.getLogger("vision_inspection_system_amd.engine")


# ----------------------------------------------------------------------------- engine
class Qwen2VLEngine(Generation):
    """One model replica on one GPU.  Not re-entrant: callers serialise through ``self.lock``."""

    speculative_supported = True      # generate(.., speculative=): spec.py

    def __init__(self, cfg: Qwen2VLConfig, weights: DeviceWeights, device, max_ctx: int = 4096,
                 decode_splits: int = 0, max_batch: int = 1, decode_weights: str = "bf16",
                 prefill_dtype: str = "bf16", mxfp4_gemm_from: Optional[int] = None, batch_speculative=None):
        """decode_weights="fp8" (BASELINE configs[4] slice, also VIS_DECODE_WEIGHTS=fp8): the single-sequence decode
        step streams OCP-e4m3 copies of the LLM projections and the lm_head (per-output-row f32 scales,
        hip.quantize_fp8_rows at load time) through vis_gemv_fp8w; prefill and the batched decode keep bf16.
        decode_weights="mxfp4" (VIS_DECODE_WEIGHTS=mxfp4): the same projections as OCP Microscaling FP4 (E2M1 codes, one
        E8M0 scale per 32 inputs, hip.quantize_mxfp4_rows at load time) through vis_gemv_mxfp4w at EVERY batch size: 2..4
        sequences share one pass over the weights (vis_gemv_mxfp4w_rows), larger batches issue each projection once per
        group of 4 rows, so a sequence decodes bit-identically alone or in any batch.  Embedding, norms, biases, the KV
        cache and the prompt pass stay bf16.
        mxfp4_gemm_from=n (5..64, VIS_MXFP4_GEMM_FROM, default None = off; mxfp4 only): steps with n or more sequences run the
        bf16 batched step's launches with every projection on vis_gemm_decode_mxfp4, which streams the FP4 weights ONCE
        for up to 64 sequences.  That makes TWO arithmetic families: the GEMV summation order below n, the MFMA stream-K
        order from n on.  Each is bit-invariant inside itself to batch size and row position; a request whose batch
        crosses n may differ at near-ties (the trade VIS_ROWS_GEMV makes), which is why it is off by default.
        batch_speculative=k | {..} (VIS_SPECULATIVE_BATCH, default None = off; spec_batch.py): generate_batch drafts up to k
        tokens per sequence by prompt lookup and runs B * (k + 1) rows through the stream-K step where it can
        (spec_batch.eligible) - the replies are the plain replies; a batch that cannot runs the plain step, silently."""
        cfg.validate_for_kernels()
        if batch_speculative is not None:      # kept off the instance otherwise: the class default None
            self.batch_speculative = spec_batch.check_setting(batch_speculative)
        self.check_decode_weights(cfg, decode_weights)
        self.check_mxfp4_gemm_from(cfg, decode_weights, mxfp4_gemm_from)
        if prefill_dtype not in ("bf16", "fp8"):
            raise ValueError("prefill_dtype must be 'bf16' or 'fp8'")
        if prefill_dtype == "fp8" and (cfg.hidden % 128 or (cfg.heads * cfg.head_dim) % 128):
            raise ValueError("fp8 prefill needs hidden and heads*head_dim to be multiples of 128")
        hip.load()  # fail loudly when the gfx950 library is missing: there is no other path
        if not torch.cuda.is_available():
            raise hip.HipLibraryError("Qwen2VLEngine needs a ROCm GPU (no CPU fallback exists)")
        self.cfg, self.w, self.device = cfg, weights, torch.device(device)
        self.max_ctx = _round_up(max_ctx, 64)
        self.lock = threading.Lock()
        self.prefill_dtype = prefill_dtype
        # what the decode stage works on (decode_stage.py): caches, counters, activation rows, workspaces, chain state, flags
        self._init_decode_state(max_batch, cfg.layers, decode_weights, mxfp4_gemm_from, decode_splits=decode_splits,
                                prefill_fp8=prefill_dtype == "fp8")
        dev = self.device
        # M-RoPE rows differ per request: every slot owns its tables; slot 0 doubles as the single-sequence engine
        self.cos_b = torch.zeros((max_batch, self.max_ctx, cfg.head_dim), dtype=torch.float32, device=dev)
        self.sin_b = torch.zeros((max_batch, self.max_ctx, cfg.head_dim), dtype=torch.float32, device=dev)
        self.cos_t, self.sin_t = self.cos_b[0], self.sin_b[0]
        # stacked suffix pass: rope / KV write / attention of the group's requests as ONE launch each (vis_*_many, per request
        # bit-identical to the per-request launches); VIS_GROUP_ATTN=0 keeps one launch per request (A/B)
        self.group_attn = os.environ.get("VIS_GROUP_ATTN", "1") == "1"
        self._chain_state: Optional[tuple] = None      # (ws, sync) kept while the chain is switched off after a stall
        self._chain_clean_requests = 0                 # requests served on the four launches since a stall
        # the LLM projections in e4m3 for the decode step and / or the fp8 prompt pass, in MXFP4 for the decode step
        self.q8, self.q4, self.q8_lm_head, self.q4_lm_head = quantize_decode_weights(
            weights.llm, weights.lm_head, decode_weights == "fp8" or prefill_dtype == "fp8", decode_weights == "mxfp4",
            pad_down=self.kpad is not None)
        self.vq8: List[dict] = []
        if prefill_dtype == "fp8" and cfg.v_mlp % 128 == 0 and os.environ.get("VIS_VIT_FP8", "1") == "1":
            # ViT block projections in e4m3 too (VIS_VIT_FP8=0 keeps the tower in bf16).  With only the 256x256 fp8 tile
            # this was slower than bf16 (M = 4900, N = 1280..5120 leaves 100-400 tiles for 256 CUs: 41.0 vs 40.3 ms);
            # with the 128x128 fp8 tile it pays: 39.8 -> 38.3 ms.  K = v_embed is zero-padded to a multiple of 128
            # when necessary (tiny: 320).
            self.vepad = _round_up(cfg.v_embed, 128)
            for b in weights.vit:
                q8 = {n: hip.quantize_fp8_rows(getattr(b, n)) for n in ("qkv_w", "proj_w", "fc1_w", "fc2_w")}
                self.vq8.append({n: (pad_cols(wq, 128), sc) for n, (wq, sc) in q8.items()})
        # keys [0, batch_shared_len) of the CURRENT batch's slots are identical copies of one text prefix (prefill_many):
        # the batched decode attention reads them from slot 0 (VIS_DECODE_SHARED=0: every sequence reads its own copy)
        self.batch_shared_len = 0
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self.min_shared_prefix = 256     # shorter common prefixes are not worth a separate pass
        # K / V / V^T of text prefixes seen before (prompt caching across requests): the reference's agents put the same
        # ~1000-token inspection prompt in front of every image (vlm_inspector.py:452-470), so a later request - single or
        # batched - computes only its rows from the image on.  LRU; VIS_PREFIX_CACHE = entries kept (0 = off), ~82 MB each
        # at 7B shapes and 960 tokens.
        self._prefix_cache: "collections.OrderedDict[bytes, dict]" = collections.OrderedDict()
        self.prefix_cache_hits = 0
        self._vis_rope_cache: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._rope_cache: Dict[tuple, tuple] = {}
        self._pairs_cache: Dict[tuple, torch.Tensor] = {}
        self._vis_work_cache: Dict[tuple, torch.Tensor] = {}
        self.last_first_logits: Optional[torch.Tensor] = None
        self.tokenizer = None
        # what the decode stage needs to know of the model; it also sets up the pick stage (pick.py)
        self._init_decode_stage([DecodeLayer(lw, self.q8[i] if self.q8 else None, self.q4[i] if self.q4 else None, False, i, lw.qkv_b)
                                 for i, lw in enumerate(weights.llm)], weights.final_norm_w, weights.lm_head,
                                self.q8_lm_head, self.q4_lm_head)

    # ------------------------------------------------------------------ vision tower
    def vision_forward(self, frames: Sequence[torch.Tensor], split_rows: bool = True) -> torch.Tensor:
        """frames: uint8 device tensors [H, W, 3] (H, W multiples of 28) -> [n_image_tokens, hidden] bf16."""
        cfg, w, dev, bf = self.cfg, self.w, self.device, torch.bfloat16
        grids = [(1, f.shape[0] // cfg.patch, f.shape[1] // cfg.patch) for f in frames]
        counts = [g[1] * g[2] for g in grids]
        # Every image starts on a 64-row boundary: the attention kernel walks keys in absolute 64-row tiles, so an
        # image's online-softmax grouping (and with it the bf16 rounding of its features) would otherwise depend on
        # what precedes it in the batch.  With aligned starts an image's features are bit-identical whether it runs
        # alone, second in a request, or batched with other requests' images (tests/test_engine_gpu.py).  The pad
        # rows (<= 60 per image) are zero patches that nothing attends to; they are dropped from the result.
        starts, s0 = [], 0
        for c in counts:
            starts.append(s0)
            s0 += _round_up(c, 64)
        N = starts[-1] + counts[-1]
        padded = N != sum(counts)
        E, Hh, D = cfg.v_embed, cfg.v_heads, cfg.v_head_dim
        kp = w.patch_w.shape[1]
        patches = (torch.zeros if padded else torch.empty)((N, kp), dtype=bf, device=dev)
        for f, r0 in zip(frames, starts):
            hip.patchify(f, patches, r0, cfg.image_mean, cfg.image_std)
        x = hip.gemm(patches, w.patch_w)
        key = tuple(grids)
        if key not in self._vis_rope_cache:
            c, s = vision_cos_sin(cfg, grids)
            if padded:
                cp, sp = np.zeros((N, c.shape[1]), c.dtype), np.zeros((N, s.shape[1]), s.dtype)
                o = 0
                for r0, n in zip(starts, counts):
                    cp[r0:r0 + n], sp[r0:r0 + n] = c[o:o + n], s[o:o + n]
                    o += n
                c, s = cp, sp
            self._vis_rope_cache[key] = (torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev))
            if len(self._vis_rope_cache) > 16:
                self._vis_rope_cache.pop(next(iter(self._vis_rope_cache)))
        cos, sin = self._vis_rope_cache[key]
        if cfg.vision_arch == "qwen2_5_vl":
            return self._vision_forward_windowed(x, grids, starts, counts, N, padded, cos, sin)
        segs = [(r0, r0 + c) for r0, c in zip(starts, counts)]
        work = self._vis_work_cache.get(tuple(segs))
        if work is None:
            if len(self._vis_work_cache) >= 16:
                self._vis_work_cache.clear()
            # key-split plan for long segments (one 1024 x 1024 image: 9 of 39 row blocks); VIS_ATTN_SPLIT=0: plain items (A/B)
            work = self._vis_work_cache[tuple(segs)] = hip.make_vit_attn_plan(
                segs, dev, Hh, split=(D == 80 and os.environ.get("VIS_ATTN_SPLIT", "1") != "0"))
        ld = _round_up(N, 64)
        y = torch.empty((N, E), dtype=bf, device=dev)
        qkv = torch.empty((N, 3 * E), dtype=bf, device=dev)
        q = torch.empty((Hh, N, D), dtype=bf, device=dev)
        k = torch.empty((Hh, N, D), dtype=bf, device=dev)
        vt = torch.empty((Hh, D, ld), dtype=bf, device=dev)
        att = (torch.zeros if padded else torch.empty)((N, E), dtype=bf, device=dev)     # pad rows are never written
        hmid = torch.empty((N, cfg.v_mlp), dtype=bf, device=dev)
        scale = D ** -0.5
        merger_ln_done = False
        if self.vq8:
            # fp8 configuration: the four block projections on the fp8 MFMA, LayerNorm fused into the activation quantiser
            xq = torch.zeros((N, self.vepad), dtype=torch.uint8, device=dev)      # pad columns stay 0
            hq = torch.empty((N, cfg.v_mlp), dtype=torch.uint8, device=dev)
            sx = torch.empty(N, dtype=torch.float32, device=dev)
            for b, q8 in zip(w.vit, self.vq8):
                hip.quant_rows_fp8(x, xq, sx, norm_w=b.ln1_w, norm_b=b.ln1_b, eps=1e-6)
                hip.gemm_fp8(xq, sx, *q8["qkv_w"], bias=b.qkv_b, out=qkv)
                hip.qkv_rope_split(qkv, cos, sin, q, k, None, vt, Hh, Hh, D)
                hip.attn_prefill_plan(q, k, vt, att, work, scale)
                hip.quant_rows_fp8(att, xq, sx)
                hip.gemm_fp8(xq, sx, *q8["proj_w"], bias=b.proj_b, residual=x, out=x)
                hip.quant_rows_fp8(x, xq, sx, norm_w=b.ln2_w, norm_b=b.ln2_b, eps=1e-6)
                hip.gemm_fp8(xq, sx, *q8["fc1_w"], bias=b.fc1_b, act=hip.ACT_QUICKGELU, out=hmid)
                hip.quant_rows_fp8(hmid, hq, sx)
                hip.gemm_fp8(hq, sx, *q8["fc2_w"], bias=b.fc2_b, residual=x, out=x)
        else:
            # fc2 (K = 5120, only 100 tiles of 256 x 256 at M = 4900) runs as two K-slices (200 workgroups) whose
            # finalisation - sum + bias + residual - is fused with the NEXT LayerNorm (the next block's norm1, or the
            # merger's ln_q after the last block): the row owner exists there, so the norm costs no pass of its own.
            # The choice depends on the layer shape only, never on the row count (an image's features must not depend
            # on what shares the batch).  VIS_VIT_FC2_SPLITK=0: plain fc2 GEMM + separate LayerNorm (A/B).
            splitk = cfg.v_mlp >= 1024 and os.environ.get("VIS_VIT_FC2_SPLITK", "1") != "0"
            swork = torch.empty(2 * N * E, dtype=torch.float32, device=dev) if splitk else None
            nb = len(w.vit)
            hip.layernorm(x, w.vit[0].ln1_w, w.vit[0].ln1_b, 1e-6, out=y)
            for bi, b in enumerate(w.vit):
                hip.gemm(y, b.qkv_w, bias=b.qkv_b, out=qkv)
                hip.qkv_rope_split(qkv, cos, sin, q, k, None, vt, Hh, Hh, D)
                hip.attn_prefill_plan(q, k, vt, att, work, scale)
                hip.gemm(att, b.proj_w, bias=b.proj_b, residual=x, out=x)
                hip.layernorm(x, b.ln2_w, b.ln2_b, 1e-6, out=y)
                hip.gemm(y, b.fc1_w, bias=b.fc1_b, act=hip.ACT_QUICKGELU, out=hmid)
                nw, nbias = (w.vit[bi + 1].ln1_w, w.vit[bi + 1].ln1_b) if bi + 1 < nb else (w.merger_ln_w, w.merger_ln_b)
                if splitk:
                    hip.gemm_splitk_part(hmid, b.fc2_w, swork, 2)
                    hip.splitk_finalize_norm(swork, 2, x, bias=b.fc2_b, residual=x, norm_w=nw, norm_b=nbias, y_out=y,
                                             eps=1e-6)
                else:
                    hip.gemm(hmid, b.fc2_w, bias=b.fc2_b, residual=x, out=x)
                    hip.layernorm(x, nw, nbias, 1e-6, out=y)
            merger_ln_done = True
        if not merger_ln_done:
            hip.layernorm(x, w.merger_ln_w, w.merger_ln_b, 1e-6, out=y)
        m = cfg.merge ** 2
        z = hip.gemm(y.view(N // m, E * m), w.merger_fc0_w, bias=w.merger_fc0_b, act=hip.ACT_GELU_ERF)
        out = hip.gemm(z, w.merger_fc2_w, bias=w.merger_fc2_b)
        if padded:
            out = torch.cat([out[r0 // m:(r0 + c) // m] for r0, c in zip(starts, counts)])
        return out

    def _vision_forward_windowed(self, x, grids, starts, counts, N: int, padded: bool, cos, sin) -> torch.Tensor:
        """Qwen2.5-VL tower (TF:models/qwen2_5_vl/modeling_qwen2_5_vl.py:408-472) on the patch-embedded rows ``x``: the
        2x2 merge units of every image are permuted into window order (one row gather; the rope rows move with them),
        blocks = RMSNorm -> qkv -> 2-D rope -> attention over the WINDOWS (work items of <= 64 rows) or, in the
        v_fullatt blocks, over the whole image -> proj(+res) -> RMSNorm -> gate/up GEMM with bias + SwiGLU epilogue ->
        down projection as two K-slices finalised together with the next RMSNorm; merger (RMSNorm, GELU MLP); the merged
        rows are gathered back into the original order.  Same kernels as the Qwen2-VL tower."""
        cfg, w, dev, bf = self.cfg, self.w, self.device, torch.bfloat16
        E, Hh, D = cfg.v_embed, cfg.v_heads, cfg.v_head_dim
        m = cfg.merge ** 2
        key = ("win", tuple(grids))
        lay = self._vis_work_cache.get(key)
        if lay is None:
            row_idx = np.arange(N, dtype=np.int32)                 # pad rows (if any) stay where they are
            rev = np.arange(N // m, dtype=np.int32)
            win_segs, full_segs = [], []
            for g, r0, c in zip(grids, starts, counts):
                widx, cu = vision_window_order(cfg, g)
                rows = (widx[:, None] * m + np.arange(m)[None, :]).reshape(-1)
                row_idx[r0:r0 + c] = r0 + rows
                rev[r0 // m:(r0 + c) // m] = r0 // m + np.argsort(widx)
                win_segs += [(r0 + a, r0 + b) for a, b in zip(cu[:-1], cu[1:])]
                full_segs.append((r0, r0 + c))
            c_np, s_np = vision_cos_sin(cfg, grids)                 # rope rows follow their patches: permuted on the host
            cp, sp = np.zeros((N, c_np.shape[1]), np.float32), np.zeros((N, s_np.shape[1]), np.float32)
            o = 0
            for r0, c in zip(starts, counts):
                cp[r0:r0 + c], sp[r0:r0 + c] = c_np[o:o + c], s_np[o:o + c]
                o += c
            if len(self._vis_work_cache) >= 16:
                self._vis_work_cache.clear()
            lay = self._vis_work_cache[key] = (
                torch.from_numpy(row_idx).to(dev), torch.from_numpy(rev).to(dev),
                hip.make_vit_attn_plan(win_segs, dev, Hh, split=False),
                hip.make_vit_attn_plan(full_segs, dev, Hh, split=(D == 80 and os.environ.get("VIS_ATTN_SPLIT", "1") != "0")),
                torch.from_numpy(cp[row_idx]).to(dev), torch.from_numpy(sp[row_idx]).to(dev))
        row_idx, rev, work_win, work_full, cw, sw = lay
        xw = torch.empty_like(x)
        hip.gather_rows(x, row_idx, xw)
        x = xw
        ld = _round_up(N, 64)
        pad = cfg.v_mlp_pad
        y = torch.empty((N, E), dtype=bf, device=dev)
        qkv = torch.empty((N, 3 * E), dtype=bf, device=dev)
        q = torch.empty((Hh, N, D), dtype=bf, device=dev)
        k = torch.empty((Hh, N, D), dtype=bf, device=dev)
        vt = torch.empty((Hh, D, ld), dtype=bf, device=dev)
        att = (torch.zeros if padded else torch.empty)((N, E), dtype=bf, device=dev)
        hmid = torch.empty((N, pad), dtype=bf, device=dev)
        swork = torch.empty(2 * N * E, dtype=torch.float32, device=dev)
        scale = D ** -0.5
        nb = len(w.vit)
        hip.rmsnorm(x, w.vit[0].ln1_w, 1e-6, out=y)
        for bi, b in enumerate(w.vit):
            hip.gemm(y, b.qkv_w, bias=b.qkv_b, out=qkv)
            hip.qkv_rope_split(qkv, cw, sw, q, k, None, vt, Hh, Hh, D)
            hip.attn_prefill_plan(q, k, vt, att, work_full if bi in cfg.v_fullatt else work_win, scale)
            hip.gemm(att, b.proj_w, bias=b.proj_b, residual=x, out=x)
            hip.rmsnorm(x, b.ln2_w, 1e-6, out=y)
            hip.gemm(y, b.fc1_w, bias=b.fc1_b, act=hip.ACT_SWIGLU, out=hmid)
            nw = w.vit[bi + 1].ln1_w if bi + 1 < nb else w.merger_ln_w
            hip.gemm_splitk_part(hmid, b.fc2_w, swork, 2)
            hip.splitk_finalize_norm(swork, 2, x, bias=b.fc2_b, residual=x, norm_w=nw, y_out=y, eps=1e-6)
        z = hip.gemm(y.view(N // m, E * m), w.merger_fc0_w, bias=w.merger_fc0_b, act=hip.ACT_GELU_ERF)
        out_w = hip.gemm(z, w.merger_fc2_w, bias=w.merger_fc2_b)
        out = torch.empty_like(out_w)
        hip.gather_rows(out_w, rev, out)
        if padded:
            out = torch.cat([out[r0 // m:(r0 + c) // m] for r0, c in zip(starts, counts)])
        return out

    # ------------------------------------------------------------------ prefill
    def prefill(self, input_ids: Sequence[int], frames: Sequence[torch.Tensor] = (),
                ids_dev: Optional[torch.Tensor] = None, taps: Optional[dict] = None,
                temperature: float = 0.0, seed: int = 0, max_new_tokens: Optional[int] = None,
                slot: int = 0, split_vit: bool = True, image_embeds: Optional[torch.Tensor] = None,
                prefix: Optional[dict] = None, collect_prefix: bool = False) -> Optional[dict]:
        """Run the prompt through the LLM, fill the KV cache of ``slot`` and pick the first token
        (greedy when temperature == 0, Gumbel-max sampled otherwise): the tower over the request's frames, then the text
        pass as a group of one (_prefill_group describes ``prefix``, ``collect_prefix`` and ``taps``).
        image_embeds: the merged ViT output of these frames computed elsewhere (prefill_many batches the tower over
        several requests' images)."""
        if not 0 <= slot < self.max_batch:
            raise ValueError("slot out of range")
        img = None
        if len(frames):
            img = image_embeds if image_embeds is not None else self.vision_forward(frames, split_rows=split_vit)
        return self._prefill_group([(slot, input_ids, ids_dev, img)], prefix, temperature, seed, max_new_tokens, frames,
                                   taps, collect_prefix)

    def _rope_tables(self, ids_np: np.ndarray, grids: Sequence[tuple], n_dec: int) -> tuple:
        """(cos, sin [S + n_dec, head_dim] f32, image-token scatter index) of a prompt structure, on the device.  The M-RoPE
        tables depend only on WHERE the image tokens sit, not on the text: the images of a batch inspection - and every
        request with the same prompt template and frame size - share them, so they are built once (host trigonometry + H2D)
        and kept.  Decode rows: slot S + t carries rope position next_pos + t on all three axes."""
        cfg, dev = self.cfg, self.device
        is_img = ids_np == cfg.image_token_id
        key = (len(ids_np), n_dec, tuple(grids), bool(is_img[0]), np.flatnonzero(np.diff(is_img.view(np.int8))).tobytes())
        hit = self._rope_cache.get(key)
        if hit is None:
            pos3, next_pos = rope_index(cfg, ids_np, grids)
            cos_np, sin_np = mrope_cos_sin(cfg, pos3)
            dpos = np.broadcast_to((next_pos + np.arange(n_dec))[None, :], (3, n_dec))
            dcos, dsin = mrope_cos_sin(cfg, dpos)
            img_idx = np.nonzero(is_img)[0].astype(np.int32)
            hit = (torch.from_numpy(np.concatenate([cos_np, dcos])).to(dev), torch.from_numpy(np.concatenate([sin_np, dsin])).to(dev),
                   torch.from_numpy(img_idx).to(dev))
            if len(self._rope_cache) >= 16:
                self._rope_cache.pop(next(iter(self._rope_cache)))
            self._rope_cache[key] = hit
        return hit

    def _llm_layers(self, x: torch.Tensor, qkv: torch.Tensor, att: torch.Tensor, attend, taps: Optional[dict] = None) -> None:
        """The decoder layers of the prompt pass over the M stacked rows of ``x`` (updated in place): bf16, or with every
        projection on the fp8 MFMA and the norms fused into the per-row activation quantiser (prefill_dtype="fp8",
        configs[4]).  ``attend(li)`` does rope / KV write / attention of layer li: it reads ``qkv`` and fills ``att``."""
        cfg, w, dev, bf = self.cfg, self.w, self.device, torch.bfloat16
        M, H = x.shape
        L = len(w.llm)
        fp8 = self.prefill_dtype == "fp8"
        act = torch.empty((M, cfg.intermediate), dtype=bf, device=dev)
        # The long-K down projection always runs as two K-slices (f32 partials, fixed-order sum): at S = 2249 its 126
        # 256x256 tiles would leave half the chip idle, and making the choice a function of the LAYER only (never of the
        # row count) keeps every row's summation order the same alone, in a group, and in the full, prefix and suffix pass.
        swork = None
        if (self.kpad if fp8 else cfg.intermediate) >= 8192 and H % 8 == 0:
            swork = torch.empty(2 * M * H, dtype=torch.float32, device=dev)
        if fp8:
            xq = torch.empty((M, H), dtype=torch.uint8, device=dev)
            aq = torch.empty((M, att.shape[1]), dtype=torch.uint8, device=dev)
            hq = torch.zeros((M, self.kpad), dtype=torch.uint8, device=dev)      # pad columns stay 0 (= +0.0 in e4m3)
            sx = torch.empty(M, dtype=torch.float32, device=dev)
        else:
            y = torch.empty((M, H), dtype=bf, device=dev)
            hip.rmsnorm(x, w.llm[0].ln1_w, cfg.rms_eps, out=y)
        for li, lw in enumerate(w.llm):
            if fp8:
                q8 = self.q8[li]
                hip.quant_rows_fp8(x, xq, sx, norm_w=lw.ln1_w, eps=cfg.rms_eps)
                hip.gemm_fp8(xq, sx, *q8["qkv_w"], bias=lw.qkv_b, out=qkv)
                attend(li)
                hip.quant_rows_fp8(att, aq, sx)
                hip.gemm_fp8(aq, sx, *q8["o_w"], residual=x, out=x)
                hip.quant_rows_fp8(x, xq, sx, norm_w=lw.ln2_w, eps=cfg.rms_eps)
                hip.gemm_fp8(xq, sx, *q8["gateup_w"], act=hip.ACT_SWIGLU, out=act)
                hip.quant_rows_fp8(act, hq[:, :cfg.intermediate], sx)
                hip.gemm_fp8(hq, sx, *q8.get("down_w_pad", q8["down_w"]), residual=x, out=x, work=swork, ksplit=2)
            else:
                hip.gemm(y, lw.qkv_w, bias=lw.qkv_b, out=qkv)
                attend(li)
                hip.gemm(att, lw.o_w, residual=x, out=x)
                hip.rmsnorm(x, lw.ln2_w, cfg.rms_eps, out=y)
                hip.gemm(y, lw.gateup_w, act=hip.ACT_SWIGLU, out=act)
                nxt = w.llm[li + 1].ln1_w if li + 1 < L else None      # the next layer's input norm rides on the finalisation
                if swork is not None:
                    hip.gemm_splitk_part(act, lw.down_w, swork, 2)
                    hip.splitk_finalize_norm(swork, 2, x, residual=x, norm_w=nxt, y_out=y if nxt is not None else None,
                                             eps=cfg.rms_eps)
                else:
                    hip.gemm(act, lw.down_w, residual=x, out=x)
                    if nxt is not None:
                        hip.rmsnorm(x, nxt, cfg.rms_eps, out=y)
            if taps is not None and li == 0:
                taps["layer0"] = x.clone()

    def _prefill_group(self, items: Sequence[tuple], prefix: Optional[dict], temperature: float, seed: int,
                       max_new_tokens: Optional[int], frames: Sequence[torch.Tensor] = (), taps: Optional[dict] = None,
                       collect_prefix: bool = False) -> Optional[dict]:
        """The text prompt pass of k >= 1 requests with one prompt structure over their stacked rows - the engine's only
        text pass: ``prefill`` is a group of one, the images of a batch inspection (same template, same frame size, one
        text prefix) are a group of several.

        items: [(slot, input_ids, ids_dev or None, image_embeds or None)] - all prompts have the same length S and the
        image tokens in the same places; ``frames``: the first request's (the sizes are the group's).
        ``prefix`` (from ``collect_prefix``): K / V / V^T of the first P tokens (P a multiple of 64, text only) computed by
        another pass over the SAME leading tokens - the reference puts the ~1000-token inspection prompt in front of the
        image (src/agents/vlm_inspector.py:462-470), so the images of a batch share it.  They are copied into every slot
        and only rows P.. are computed; every row's arithmetic is unchanged (row-independent GEMMs, attention key tiles
        on absolute 64-key boundaries), so the result is bit-identical to the full pass.
        ``collect_prefix`` (a group of one): run rows 0..S-1 only (no lm_head, no token) and return that bundle.
        ``taps`` (a group of one): image_embeds, layer0, first_logits.

        Per request n = S - P rows (7B bench prompt: 1289 = 5.04 row tiles of 256: a sixth of the LLM GEMM tiles is
        padding, and the qkv / o projections fill 0.42 / 0.33 of a round of the chip); stacked, k requests give k n rows
        (four: 20.1 tiles, 1.5 / 1.15 rounds).  Only the row-independent kernels see the stack - embedding gather,
        projections, norms, finalisations; rope / KV write / attention run per request on its own rows, KV-cache slot and
        V^T buffer, and a group of one issues exactly one request's launches.  A projection's K order does not depend on
        M, the down projection is two K-slices either way and key tiles are absolute, so a request's tokens and logits do
        not depend on its group (tests/test_engine_gpu.py, test_fullsize_gpu.py, test_qwen_prompt_pass_gpu.py)."""
        cfg, w, dev, bf = self.cfg, self.w, self.device, torch.bfloat16
        self.temperature, self.seed = float(temperature), int(seed)
        k = len(items)
        if k > 1 and (taps is not None or collect_prefix):
            raise ValueError("_prefill_group: taps and collect_prefix need a group of one")
        ids0 = np.asarray(list(items[0][1]), dtype=np.int64)
        S = len(ids0)
        if S < 1 or S + 1 > self.max_ctx:
            raise ValueError(f"prompt of {S} tokens does not fit the context of {self.max_ctx}")
        P = 0
        if prefix is not None:
            P = int(prefix["len"])
            if P % 64 or not 0 < P < S or collect_prefix:
                raise ValueError("bad shared prefix")
            if (ids0[:P] == cfg.image_token_id).any():
                raise ValueError("a shared prefix must be text only")
        n = S - P                                   # rows computed here, per request
        H, Hq, Hkv, D = cfg.hidden, cfg.heads, cfg.kv_heads, cfg.head_dim
        L = len(w.llm)
        n_dec = self.max_ctx - S if max_new_tokens is None else min(self.max_ctx - S, max_new_tokens + 1)
        grids = [(1, f.shape[0] // cfg.patch, f.shape[1] // cfg.patch) for f in frames]
        cos_all, sin_all, img_idx = self._rope_tables(ids0, grids, n_dec)
        is_img = ids0 == cfg.image_token_id
        ld = _round_up(S, 64)
        x = torch.empty((k * n, H), dtype=bf, device=dev)
        # V^T per layer: one buffer re-used by all layers, or - when a prefix is involved - one per layer, so that the
        # prefix columns can be copied in (or handed out) in one go
        per_layer_vt = bool(P) or collect_prefix
        vt_all = torch.empty((k, L if per_layer_vt else 1, Hkv, D, ld), dtype=bf, device=dev)
        ids_devs = []
        for j, (slot, ids, ids_dev, img) in enumerate(items):
            ids_np = np.asarray(list(ids), dtype=np.int64)
            if len(ids_np) != S or not np.array_equal(ids_np == cfg.image_token_id, is_img):
                raise ValueError("_prefill_group: the prompts of a group must share length and image positions")
            if P and not np.array_equal(ids_np[:P], prefix["ids"]):
                raise ValueError("the shared prefix does not match this prompt")
            if ids_np.min() < 0 or ids_np.max() >= cfg.vocab:
                raise ValueError("token id out of range")
            n_feat = 0 if img is None else img.shape[0]
            if n_feat != img_idx.shape[0]:
                raise ValueError(f"image tokens ({img_idx.shape[0]}) and image features ({n_feat}) do not match")
            self.cos_b[slot][:S + n_dec].copy_(cos_all, non_blocking=True)
            self.sin_b[slot][:S + n_dec].copy_(sin_all, non_blocking=True)
            if slot == 0:
                self.decode_limit = S + n_dec
            if ids_dev is None:
                ids_dev = hip.upload(ids_np.astype(np.int32), dev)
            ids_devs.append(ids_dev)
            xj = x[j * n:(j + 1) * n]
            hip.gather_rows(w.embed, ids_dev[P:] if P else ids_dev, xj)
            if img is not None:
                hip.scatter_rows(img, (img_idx - P) if P else img_idx, xj)
            if P:
                self.kcache_b[slot][:, :, :P].copy_(prefix["k"])
                self.vcache_b[slot][:, :, :P].copy_(prefix["v"])
                vt_all[j][:, :, :, :P].copy_(prefix["vt"])
        if taps is not None and items[0][3] is not None:
            taps["image_embeds"] = items[0][3]
        slots = [it[0] for it in items]
        s0 = slots[0]                         # every slot of the group now holds the same (contiguous) tables
        cos, sin = self.cos_b[s0][P:S], self.sin_b[s0][P:S]
        # causal pass over rows P..S-1: 128-row query blocks paired latest-with-earliest, one pair per workgroup
        # (hip.attn_prefill_pairs); VIS_ATTN_PAIRS=0 keeps one block per workgroup (A/B: same results, bit for bit) - for a
        # group of one, the only pass there was when the switch was measured; a group of several ignores it
        pairs = k > 1 or os.environ.get("VIS_ATTN_PAIRS", "1") != "0"
        if pairs:
            work = self._pairs_cache.get((P, S))
            if work is None:
                if len(self._pairs_cache) >= 64:
                    self._pairs_cache.clear()
                work = self._pairs_cache[(P, S)] = hip.make_attn_pairs(P, S, dev)
        elif P:
            blocks = [(q0, min(128, S - q0), 0, S) for q0 in range(P, S, 128)]
            blocks.sort(key=lambda it: -(it[0] + it[1]))
            work = torch.tensor(blocks, dtype=torch.int32, device=dev).reshape(-1, 4).contiguous()
        else:
            work = hip.make_attn_work([(0, S)], True, dev)
        qkv = torch.empty((k * n, (Hq + 2 * Hkv) * D), dtype=bf, device=dev)
        q = torch.empty((k, Hq, n, D), dtype=bf, device=dev)
        att = torch.empty((k * n, Hq * D), dtype=bf, device=dev)
        scale = D ** -0.5
        T = self.kcache_b.shape[3]
        many = self.group_attn and 1 < k <= hip.MAX_GROUP_REQUESTS and self.kcache_b.is_contiguous()

        def attend(li):        # rope / KV write / attention: per request, on its rows, cache slot and V^T buffer
            lv = li if per_layer_vt else 0
            if many:           # ... as ONE launch each for the whole group (r05: a 1289-row suffix alone fills a third of the chip)
                kv_off = [sl * self.kcache_b.stride(0) + li * self.kcache_b.stride(1) for sl in slots]
                vt_l = vt_all[:, lv]
                hip.qkv_rope_split_many(qkv, cos, sin, q, self.kcache_b, self.vcache_b, vt_l, Hq, Hkv, D, kv_off, T,
                                        k_pos0=P, vt_col0=P)
                hip.attn_prefill_pairs_many(q, self.kcache_b, vt_l, att, work, scale, kv_off, T, q_row0=P)
                return
            for j, slot in enumerate(slots):
                rows = slice(j * n, (j + 1) * n)
                kc, vc, vt = self.kcache_b[slot][li], self.vcache_b[slot][li], vt_all[j][lv]
                hip.qkv_rope_split(qkv[rows], cos, sin, q[j], kc, vc, vt, Hq, Hkv, D, k_pos0=P, vt_col0=P)
                if pairs:
                    hip.attn_prefill_pairs(q[j], kc, vt, att[rows], work, scale, q_row0=P)
                else:
                    hip.attn_prefill(q[j], kc, vt, att[rows], work, True, scale, q_row0=P)

        self._llm_layers(x, qkv, att, attend, taps)
        if collect_prefix:
            Pn = (S // 64) * 64
            return {"len": Pn, "ids": ids0[:Pn].copy(), "k": self.kcache_b[s0][:, :, :Pn].clone(),
                    "v": self.vcache_b[s0][:, :, :Pn].clone(), "vt": vt_all[0][:, :, :, :Pn].clone()}
        # first token: final norm fused into the lm_head GEMV of every request's last position only - for a group of 2..4 in
        # ONE pass over its 1.09 GB (vis_gemv_bf16_rows: every row bit-identical to the single-row GEMV) instead of one pass
        # per request; VIS_GROUP_ATTN=0 keeps the per-request calls
        grouped = self.group_attn and 1 < k <= 4 and H * 2 * (2 if k <= 2 else 4) <= 152 * 1024
        if grouped:
            lg = torch.empty((k, self.logits_b.shape[1]), dtype=torch.float32, device=dev)
            hip.gemv_rows(x[n - 1::n], w.lm_head, lg, norm_w=w.final_norm_w, eps=cfg.rms_eps)
        for j, slot in enumerate(slots):
            logits = self.logits_b[slot]
            if grouped:
                logits.copy_(lg[j])
            else:
                hip.gemv(x[(j + 1) * n - 1], w.lm_head, logits, norm_w=w.final_norm_w, eps=cfg.rms_eps)
            if taps is not None:
                taps["first_logits"] = logits.clone()
            self.step_b[slot:slot + 1].fill_(S - 1)
            self._prompt_pick(slot, ids_devs[j], logits, self.tokens_b[slot], self.cur_b[slot:slot + 1], self.step_b[slot:slot + 1])
            self.slot_prompt_len[slot] = S
            if slot == 0:
                self.prompt_len = S
                self._decoded = 0
        return None

    def prefill_many(self, requests: Sequence, temperature: float = 0.0,
                     seed: int = 0, max_new_tokens: Optional[int] = None,
                     ids_dev: Optional[Sequence[torch.Tensor]] = None,
                     seeds: Optional[Sequence[int]] = None,
                     penalties: Optional[Sequence[tuple]] = None,
                     shaping: Optional[Sequence[tuple]] = None,
                     ban: Optional[Sequence[tuple]] = None) -> Tuple[List[Optional[int]], List[Optional[Exception]]]:
        """Prefill the requests into consecutive slots.  The prefills are independent kernel chains: they are issued round-robin
        on a few HIP streams (VIS_PREFILL_STREAMS, default 2: 418 -> 381 ms for 8 images) so that the ragged last round of one image's GEMM /
        attention grids is filled by another image's workgroups.  Returns with the current stream ordered after
        all of them.

        A request is ``(input_ids, frames)`` or a zero-argument callable returning that pair (LAZY form, used by the
        batch seam: the callable waits for the image's host decode and uploads it, so the GPU starts on image 0 while
        images 1.. are still being decoded).  Lazy requests are resolved in order, a ViT group at a time; one that
        raises gets no slot and its exception is returned instead of failing the batch.
        ``seeds``: request b's own sampling seed (read by the picks while nucleus sampling / seeds are on).
        ``penalties``: request b's (repetition, frequency, presence) penalties (read by the picks while penalties are on).
        ``shaping``: request b's (top_k, min_p, bias list) (read by the picks while logit shaping is on).
        ``ban``: request b's (no_repeat_ngram_size, min_tokens) (read by the picks while token bans are on).
        Returns (slot of request b or None, exception of request b or None)."""
        B = len(requests)
        lazy = any(callable(r) for r in requests)
        resolved: List[Optional[tuple]] = [None] * B
        errors: List[Optional[Exception]] = [None] * B
        slots: List[Optional[int]] = [None] * B

        def get(b):
            if resolved[b] is None and errors[b] is None:
                r = requests[b]
                if callable(r):
                    try:
                        r = r()
                    except Exception as e:      # noqa: BLE001 - stays this request's own failure
                        errors[b] = e
                        return None
                resolved[b] = r
            return resolved[b]

        n_streams = max(1, min(B, int(os.environ.get("VIS_PREFILL_STREAMS", "2"))))
        vb = max(1, int(os.environ.get("VIS_VIT_BATCH", "4"))) if n_streams > 1 else 1
        # The text in front of the first image is the same for every image of a batch inspection (the reference's
        # INSPECTOR_PROMPT, vlm_inspector.py:452-470): its K / V / V^T are computed once and copied into every slot.
        # Eager requests: the prefix common to ALL prompts; lazy requests: the prefix common to the first group (the
        # others are not known yet) - a later prompt that does not start with it is simply computed in full.
        first = [r for r in (get(b) for b in range(B if not lazy else min(B, max(vb, 2)))) if r is not None]
        shared = None
        P = self.shared_prefix_len([r[0] for r in first]) if (B > 1 and len(first) > 1) else 0
        if P:
            shared = self.cached_prefix(first[0][0], P, temperature, seed)
        unshared = [False]        # set when some slot of this batch did NOT take the shared prefix

        def prefix_for(ids):
            if shared is None or len(ids) <= P:
                unshared[0] = True
                return None
            hit = np.array_equal(np.asarray(list(ids[:P]), dtype=np.int64), shared["ids"])
            if not hit:
                unshared[0] = True
            return shared if hit else None

        def place(slot, b):       # request b's own switches, where the picks of its slot read them
            for table, rows in ((self._slot_seed, seeds), (self._slot_pen, penalties), (self._slot_shape, shaping),
                                (self._slot_ban, ban)):
                if rows is not None:
                    table[slot] = rows[b]

        self.batch_shared_len = 0

        next_slot = 0
        if n_streams == 1:
            for b in range(B):
                r = get(b)
                if r is None:
                    continue
                place(next_slot, b)
                self.prefill(r[0], r[1], ids_dev=ids_dev[b] if ids_dev else None, temperature=temperature, seed=seed,
                             max_new_tokens=max_new_tokens, slot=next_slot, prefix=prefix_for(r[0]))
                slots[b] = next_slot
                next_slot += 1
            if shared is not None and not unshared[0] and os.environ.get("VIS_DECODE_SHARED", "1") != "0":
                self.batch_shared_len = P
            return slots, errors
        cur = torch.cuda.current_stream(self.device)
        if len(self._prefill_streams) < n_streams:
            self._prefill_streams = [torch.cuda.Stream(device=self.device) for _ in range(n_streams)]
        streams = self._prefill_streams[:n_streams]
        cfg = self.cfg
        for g0 in range(0, B, vb):
            grp_all = [b for b in range(g0, min(B, g0 + vb)) if get(b) is not None]
            # One ViT pass over the images of up to VIS_VIT_BATCH requests (default 4): at M = 4 x 4900 rows the tower's
            # GEMM grids become whole rounds of the chip (fc1 6.02, fc2 3.0, proj 3.0, qkv 9.02 rounds instead of
            # 1.56 / 0.78 / 0.76 / 2.29) and the varlen attention kernel takes the images as segments of one launch.
            embeds = {}
            grp = [b for b in grp_all if len(resolved[b][1])]
            if vb > 1 and len(grp) >= 2:
                out = self.vision_forward([f for b in grp for f in resolved[b][1]], split_rows=False)
                r0 = 0
                for b in grp:
                    n = sum((f.shape[0] // cfg.patch) * (f.shape[1] // cfg.patch) // cfg.merge ** 2 for f in resolved[b][1])
                    embeds[b] = out[r0:r0 + n]
                    r0 += n
            # Requests of the group that share the text prefix AND the prompt structure (the images of a batch inspection)
            # run their suffix rows as ONE stacked pass (_prefill_group: full LLM GEMM tiles and rounds instead of
            # 5.04-tile, 0.4-round grids per image); VIS_MERGE_PREFILL=0 keeps one pass per request (A/B, same results).
            merged: List[int] = []
            if shared is not None and os.environ.get("VIS_MERGE_PREFILL", "1") != "0":
                cand = [b for b in grp_all if b in embeds and prefix_for(resolved[b][0]) is not None]
                if len(cand) >= 2:
                    first_ids = np.asarray(list(resolved[cand[0]][0]), dtype=np.int64)
                    same = [b for b in cand if len(resolved[b][0]) == len(first_ids)
                            and embeds[b].shape[0] == embeds[cand[0]].shape[0]
                            and [f.shape for f in resolved[b][1]] == [f.shape for f in resolved[cand[0]][1]]
                            and np.array_equal(np.asarray(list(resolved[b][0]), dtype=np.int64) == cfg.image_token_id,
                                               first_ids == cfg.image_token_id)]
                    if len(same) >= 2:
                        merged = same
            slot_of = {b: next_slot + i for i, b in enumerate(grp_all)}       # slots follow the request order
            for b in grp_all:
                place(slot_of[b], b)
            next_slot += len(grp_all)
            if merged:
                st = streams[(g0 // vb) % n_streams]         # consecutive groups alternate streams
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    items = []
                    for b in merged:
                        ids, frames = resolved[b]
                        for f in frames:
                            f.record_stream(st)
                        embeds[b].record_stream(st)
                        items.append((slot_of[b], ids, ids_dev[b] if ids_dev else None, embeds[b]))
                        slots[b] = slot_of[b]
                    self._prefill_group(items, shared, temperature, seed, max_new_tokens, resolved[merged[0]][1])
            for b in grp_all:
                if b in merged:
                    continue
                ids, frames = resolved[b]
                st = streams[slot_of[b] % n_streams]
                st.wait_stream(cur)              # the frames' upload / resize and the group's ViT pass ran on `cur`
                with torch.cuda.stream(st):
                    for f in frames:
                        f.record_stream(st)
                    if b in embeds:
                        embeds[b].record_stream(st)
                    self.prefill(ids, frames, ids_dev=ids_dev[b] if ids_dev else None, temperature=temperature, seed=seed,
                                 max_new_tokens=max_new_tokens, slot=slot_of[b], split_vit=False, image_embeds=embeds.get(b),
                                 prefix=prefix_for(ids))
                slots[b] = slot_of[b]
        for st in streams:
            cur.wait_stream(st)
        if shared is not None:
            for t in (shared["k"], shared["v"], shared["vt"]):
                for st in streams:
                    t.record_stream(st)
        if shared is not None and not unshared[0] and os.environ.get("VIS_DECODE_SHARED", "1") != "0":
            self.batch_shared_len = P
        return slots, errors

    def text_prefix_len(self, ids: Sequence[int]) -> int:
        """Length (a multiple of 64, 0 = none worth keeping) of the text-only prefix of ONE prompt: everything in front of its
        first image, leaving at least one row to compute."""
        cfg = self.cfg
        a = np.asarray(list(ids), dtype=np.int64)
        special = np.nonzero((a == cfg.image_token_id) | (a == cfg.vision_start_id))[0]
        P = int(special[0]) if special.size else len(a) - 1
        P = (min(P, len(a) - 1) // 64) * 64
        return P if P >= self.min_shared_prefix else 0

    def cached_prefix(self, ids: Sequence[int], P: int, temperature: float = 0.0, seed: int = 0) -> Optional[dict]:
        """The K / V / V^T bundle of ``ids[:P]`` (P from text_prefix_len / shared_prefix_len): from the cache, or computed
        now (one pass over those rows - no more work than the full pass would have spent on them) and kept."""
        keep = int(os.environ.get("VIS_PREFIX_CACHE", "4"))
        if P <= 0:
            return None
        key = np.asarray(list(ids[:P]), dtype=np.int64).tobytes()
        hit = self._prefix_cache.get(key) if keep > 0 else None
        if hit is not None:
            self._prefix_cache.move_to_end(key)
            self.prefix_cache_hits += 1
            return hit
        bundle = self.prefill(list(ids[:P]), (), temperature=temperature, seed=seed, max_new_tokens=0, slot=0,
                              collect_prefix=True)
        if keep > 0:
            self._prefix_cache[key] = bundle
            while len(self._prefix_cache) > keep:
                self._prefix_cache.popitem(last=False)
        return bundle

    def shared_prefix_len(self, id_lists: Sequence[Sequence[int]]) -> int:
        """Length (a multiple of 64, 0 = do not share) of the text-only token prefix common to all prompts of a batch."""
        if len(id_lists) < 2 or os.environ.get("VIS_SHARE_PREFIX", "1") == "0":
            return 0
        cfg = self.cfg
        first = np.asarray(list(id_lists[0]), dtype=np.int64)
        P = len(first) - 1                       # every request keeps at least one row of its own
        for ids in id_lists[1:]:
            other = np.asarray(list(ids), dtype=np.int64)
            m = min(P, len(other) - 1)
            neq = np.nonzero(first[:m] != other[:m])[0]
            P = int(neq[0]) if neq.size else m
        special = np.nonzero((first[:P] == cfg.image_token_id) | (first[:P] == cfg.vision_start_id))[0]
        if special.size:
            P = int(special[0])
        P = (P // 64) * 64
        return P if P >= self.min_shared_prefix else 0

    # ------------------------------------------------------------------ decode
    def _decode_rope(self, B: int) -> tuple:
        """Every slot has its own M-RoPE rows; the batch's shared text prefix is read from slot 0 (DecodeStage hook)."""
        return self.cos_b[:B], self.sin_b[:B], self.batch_shared_len

    def _ensure_graph(self, batch: int = 0, chained: bool = False) -> torch.cuda.CUDAGraph:
        # temperature, seed and the batch size are kernel arguments baked into the graph; so is what _pick_key() names
        fork = bool(batch) and self.fork_on     # the fork tables are device memory: one graph for every layout
        key = (self.temperature, self.seed, batch, self.batch_shared_len if batch and not fork else 0,
               bool(chained) and not batch, fork) + self._pick_key() + self._stop_key() + self._shape_key() + self._stream_key() + self._ban_key()
        return self._captured_step(self._graphs, 8, key, batch, chained)

    def decode(self, n_steps: int, use_graph: bool = True) -> None:
        """Generate n_steps further tokens (each replays the captured step)."""
        if self.prompt_len + n_steps + 1 > self.max_ctx:
            raise ValueError("decode would overflow the KV cache")
        if self.prompt_len + self._decoded + n_steps > self.decode_limit:
            raise ValueError("decode beyond the rope rows prepared by prefill (pass max_new_tokens)")
        self._decode_ordered(n_steps, use_graph)

    def disable_chain(self) -> None:
        """Back to the four launches per layer head (same results bit for bit); the captured decode graphs hold chained launches
        and are dropped.  The (zeroed) workspace is kept: `_maybe_reenable_chain` switches back after VIS_CHAIN_RETRY_AFTER
        requests served cleanly on the four launches - one transient stall (a co-tenant's burst) does not cost the engine
        its faster step for good."""
        if self.chain_sync is not None:
            self._chain_state = (self.chain_ws, self.chain_sync)
        self.chain_sync = None
        self._chain_clean_requests = 0
        self._graphs.clear()

    def _maybe_reenable_chain(self) -> None:
        if self.chain_sync is not None or self._chain_state is None:
            return
        self._chain_clean_requests += 1
        retry_after = int(os.environ.get("VIS_CHAIN_RETRY_AFTER", "64"))
        if retry_after > 0 and self._chain_clean_requests >= retry_after:
            self.chain_ws, self.chain_sync = self._chain_state
            self._chain_state = None
            self.chain_sync.zero_()
            self.chain_ws.zero_()
            self._chain_launches = 0
            self._graphs.clear()
            _LOG.warning("vis_decode_chain: %d requests served on the four launches since the stall - chained layer head back on",
                         self._chain_clean_requests)

    # ------------------------------------------------------------------ generation (the loops: generation.Generation)
    def _fork_prefix_len(self) -> int:
        """The text prefix the batch's roots read from slot 0 (Generation hook)."""
        return self.batch_shared_len

    def _batch_graph(self, B: int) -> torch.cuda.CUDAGraph:
        return self._ensure_graph(B)

    def _clamp_request(self, input_ids: Sequence[int], max_new_tokens: int) -> int:
        """The reply clamped to the context in front of the prompt pass, which prepares that many rope rows (Generation
        hook); said once per engine: the reply may end before the model is done."""
        room = self.max_ctx - len(input_ids) - 1
        if max_new_tokens > room and not getattr(self, "_warned_clamp", False):
            self._warned_clamp = True
            _LOG.warning("max_tokens=%d does not fit the context (prompt %d + reply <= VIS_MAX_CTX=%d): generating at most %d",
                         max_new_tokens, len(input_ids), self.max_ctx, max(1, room))
        return max(1, min(max_new_tokens, room))

    def _prompt_pass(self, input_ids, frames, max_new_tokens, temperature, seed) -> None:
        """The single sequence's prompt pass (Generation hook)."""
        # the text in front of the image (the agents' fixed inspection prompt): its K / V come from the prefix cache
        P = self.text_prefix_len(input_ids) if os.environ.get("VIS_SHARE_PREFIX", "1") != "0" else 0
        prefix = self.cached_prefix(input_ids, P, temperature, seed) if P else None
        self.prefill(input_ids, frames, temperature=temperature, seed=seed, max_new_tokens=max_new_tokens, prefix=prefix)

    def generate(self, input_ids: Sequence[int], frames: Sequence[torch.Tensor] = (), max_new_tokens: int = 128,
                 ignore_eos: bool = False, use_graph: bool = True, check_every: int = 16,
                 temperature: float = 0.0, seed: int = 0, **switches) -> List[int]:
        """One request through the single-sequence loop (Generation._generate); ``switches``: the keywords request.Switches
        describes.  Here a reply that ended on EOS is cut in front of it, and a ``max_new_tokens`` the context cannot hold is
        clamped with a warning, once per engine (_clamp_request)."""
        return self._generate(input_ids, frames, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                              Switches.single(**switches))

    def generate_batch(self, requests: Sequence, max_new_tokens: int = 128, ignore_eos: bool = False, use_graph: bool = True,
                       check_every: int = 16, temperature: float = 0.0, seed: int = 0, **switches) -> list:
        """Up to max_batch requests through one shared decode loop (Generation._generate_batch); ``switches``: the keywords
        request.Switches describes.  The requests are [(input_ids, frames)], text-only ones included; prompts that start with
        the same text share its keys / values (prefill_many).  A prediction other than None is refused (ValueError):
        ``generate`` only."""
        return self._generate_batch(requests, max_new_tokens, ignore_eos, use_graph, check_every, temperature, seed,
                                    Switches.group(**switches))

    def _fork_model_state(self, root: int, child: int) -> None:
        """A further choice decodes at its root's M-RoPE positions (DecodeStage hook)."""
        self.cos_b[child].copy_(self.cos_b[root])
        self.sin_b[child].copy_(self.sin_b[root])
