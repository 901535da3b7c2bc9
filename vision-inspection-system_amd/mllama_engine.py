"""Row f2: Llama-3.2-11B-Vision ("mllama") on the same gfx950 kernel set - the model the
reference's Auditor falls back to (src/agents/vlm_auditor.py:81-83; request shape :152-158).

Everything arithmetic is a ``vis_*`` HIP entry point (hip.py); torch owns memory, streams and the hipGraph.
Published definition followed: transformers 5.15 ``models/mllama`` (``TF:``), see oracle/mllama_ref.py for the
CPU restatement the parity tests compare against.

Vision tower token order.  HF pads every tile from 1601 to 1608 tokens and masks only (padding x padding) pairs
(TF:modeling_mllama.py:75-99): real queries see every key, padding queries (pad rows and all rows of absent tiles)
see only real keys.  Attention is permutation-equivariant, so the tower runs on the order
    [ present tiles' 1601 tokens | absent tiles' 1601 tokens | the 7 pad rows of every tile ]
which makes both key sets contiguous ranges - two groups of plain work items for vis_attn_prefill - and leaves
the first max_tiles*1601 rows in exactly the order the cross-attention layers consume.

Scope: one image per prompt (what the reference sends).  Up to ``max_batch`` requests are in flight at once: every
request ("slot") owns its self-attention KV cache, its cross-attention keys/values and its position counter; prompt
passes run per request, then ONE decode loop serves all of them - every projection weight is streamed once per step
for the whole batch (gemm_decode_stream_kernel + skinny_finalize, the kernels of the Qwen2-VL batched decode), the
self-attention takes the sequence index on its grid and the cross-attention reads each sequence's own static keys
(vis_decode_cross_attn_batch).  Reference: VLMAuditorAgent.verify is called once per image of a batch
(src/agents/vlm_auditor.py:166-234, src/orchestration/graph.py:308-357).
"""
from __future__ import annotations

import math
import os
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .decode_stage import DecodeLayer, quantize_decode_weights
from .generation import Generation
from .request import Switches
from .mllama_weights import MllamaConfig, MllamaDeviceWeights


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- host logic (image geometry, rope)
def supported_aspect_ratios(max_tiles: int) -> List[Tuple[int, int]]:
    """TF:image_processing_pil_mllama.py get_all_supported_aspect_ratios."""
    return [(w, h) for w in range(1, max_tiles + 1) for h in range(1, max_tiles + 1) if w * h <= max_tiles]


def optimal_canvas(h: int, w: int, max_tiles: int, tile: int) -> Tuple[int, int]:
    """Canvas (height, width) in pixels: the smallest upscale >= 1 if one exists, else the largest downscale;
    ties go to the smallest area (TF:image_processing_pil_mllama.py get_optimal_tiled_canvas)."""
    best = None
    cands = []
    for (a, b) in supported_aspect_ratios(max_tiles):
        ch, cw = a * tile, b * tile
        sh, sw = ch / h, cw / w
        cands.append((sh if sw > sh else sw, ch, cw))
    ups = [c for c in cands if c[0] >= 1]
    sel = min(c[0] for c in ups) if ups else max(c[0] for c in cands if c[0] < 1)
    chosen = [c for c in cands if c[0] == sel]
    best = min(chosen, key=lambda c: c[1] * c[2]) if len(chosen) > 1 else chosen[0]
    # numpy's argmin takes the FIRST minimum; min() with a key does too
    return best[1], best[2]


def fit_to_canvas(h: int, w: int, ch: int, cw: int, tile: int) -> Tuple[int, int]:
    """TF:image_processing_pil_mllama.py get_image_size_fit_to_canvas."""
    tw = min(max(w, tile), cw)
    th = min(max(h, tile), ch)
    sh, sw = th / h, tw / w
    if sw < sh:
        return min(math.floor(h * sw) or 1, th), tw
    return th, min(math.floor(w * sh) or 1, tw)


def llama3_rope_tables(cfg: MllamaConfig, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """cos/sin [n, head_dim] f32 for positions 0..n-1 with the llama3 frequency scaling
    (TF:modeling_rope_utils.py llama3; TF:modeling_mllama.py:747-758).  float32 arithmetic like the reference."""
    D = cfg.head_dim
    inv = (1.0 / (np.float32(cfg.rope_theta) ** (np.arange(0, D, 2, dtype=np.float32) / np.float32(D)))).astype(np.float32)
    if cfg.rope_factor and cfg.rope_factor > 0:
        low_wl = cfg.rope_orig_ctx / cfg.rope_low_freq
        high_wl = cfg.rope_orig_ctx / cfg.rope_high_freq
        wl = (np.float32(2 * math.pi) / inv).astype(np.float32)
        inv_l = np.where(wl > low_wl, inv / np.float32(cfg.rope_factor), inv).astype(np.float32)
        smooth = ((np.float32(cfg.rope_orig_ctx) / wl - np.float32(cfg.rope_low_freq)) /
                  np.float32(cfg.rope_high_freq - cfg.rope_low_freq)).astype(np.float32)
        smoothed = ((1 - smooth) * inv_l / np.float32(cfg.rope_factor) + smooth * inv_l).astype(np.float32)
        medium = ~(wl < high_wl) & ~(wl > low_wl)
        inv = np.where(medium, smoothed, inv_l).astype(np.float32)
    freqs = np.arange(n, dtype=np.float32)[:, None] * inv[None, :]
    emb = np.concatenate([freqs, freqs], axis=1)
    return np.cos(emb).astype(np.float32), np.sin(emb).astype(np.float32)


class MllamaEngine(Generation):
    """One mllama replica on one GPU.  Not re-entrant: callers serialise through ``self.lock``."""

    @staticmethod
    def check_cross_kv(cross_kv: str) -> None:
        if cross_kv not in ("bf16", "fp8"):
            raise ValueError("cross_kv must be 'bf16' or 'fp8'")

    def __init__(self, cfg: MllamaConfig, weights: MllamaDeviceWeights, device, max_ctx: int = 4096, max_batch: int = 1,
                 decode_weights: str = "bf16", mxfp4_gemm_from: Optional[int] = None, cross_kv: str = "bf16",
                 speculative: bool = False, batch_speculative=None):
        """decode_weights="fp8" / "mxfp4" (VIS_AUDITOR_DECODE_WEIGHTS), mxfp4_gemm_from (VIS_AUDITOR_MXFP4_GEMM_FROM): the
        decode projections of EVERY layer - a cross-attention layer's q projection too - and the lm_head are quantised at load
        and decoded as on the Qwen2-VL engine (Qwen2VLEngine.__init__ describes the formats and the two arithmetic families
        of mxfp4_gemm_from); a quantised engine decodes the single sequence on the un-chained step.  The prompt pass, the
        vision tower, embedding, norms and both caches stay bf16.
        cross_kv="fp8" (VIS_AUDITOR_CROSS_KV): the decode step reads an e4m3 copy of the image's static cross-attention keys
        and values (codes + one f32 scale per key row, csrc/cross_attn.hip), written once per prompt pass from the bf16 rows;
        the bf16 rows stay (the prompt pass reads them), so the copy costs half as much memory again.  Independent of
        decode_weights.  Everything defaults to bf16: the launches of an engine built without these keywords are unchanged.
        speculative=True (VIS_AUDITOR_SPECULATIVE): ``generate`` accepts ``speculative=`` / ``prediction=`` for one greedy
        request - the lossless speculative step of the Qwen2-VL engines (DecodeStage._decode_step_spec), its cross-attention
        layers on vis_decode_cross_attn_draft / _fp8_draft according to cross_kv; every decode_weights format.  Nothing is
        allocated until the first such request, and a request without either argument issues the launches of before."""
        cfg.validate_for_kernels()
        if batch_speculative is not None:
            raise ValueError("batch_speculative is the Qwen2-VL / Qwen2.5-VL engine's: batched cross-attention rows have no draft form")
        self.check_decode_weights(cfg, decode_weights)
        self.check_mxfp4_gemm_from(cfg, decode_weights, mxfp4_gemm_from)
        self.check_cross_kv(cross_kv)
        if not isinstance(speculative, bool):
            raise ValueError("speculative must be True or False (the per-request k goes to generate)")
        self.speculative_supported = speculative
        hip.load()
        if not torch.cuda.is_available():
            raise hip.HipLibraryError("MllamaEngine needs a ROCm GPU (no CPU fallback exists)")
        self.cfg, self.w, self.device = cfg, weights, torch.device(device)
        self.max_ctx = _round_up(max_ctx, 64)
        self.lock = threading.Lock()
        dev, bf = self.device, torch.bfloat16
        Hkv, D = cfg.kv_heads, cfg.head_dim
        self.self_idx = [i for i in range(cfg.layers) if i not in cfg.cross_layers]
        self.n_self, self.n_cross = len(self.self_idx), len(cfg.cross_layers)
        self.TP = cfg.max_tiles * cfg.tile_tokens
        self.Tk = _round_up(self.TP, 64)
        self.xsplit = -(-self.Tk // hip.DECODE_KEYS_PER_SPLIT)
        # what the decode stage works on (decode_stage.py): caches, counters, activation rows, workspaces, chain state, flags.
        # The chained step covers the SELF-attention layers; the eight cross-attention layers keep their launches.
        self._init_decode_state(max_batch, self.n_self, decode_weights, mxfp4_gemm_from, cross_splits=self.xsplit,
                                fused_quantised=False)
        Bm = max_batch
        # per-request ("slot") cross-attention keys / values of the image; slot 0 doubles as the single-sequence engine
        self.xk_b = torch.zeros((Bm, self.n_cross, Hkv, self.Tk, D), dtype=bf, device=dev)
        self.xv_b = torch.zeros((Bm, self.n_cross, Hkv, self.Tk, D), dtype=bf, device=dev)
        self.cross_kv = cross_kv
        if cross_kv == "fp8":       # e4m3 codes + row scales of xk_b / xv_b, what the decode step's cross-attention reads
            self.xkq_b = torch.zeros((Bm, self.n_cross, Hkv, self.Tk, D), dtype=torch.uint8, device=dev)
            self.xvq_b = torch.zeros((Bm, self.n_cross, Hkv, self.Tk, D), dtype=torch.uint8, device=dev)
            self.xks_b = torch.zeros((Bm, self.n_cross, Hkv, self.Tk), dtype=torch.float32, device=dev)
            self.xvs_b = torch.zeros((Bm, self.n_cross, Hkv, self.Tk), dtype=torch.float32, device=dev)
        cos, sin = llama3_rope_tables(cfg, self.max_ctx)
        self.cos_t = torch.from_numpy(cos).to(dev)          # plain positions: one table for every sequence
        self.sin_t = torch.from_numpy(sin).to(dev)
        self.nkeys_b = torch.zeros(Bm, dtype=torch.int32, device=dev)
        self.xk, self.xv, self.nkeys_m1 = self.xk_b[0], self.xv_b[0], self.nkeys_b[0:1]
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self._graphs_b: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self._vis_plans: Dict[tuple, "hip.AttnPlan"] = {}
        self.has_image = False
        self.tokenizer = None
        # what the decode stage needs to know of the model; it also sets up the pick stage.  Quantised decode weights as on
        # the Qwen2-VL engine: every layer's four projections (a cross layer's qkv_w is its q projection) and the lm_head.
        q8, q4, q8_head, q4_head = quantize_decode_weights(weights.layers, weights.lm_head, decode_weights == "fp8",
                                                           decode_weights == "mxfp4", pad_down=self.kpad is not None)
        si = ci = 0
        layers = []
        for i, lw in enumerate(weights.layers):
            layers.append(DecodeLayer(lw, q8[i] if q8 else None, q4[i] if q4 else None, lw.cross, ci if lw.cross else si, None))
            ci, si = ci + lw.cross, si + (not lw.cross)
        self._init_decode_stage(layers, weights.norm_w, weights.lm_head, q8_head=q8_head, q4_head=q4_head)

    def _quantize_cross_kv(self, slot: int) -> None:
        """cross_kv="fp8": the e4m3 copy of slot ``slot``'s cross-attention keys / values, all cross layers in one launch each -
        once per prompt pass, after the bf16 rows of every cross layer have been written.  Every row of the buffer is
        quantised, rows at or past the request's key count too (whatever they hold: the decode kernel never uses them)."""
        hip.quantize_cross_kv(self.xk_b[slot], self.xkq_b[slot], self.xks_b[slot])
        hip.quantize_cross_kv(self.xv_b[slot], self.xvq_b[slot], self.xvs_b[slot])

    # ------------------------------------------------------------------ preprocessing (geometry on host, pixels on GPU)
    def prepare_image(self, frame: torch.Tensor):
        """uint8 device frame [H, W, 3] -> (resized frame, tiles_h, tiles_w, aspect_ratio_id); bilinear resample on
        the GPU, bit-exact with the PIL call of the HF processor."""
        cfg = self.cfg
        h, w = int(frame.shape[0]), int(frame.shape[1])
        ch, cw = optimal_canvas(h, w, cfg.max_tiles, cfg.image_size)
        th, tw = ch // cfg.image_size, cw // cfg.image_size
        nh, nw = fit_to_canvas(h, w, ch, cw, cfg.image_size)
        if (nh, nw) != (h, w):
            frame = hip.resize_rgb(frame.contiguous(), nh, nw, kind="bilinear")
        ar_id = supported_aspect_ratios(cfg.max_tiles).index((th, tw)) + 1
        return frame.contiguous(), th, tw, ar_id

    # ------------------------------------------------------------------ vision tower
    def _vision_plan(self, layout: Sequence[Tuple[int, int, int]]) -> "hip.AttnPlan":
        """Attention plan of the tower over a stack of canvases [(first row, present rows, canvas rows)]: a present tile's
        rows attend every canvas row, the pad rows only the present ones (HF's mask as two key ranges).  The long segment
        of a canvas (51 row blocks per head for 2 x 2 tiles, on 48 resident slots per head) is key-split up to whole rounds
        of the chip (hip.plan_attn_items_split; r04 - DESIGN section 4 had it as "does not yet"); the rule looks at one
        canvas only, so an image's features do not depend on what it is stacked with.  Measured (r04, exact 11B shapes, same
        box, alternating): ONE canvas 44.2 -> 43.1 ms per prompt pass (two rounds with the second 6 % full become 2.02 rounds of
        mostly half items), FOUR stacked canvases (the batch path) 33.75 -> 34.0 ms per image (4.3 rounds of whole items already
        fill the chip; the halves add merge work) - and one rule has to serve both, or an image's features would differ between
        the single and the batched path.  Hence OFF by default (VIS_MLLAMA_ATTN_SPLIT=1 turns it on)."""
        key = tuple(layout)
        plan = self._vis_plans.get(key)
        if plan is None:
            segs = []
            for r0, n_real, n_all in layout:
                segs.append((r0, r0 + n_real, r0, r0 + n_all))
                if n_all > n_real:
                    segs.append((r0 + n_real, r0 + n_all, r0, r0 + n_real))
            if len(self._vis_plans) >= 16:
                self._vis_plans.clear()
            plan = self._vis_plans[key] = hip.make_vit_attn_plan(
                segs, self.device, self.cfg.v_heads,
                split=(self.cfg.v_head_dim == 80 and os.environ.get("VIS_MLLAMA_ATTN_SPLIT", "0") == "1"))
        return plan

    def vision_forward(self, frame: torch.Tensor, taps: Optional[dict] = None) -> Tuple[torch.Tensor, int]:
        """uint8 device frame [H, W, 3] -> (cross-attention states [max_tiles*tile_tokens, hidden] bf16, n_tiles): a stack of one."""
        return self.vision_forward_many([frame], taps)[0]

    def vision_forward_many(self, frames: Sequence[torch.Tensor], taps: Optional[dict] = None) -> List[Tuple[torch.Tensor, int]]:
        """The tower over a stack of k >= 1 images in one pass -> [(cross-attention states [max_tiles*tile_tokens, hidden] bf16,
        n_tiles)] (k > 1 is the batch seam: verify_many).  One image is 6432 rows: its projections are 1 - 2 rounds of the chip
        (qkv 390 tiles, fc1 520) and its attention list 816 workgroups for 768 slots - two rounds, the second 6 % full; four
        images stacked make whole rounds of all of them.  Every image owns round_up(6432, 64) rows of the stack, whatever k: it
        starts on a 64-row boundary (the attention kernel walks keys in absolute 64-row tiles) and its rows see the same launches
        alone as stacked, so its features - and with them the whole answer - do not depend on what it is stacked with
        (test_batched_decode_matches_single_and_is_batch_invariant).  Row order inside an image: the module docstring.
        ``taps["vision_features"]``: the features of a single image in front of the projection."""
        k = len(frames)
        cfg, w, dev, bf = self.cfg, self.w, self.device, torch.bfloat16
        T, P, E, Hh, D = cfg.max_tiles, cfg.tile_tokens, cfg.v_hidden, cfg.v_heads, cfg.v_head_dim
        npad = (8 - P % 8) % 8
        TP, N = T * P, T * (P + npad)
        NS = _round_up(N, 64)                         # rows per image in the stack
        x = torch.zeros((k * NS, E), dtype=bf, device=dev)                 # pad rows start as exact zeros
        layout, n_tiles_of = [], []
        tile_of = np.concatenate([np.repeat(np.arange(T), P), np.repeat(np.arange(T), npad),
                                  np.zeros(NS - N, dtype=np.int64)]).astype(np.int32)
        idx_all = np.empty(k * NS, dtype=np.int32)
        for i, frame in enumerate(frames):
            fr, th, tw, ar_id = self.prepare_image(frame)
            n_tiles = th * tw
            n_tiles_of.append(n_tiles)
            r0, nR = i * NS, n_tiles * P
            patches = torch.zeros((TP, w.patch_w.shape[1]), dtype=bf, device=dev)
            hip.patchify_tiles(fr, patches, th, tw, cfg.image_size, cfg.image_mean, cfg.image_std)
            hip.gemm(patches, w.patch_w, residual=w.cls_pos[ar_id].view(TP, E), out=x[r0:r0 + TP])
            hip.layernorm(x[r0:r0 + TP], w.ln_pre_w, w.ln_pre_b, 1e-5, out=x[r0:r0 + TP])
            layout.append((r0, nR, N))
            idx_all[r0:r0 + NS] = ar_id * T + tile_of
        plan = self._vision_plan(layout)
        M = k * NS
        y = torch.empty((M, E), dtype=bf, device=dev)
        qkv = torch.empty((M, 3 * E), dtype=bf, device=dev)
        q = torch.empty((Hh, M, D), dtype=bf, device=dev)
        kk = torch.empty((Hh, M, D), dtype=bf, device=dev)
        vt = torch.empty((Hh, D, M), dtype=bf, device=dev)
        att = torch.zeros((M, E), dtype=bf, device=dev)          # the NS - N tail rows of an image are never written
        hmid = torch.empty((M, cfg.v_mlp), dtype=bf, device=dev)
        feats = torch.empty((k, TP, cfg.v_out), dtype=bf, device=dev)
        scale = D ** -0.5

        def layer(b):
            hip.layernorm(x, b.ln1_w, b.ln1_b, cfg.v_eps, out=y)
            hip.gemm(y, b.qkv_w, out=qkv)
            hip.qkv_rope_split(qkv, None, None, q, kk, None, vt, Hh, Hh, D)
            hip.attn_prefill_plan(q, kk, vt, att, plan, scale)
            hip.gemm(att, b.o_w, residual=x, out=x)
            hip.layernorm(x, b.ln2_w, b.ln2_b, cfg.v_eps, out=y)
            hip.gemm(y, b.fc1_w, bias=b.fc1_b, act=hip.ACT_GELU_ERF, out=hmid)
            hip.gemm(hmid, b.fc2_w, bias=b.fc2_b, residual=x, out=x)

        def take(col0):
            for i in range(k):
                feats[i][:, col0:col0 + E].copy_(x[i * NS:i * NS + TP])

        j = 0
        for li, b in enumerate(w.v_layers):
            layer(b)
            if li in cfg.v_inter:
                take(E * (1 + j))
                j += 1
        hip.layernorm(x, w.ln_post_w, w.ln_post_b, 1e-5, out=x)
        hip.add_rows(x, w.post_tile.view(-1, E), hip.upload(idx_all, dev))
        for b in w.v_global:
            layer(b)
        take(0)
        if taps is not None and k == 1:
            taps["vision_features"] = feats[0]
        cross = hip.gemm(feats.view(k * TP, cfg.v_out), w.proj_w, bias=w.proj_b)
        return [(cross[i * TP:(i + 1) * TP], n_tiles_of[i]) for i in range(k)]

    # ------------------------------------------------------------------ prefill
    def _check_prompt(self, input_ids: Sequence[int], has_frame: bool, slot: int) -> Tuple[np.ndarray, int]:
        """The argument checks of a prompt pass, before anything is launched -> (ids as int64, index of the image token; 0
        without an image)."""
        if not 0 <= slot < self.max_batch:
            raise ValueError("slot out of range")
        S = len(input_ids)
        if S < 1 or S + 1 > self.max_ctx:
            raise ValueError(f"prompt of {S} tokens does not fit the context of {self.max_ctx}")
        ids_np = np.asarray(list(input_ids), dtype=np.int64)
        if ids_np.min() < 0 or ids_np.max() >= self.cfg.vocab + 8:
            raise ValueError("token id out of range")
        locs = np.nonzero(ids_np == self.cfg.image_token_id)[0]
        if len(locs) > 1:
            raise ValueError("one image per prompt")
        if has_frame != (len(locs) == 1):
            raise ValueError("image token and image frame must come together")
        return ids_np, int(locs[0]) if has_frame else 0

    def prefill(self, input_ids: Sequence[int], frame: Optional[torch.Tensor] = None, taps: Optional[dict] = None,
                temperature: float = 0.0, seed: int = 0, slot: int = 0,
                cross_states: Optional[Tuple[torch.Tensor, int]] = None) -> None:
        """One request's prompt pass into ``slot``: the tower over its image, then the text pass as a group of one.
        cross_states: the tower's output for this frame computed elsewhere (prefill_many stacks several requests' images).
        taps: cross_states, layer{i} of every layer that ran, first_logits (and the tower's vision_features)."""
        self._check_prompt(input_ids, frame is not None, slot)
        cross, n_tiles = None, 0
        if frame is not None:
            cross, n_tiles = cross_states if cross_states is not None else self.vision_forward(frame, taps)
        self._prefill_group([(slot, input_ids, cross, n_tiles)], temperature, seed, taps)

    def _prefill_group(self, items: Sequence[tuple], temperature: float, seed: int, taps: Optional[dict] = None) -> None:
        """The text decoder's prompt pass of k >= 1 requests with one prompt layout over their stacked rows - the engine's only
        text pass: ``prefill`` is a group of one, verify_many (the same Auditor prompt in front of every image) one of several.
        items: [(slot, ids, cross_states, n_tiles)], all prompts S tokens long with the image token at the same index; a group of
        one may come without an image (cross_states None): its cross layers are skipped.  At S ~ 700 a request is 2.75 row tiles
        of 256: stacked, four give 11 (gate/up 112 x 3 = 1.3 rounds per request -> 4.8 for four).  Only the row-independent
        kernels see the stack (projections, norms); K / V projection of the image, rope / cache write and both attentions run per
        request, and a group of one issues exactly one request's launches.  The K order of every projection is M-independent and
        the K-slice counts are a function of the layer shape, so a request's tokens do not depend on its group
        (test_batched_decode_matches_single_and_is_batch_invariant).  taps (a group of one only): see ``prefill``."""
        cfg, w, dev, bf = self.cfg, self.w, self.device, torch.bfloat16
        self.temperature, self.seed = float(temperature), int(seed)
        k = len(items)
        S = len(items[0][1])
        has_image = items[0][2] is not None
        if (k > 1 and not has_image) or (taps is not None and k != 1):
            raise ValueError("_prefill_group: a prompt without an image, and taps, need a group of one")
        H, Hq, Hkv, D = cfg.hidden, cfg.heads, cfg.kv_heads, cfg.head_dim
        P, TP = cfg.tile_tokens, self.TP
        M = k * S
        x = torch.empty((M, H), dtype=bf, device=dev)
        nm, xworks, ids_devs = 0, [], []
        for j, (slot, ids, cross, n_tiles) in enumerate(items):
            ids_np, nm_j = self._check_prompt(ids, cross is not None, slot)
            if j == 0:
                nm = nm_j
            if len(ids_np) != S or (cross is not None) != has_image or nm_j != nm:
                raise ValueError("_prefill_group: the prompts of a group must share length and image-token position")
            ids_devs.append(hip.upload(ids_np.astype(np.int32), dev))
            hip.gather_rows(w.embed, ids_devs[j], x[j * S:(j + 1) * S])
            if has_image:
                nR = n_tiles * P
                self.nkeys_b[slot:slot + 1].fill_(nR - 1)
                xworks.append([(q0, min(128, nm - q0), 0, TP) for q0 in range(0, nm, 128)] +
                              [(q0, min(128, S - q0), 0, nR) for q0 in range(nm, S, 128)])
        if has_image:
            if taps is not None:
                taps["cross_states"] = items[0][2]
            xvt_all = torch.empty((k, Hkv, D, self.Tk), dtype=bf, device=dev)
            xwork_all = torch.tensor(xworks, dtype=torch.int32, device=dev).reshape(k, -1, 4).contiguous()   # same item count: same S, nm
            kvbuf = torch.empty((TP, 2 * Hkv * D), dtype=bf, device=dev)
            q2 = torch.empty((M, Hq * D), dtype=bf, device=dev)
        cos, sin = self.cos_t[:S], self.sin_t[:S]
        work = hip.make_attn_pairs(0, S, dev)        # causal self-attention: paired query blocks (hip.attn_prefill_pairs)
        ld = _round_up(S, 64)
        nq = (Hq + 2 * Hkv) * D
        y = torch.empty((M, H), dtype=bf, device=dev)
        qkv = torch.empty((M, nq), dtype=bf, device=dev)
        q = torch.empty((k, Hq, S, D), dtype=bf, device=dev)
        vt = torch.empty((k, Hkv, D, ld), dtype=bf, device=dev)
        att = torch.empty((M, Hq * D), dtype=bf, device=dev)
        act = torch.empty((M, cfg.intermediate), dtype=bf, device=dev)
        scale = D ** -0.5
        # Long-K projections at a prompt's few hundred rows (o: 3 x 16 tiles of 256^2 at K = 4096; down: the same tiles at
        # K = 14336) leave most of the chip idle as plain tiles: they run as K-slices (f32 slabs + fixed-order finalisation
        # with the residual, vis_gemm_bf16_splitk).  The slice count is a function of the LAYER shape only, never of the row
        # count, so a row's summation order - and slot / batch invariance - does not depend on the prompt (A/B: VIS_MLLAMA_SPLITK=0).
        ks_down = int(os.environ.get("VIS_MLLAMA_SPLITK", "4")) if cfg.intermediate >= 8192 else 0
        ks_o = int(os.environ.get("VIS_MLLAMA_SPLITK_O", "4")) if H >= 4096 else 0
        ks_qkv = int(os.environ.get("VIS_MLLAMA_SPLITK_QKV", "0"))
        swork = torch.empty(max(ks_down, ks_o, 1) * M * max(H, nq if ks_qkv else 0), dtype=torch.float32, device=dev) \
            if (ks_down or ks_o or ks_qkv) else None

        def proj(a, wt, ks):        # x += a @ wt.T
            if ks >= 2:
                hip.gemm_splitk(a, wt, swork, ks, residual=x, out=x)
            else:
                hip.gemm(a, wt, residual=x, out=x)

        Tc = self.kcache_b.shape[3]
        many = os.environ.get("VIS_GROUP_ATTN", "1") == "1" and 1 < k <= hip.MAX_GROUP_REQUESTS and self.kcache_b.is_contiguous()
        si = ci = 0
        for li, lw in enumerate(w.layers):
            if lw.cross:
                if not has_image:
                    ci += 1
                    continue                      # text-only prompt: cross layers are skipped (TF:...:1128-1138)
                for j, (slot, _, cross, _) in enumerate(items):
                    hip.gemm(cross, lw.kv_w, out=kvbuf)
                    hip.rmsnorm_heads(kvbuf, lw.k_norm, Hkv, cfg.rms_eps)     # k_norm on the Hkv key heads of every row (one launch)
                    hip.qkv_rope_split(kvbuf, None, None, None, self.xk_b[slot][ci], self.xv_b[slot][ci], xvt_all[j], 0, Hkv, D,
                                       k_pos0=0)
                hip.rmsnorm(x, lw.ln1_w, cfg.rms_eps, out=y)
                hip.gemm(y, lw.qkv_w, out=q2)
                hip.rmsnorm(q2.view(M * Hq, D), lw.q_norm, cfg.rms_eps, out=q2.view(M * Hq, D))
                if many and self.xk_b.is_contiguous():
                    xoff = [it[0] * self.xk_b.stride(0) + ci * self.xk_b.stride(1) for it in items]
                    for j in range(k):
                        hip.qkv_rope_split(q2[j * S:(j + 1) * S], None, None, q[j], None, None, None, Hq, 0, D)
                    hip.attn_prefill_many(q, self.xk_b, xvt_all, att, xwork_all, False, scale, xoff, self.Tk)
                else:
                    for j, (slot, _, _, _) in enumerate(items):
                        rows = slice(j * S, (j + 1) * S)
                        hip.qkv_rope_split(q2[rows], None, None, q[j], None, None, None, Hq, 0, D)
                        hip.attn_prefill(q[j], self.xk_b[slot][ci], xvt_all[j], att[rows], xwork_all[j], False, scale)
                proj(att, lw.o_w, ks_o)
                keep = [x[j * S:j * S + nm].clone() for j in range(k)] if nm > 0 else None
                hip.rmsnorm(x, lw.ln2_w, cfg.rms_eps, out=y)
                hip.gemm(y, lw.gateup_w, act=hip.ACT_SWIGLU, out=act)
                proj(act, lw.down_w, ks_down)
                if keep is not None:              # rows before the image: MLP contribution zeroed (TF:...:697-699)
                    for j in range(k):
                        x[j * S:j * S + nm].copy_(keep[j])
                ci += 1
            else:
                hip.rmsnorm(x, lw.ln1_w, cfg.rms_eps, out=y)
                if ks_qkv >= 2:
                    hip.gemm_splitk(y, lw.qkv_w, swork, ks_qkv, out=qkv)
                else:
                    hip.gemm(y, lw.qkv_w, out=qkv)
                if many:           # the group's requests as ONE launch each (per request bit-identical; see Qwen2VLEngine._prefill_group)
                    kv_off = [it[0] * self.kcache_b.stride(0) + si * self.kcache_b.stride(1) for it in items]
                    hip.qkv_rope_split_many(qkv, cos, sin, q, self.kcache_b, self.vcache_b, vt, Hq, Hkv, D, kv_off, Tc, k_pos0=0)
                    hip.attn_prefill_pairs_many(q, self.kcache_b, vt, att, work, scale, kv_off, Tc)
                else:
                    for j, (slot, _, _, _) in enumerate(items):
                        rows = slice(j * S, (j + 1) * S)
                        kc, vc = self.kcache_b[slot][si], self.vcache_b[slot][si]
                        hip.qkv_rope_split(qkv[rows], cos, sin, q[j], kc, vc, vt[j], Hq, Hkv, D, k_pos0=0)
                        hip.attn_prefill_pairs(q[j], kc, vt[j], att[rows], work, scale)
                proj(att, lw.o_w, ks_o)
                hip.rmsnorm(x, lw.ln2_w, cfg.rms_eps, out=y)
                hip.gemm(y, lw.gateup_w, act=hip.ACT_SWIGLU, out=act)
                proj(act, lw.down_w, ks_down)
                si += 1
            if taps is not None:
                taps[f"layer{li}"] = x.clone()
        if has_image and self.cross_kv == "fp8":
            for slot, _, _, _ in items:
                self._quantize_cross_kv(slot)
        grouped = many and k <= 4 and H * 2 * (2 if k <= 2 else 4) <= 152 * 1024   # one pass over the lm_head for the group's last rows
        if grouped:
            lg = torch.empty((k, self.logits_b.shape[1]), dtype=torch.float32, device=dev)
            hip.gemv_rows(x[S - 1::S], w.lm_head, lg, norm_w=w.norm_w, eps=cfg.rms_eps)
        for j, (slot, _, _, _) in enumerate(items):
            logits = self.logits_b[slot]
            if grouped:
                logits.copy_(lg[j])
            else:
                hip.gemv(x[(j + 1) * S - 1], w.lm_head, logits, norm_w=w.norm_w, eps=cfg.rms_eps)
            if taps is not None:
                taps["first_logits"] = logits.clone()
            self.step_b[slot:slot + 1].fill_(S - 1)
            self._prompt_pick(slot, ids_devs[j], logits, self.tokens_b[slot], self.cur_b[slot:slot + 1], self.step_b[slot:slot + 1])
            self.slot_prompt_len[slot] = S
            if slot == 0:
                self.has_image = has_image
                self.prompt_len, self._decoded = S, 0
                self.decode_limit = self.max_ctx

    # ------------------------------------------------------------------ decode
    def _decode_rope(self, B: int) -> tuple:
        """Plain positions: the one rope table for every sequence (batch stride 0), no shared keys (DecodeStage hook)."""
        return self.cos_t.unsqueeze(0).expand(B, -1, -1), self.sin_t.unsqueeze(0).expand(B, -1, -1), 0

    def _decode_cross_attn(self, L, q: torch.Tensor, att: torch.Tensor, B: int) -> None:
        """Attention of the new token(s) over the image's static keys / values of cross layer ``L`` (DecodeStage hook)."""
        cfg = self.cfg
        if self.cross_kv == "fp8":      # the e4m3 copy the prompt pass left (csrc/cross_attn.hip)
            if B:
                fn, nkeys = hip.decode_cross_attn_fp8_batch, self.nkeys_b[:B]
                kv = (self.xkq_b[:B, L.idx], self.xks_b[:B, L.idx], self.xvq_b[:B, L.idx], self.xvs_b[:B, L.idx])
            else:
                fn, nkeys = hip.decode_cross_attn_fp8, self.nkeys_m1
                kv = (self.xkq_b[0, L.idx], self.xks_b[0, L.idx], self.xvq_b[0, L.idx], self.xvs_b[0, L.idx])
        elif B:
            fn, kv, nkeys = hip.decode_cross_attn_batch, (self.xk_b[:B, L.idx], self.xv_b[:B, L.idx]), self.nkeys_b[:B]
        else:
            fn, kv, nkeys = hip.decode_cross_attn, (self.xk[L.idx], self.xv[L.idx]), self.nkeys_m1
        fn(q, L.w.q_norm, *kv, nkeys, self.part_o, self.part_ml, att, cfg.heads, cfg.kv_heads, cfg.head_dim, self.xsplit,
           cfg.head_dim ** -0.5, cfg.rms_eps)

    def _decode_cross_attn_draft(self, L, q: torch.Tensor, att: torch.Tensor, R: int) -> None:
        """The R rows of a speculative step over the image's static keys / values of cross layer ``L``: one pass over K / V for
        all rows, row r bit-identical to ``_decode_cross_attn`` on row r (DecodeStage hook)."""
        cfg, sp = self.cfg, self._spec
        if self.cross_kv == "fp8":
            fn = hip.decode_cross_attn_fp8_draft
            kv = (self.xkq_b[0, L.idx], self.xks_b[0, L.idx], self.xvq_b[0, L.idx], self.xvs_b[0, L.idx])
        else:
            fn, kv = hip.decode_cross_attn_draft, (self.xk[L.idx], self.xv[L.idx])
        fn(q, L.w.q_norm, *kv, self.nkeys_m1, sp.part_o, sp.part_ml, att[:R], cfg.heads, cfg.kv_heads, cfg.head_dim,
           self.xsplit, cfg.head_dim ** -0.5, cfg.rms_eps)

    def _ensure_graph(self, chained: bool = False) -> torch.cuda.CUDAGraph:
        chained = chained and self.chain_sync is not None
        key = (self.temperature, self.seed, self.has_image, chained) + self._pick_key() + self._stop_key() + self._shape_key() + self._stream_key() + self._ban_key()
        return self._captured_step(self._graphs, 6, key, 0, chained)

    def _batch_graph(self, B: int) -> torch.cuda.CUDAGraph:
        """The captured batched step (Generation hook)."""
        key = (self.temperature, self.seed, B, self.fork_on) + self._pick_key() + self._stop_key() + self._shape_key() + self._stream_key() + self._ban_key()
        return self._captured_step(self._graphs_b, 4, key, B, False)

    def decode(self, n_steps: int, use_graph: bool = True) -> None:
        if self.prompt_len + self._decoded + n_steps >= self.decode_limit:
            raise ValueError("decode would run past the context window")
        self._decode_ordered(n_steps, use_graph)

    # ------------------------------------------------------------------ generation (the loops: generation.Generation)
    keep_eos = True                      # a reply that ended on EOS keeps its EOS token here, with or without stop strings
    lazy_single_owns_failure = True      # one lazy request: whatever fails in it, its prompt pass too, stays its own
    single_route_check_every = 32        # generate_batch with one request runs generate at ITS default chunk

    def _prompt_pass(self, input_ids, frame, max_new_tokens, temperature, seed) -> None:
        """The single sequence's prompt pass; it prepares no rope rows, so the reply's length is not its concern
        (Generation hook)."""
        self.prefill(input_ids, frame, temperature=temperature, seed=seed)

    def _check_batch(self, requests: Sequence) -> None:
        """The batched step always runs the cross-attention layers (Generation hook)."""
        if not any(callable(r) for r in requests) and any(fr is None for _, fr in requests):
            raise ValueError("generate_batch needs an image in every request (text-only prompts go through generate)")

    def generate(self, input_ids: Sequence[int], frame: Optional[torch.Tensor] = None, max_new_tokens: int = 128,
                 temperature: float = 0.0, seed: int = 0, stop_on_eos: bool = True, use_graph: bool = True,
                 chunk: int = 32, **switches) -> List[int]:
        """One request through the single-sequence loop (Generation._generate), with ``stop_on_eos`` = not ignore_eos,
        ``chunk`` = check_every (the boundary at which a cancelled request ends) and ``frame`` the request's one image or
        None; ``switches``: the keywords request.Switches describes.  A reply that ended on EOS keeps its EOS token here; a
        ``max_new_tokens`` the context cannot hold is clamped silently; after a stalled chained launch this engine stays on
        the separate launches for good.  A speculative request or a prediction needs an engine built with speculative=True
        (else ValueError: by default they are the Qwen2-VL engines'); the reply is then the plain reply, EOS token included."""
        return self._generate(input_ids, frame, max_new_tokens, not stop_on_eos, use_graph, chunk, temperature, seed,
                              Switches.single(**switches))

    def generate_batch(self, requests: Sequence, max_new_tokens: int = 128, temperature: float = 0.0, seed: int = 0,
                       stop_on_eos: bool = True, use_graph: bool = True, chunk: int = 16, **switches) -> list:
        """Up to max_batch requests through one shared decode loop (Generation._generate_batch; ``stop_on_eos`` / ``chunk`` as
        in generate, ``switches``: the keywords request.Switches describes; a prediction other than None is refused).
        requests: [(input_ids, frame)]; every request of a batch carries an image - one text-only request alone takes the
        single-sequence path.  A reply that ended on EOS keeps its EOS token.  With several choices per request, the image's
        cross-attention keys / values are copied whole into every further choice's slot and the forked attention serves the
        self-attention layers."""
        return self._generate_batch(requests, max_new_tokens, not stop_on_eos, use_graph, chunk, temperature, seed,
                                    Switches.group(**switches))

    def _fork_model_state(self, root: int, child: int) -> None:
        """A further choice attends to its root's image: the cross-attention keys / values, whole (DecodeStage hook)."""
        self.xk_b[child].copy_(self.xk_b[root])
        self.xv_b[child].copy_(self.xv_b[root])
        if self.cross_kv == "fp8":
            for t in (self.xkq_b, self.xvq_b, self.xks_b, self.xvs_b):
                t[child].copy_(t[root])
        self.nkeys_b[child:child + 1].copy_(self.nkeys_b[root:root + 1])

    def prefill_many(self, requests: Sequence, temperature: float = 0.0, seed: int = 0, max_new_tokens: Optional[int] = None,
                     seeds: Optional[Sequence[int]] = None, penalties: Optional[Sequence[tuple]] = None,
                     shaping: Optional[Sequence[tuple]] = None,
                     ban: Optional[Sequence[tuple]] = None) -> Tuple[List[Optional[int]], List[Optional[Exception]]]:
        """The prompt passes of a batch into consecutive slots (Generation hook, the contract of
        Qwen2VLEngine.prefill_many): requests [(input_ids, frame)] or zero-argument callables returning that pair (the batch
        seam: a callable waits for the image's host decode, so the prompt pass of image 0 runs while images 1.. are still
        being decoded).  With a callable among them a request that fails gets no slot and keeps its exception; without,
        the failure is raised.  ``seeds`` / ``penalties`` / ``shaping`` / ``ban``: request b's rows, read by the picks while the
        switch is on; ``max_new_tokens`` is not needed (no rope rows are prepared per request).  Returns with the current
        stream ordered after all passes: (slot of request b or None, exception of request b or None)."""
        n_req = len(requests)
        lazy = any(callable(r) for r in requests)
        slots: List[Optional[int]] = [None] * n_req
        errors: List[Optional[Exception]] = [None] * n_req
        B = 0
        # The prompt passes are independent kernel chains (own buffers, own cache slot): issued round-robin on two HIP
        # streams (VIS_PREFILL_STREAMS, as in Qwen2VLEngine.prefill_many) the ragged last round of one image's GEMM /
        # attention grids - the 6432-row tower is 1-1.5 rounds of the chip per projection - is filled by the other's.
        n_streams = max(1, min(n_req, int(os.environ.get("VIS_PREFILL_STREAMS", "2"))))
        cur = torch.cuda.current_stream(self.device)
        if n_streams > 1 and len(self._prefill_streams) < n_streams:
            self._prefill_streams = [torch.cuda.Stream(device=self.device) for _ in range(n_streams)]
        vb = max(1, int(os.environ.get("VIS_VIT_BATCH", "4"))) if n_streams > 1 else 1

        def place(slot, b):      # request b's switch rows into its slot, before its prompt pass picks the first token
            for name, rows in (("_slot_seed", seeds), ("_slot_pen", penalties), ("_slot_shape", shaping), ("_slot_ban", ban)):
                if rows is not None:
                    getattr(self, name)[slot] = rows[b]

        for g0 in range(0, n_req, vb):
            grp = []                                     # (request index, ids, frame) of the requests that resolved
            for b in range(g0, min(n_req, g0 + vb)):
                r = requests[b]
                try:
                    ids, fr = r() if callable(r) else r
                    if fr is None:
                        raise ValueError("generate_batch needs an image in every request")
                    grp.append((b, ids, fr))
                except Exception as e:      # noqa: BLE001 - a lazy request's failure stays its own
                    if not lazy:
                        raise
                    errors[b] = e
            if not grp:
                continue
            try:      # the tower once over the group's images (whole rounds of the chip), on the current stream
                crosses = self.vision_forward_many([fr for _, _, fr in grp]) if len(grp) > 1 else [None] * len(grp)
            except Exception as e:      # noqa: BLE001
                if not lazy:
                    raise
                for b, _, _ in grp:
                    errors[b] = e
                continue
            # requests with one prompt layout (the Auditor's fixed prompt): ONE stacked text pass (VIS_MERGE_PREFILL=0: A/B)
            stack = len(grp) > 1 and n_streams > 1 and os.environ.get("VIS_MERGE_PREFILL", "1") != "0"
            if stack:
                l0 = [i for i, t in enumerate(grp[0][1]) if t == self.cfg.image_token_id]
                stack = all(len(ids) == len(grp[0][1]) and
                            [i for i, t in enumerate(ids) if t == self.cfg.image_token_id] == l0 for _, ids, _ in grp) and len(l0) == 1
            if stack:
                st = self._prefill_streams[(g0 // vb) % n_streams]      # consecutive groups alternate streams
                st.wait_stream(cur)
                try:
                    with torch.cuda.stream(st):
                        items = []
                        for (b, ids, fr), cs in zip(grp, crosses):
                            cs[0].record_stream(st)
                            place(B + len(items), b)
                            items.append((B + len(items), ids, cs[0], cs[1]))
                        self._prefill_group(items, temperature, seed)
                    for (b, _, _) in grp:
                        slots[b] = B
                        B += 1
                except Exception as e:      # noqa: BLE001
                    if not lazy:
                        raise
                    for b, _, _ in grp:
                        errors[b] = e
                continue
            for (b, ids, fr), cs in zip(grp, crosses):
                place(B, b)
                try:
                    if n_streams > 1:
                        st = self._prefill_streams[B % n_streams]
                        st.wait_stream(cur)          # the frame's upload / JPEG kernels and the group's tower ran on `cur`
                        with torch.cuda.stream(st):
                            fr.record_stream(st)
                            if cs is not None:
                                cs[0].record_stream(st)
                            self.prefill(ids, fr, temperature=temperature, seed=seed, slot=B, cross_states=cs)
                    else:
                        self.prefill(ids, fr, temperature=temperature, seed=seed, slot=B, cross_states=cs)
                except Exception as e:      # noqa: BLE001
                    if not lazy:
                        raise
                    errors[b] = e
                    continue
                slots[b] = B
                B += 1
        if n_streams > 1:
            for st in self._prefill_streams[:n_streams]:
                cur.wait_stream(st)
        return slots, errors
