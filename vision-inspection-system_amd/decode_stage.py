"""The decode stage of both engines: one token for the single sequence or for B in-flight sequences, the graph that replays
it, and the ordered chained decode of a device.  Which launches make a step, and in which form every projection is issued,
is decided here and nowhere else; both engines derive from ``DecodeStage`` (through ``generation.Generation``, which drives
a request through these steps) and describe their layers to it once."""
from __future__ import annotations

import logging
import os
import threading
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import hip, spec
from .fork import check_fork_tables, fork_layout
from .pick import PickStage
from .weights import pad_cols

_LOG = logging.getLogger("vision_inspection_system_amd.engine")

# the last chained decode call enqueued per device (DecodeStage._decode_ordered orders such calls on the GPU); one lock per
# device: engines on different GPUs driven from different threads do not serialise their host launch loops
_CHAIN_LOCKS_GUARD = threading.Lock()
_CHAIN_ORDER_LOCKS: Dict[Optional[int], threading.Lock] = {}
_CHAIN_LAST: Dict[Optional[int], "torch.cuda.Event"] = {}


def _chain_order_lock(index: Optional[int]) -> threading.Lock:
    with _CHAIN_LOCKS_GUARD:
        return _CHAIN_ORDER_LOCKS.setdefault(index, threading.Lock())


class DecodeLayer(NamedTuple):
    """One transformer layer as the decode stage sees it."""
    w: object                        # qkv_w, o_w, gateup_w, down_w, ln1_w, ln2_w (a cross-attention layer: q_norm too)
    q8: Optional[dict]               # name -> (e4m3 codes, row scales), "down_w_pad" where K was padded; None: not quantised
    q4: Optional[dict]               # name -> (MXFP4 codes, block scales); None: not quantised
    cross: bool                      # cross-attention over the image's static keys instead of self-attention
    idx: int                         # the layer's index into the self KV cache, or into the cross KV cache
    bias: Optional[torch.Tensor]     # qkv bias


_GEMV = {"bf16": "gemv", "fp8": "gemv_fp8", "mxfp4": "gemv_mxfp4"}      # hip's fused GEMV per weight format; + "_rows": 2..4 rows


def _wt(L: DecodeLayer, name: str, fmt: str) -> tuple:
    """The weight operands of one projection in one format: (w,), (codes, row scales) or (codes, block scales)."""
    return (getattr(L.w, name),) if fmt == "bf16" else (L.q8 if fmt == "fp8" else L.q4)[name]


def quantize_decode_weights(layer_weights: Sequence, lm_head: torch.Tensor, fp8: bool, mxfp4: bool,
                            pad_down: bool = False) -> tuple:
    """The decode projections of every layer and the lm_head in the quantised formats asked for, once at load time ->
    (q8, q4, q8_head, q4_head): a dict per layer over qkv_w / o_w / gateup_w / down_w, name -> (e4m3 codes, row scales) /
    (MXFP4 codes, block scales), and the lm_head's pair; a format that is off gives an empty list and None.  ``pad_down``:
    the fp8 MFMA reads down_w (``kpad`` is set) and needs K % 128 == 0 - where K is no such multiple, "down_w_pad" holds the
    codes with zero columns appended, under the unpadded tensor's scales."""
    names = ("qkv_w", "o_w", "gateup_w", "down_w")
    q8 = [{n: hip.quantize_fp8_rows(getattr(lw, n)) for n in names} for lw in layer_weights] if fp8 else []
    q4 = [{n: hip.quantize_mxfp4_rows(getattr(lw, n)) for n in names} for lw in layer_weights] if mxfp4 else []
    for q in q8 if pad_down else ():
        wq, sc = q["down_w"]
        if wq.shape[1] % 128:
            q["down_w_pad"] = (pad_cols(wq, 128), sc)
    return q8, q4, hip.quantize_fp8_rows(lm_head) if fp8 else None, hip.quantize_mxfp4_rows(lm_head) if mxfp4 else None


class DecodeStage(PickStage):
    """Base class of the engines: works on ``self``, holds no model knowledge.

    Contract - what an engine brings before ``_init_decode_state()`` runs: ``cfg``, ``device`` and ``max_ctx`` (a multiple of
    64); and before the first step: ``w.embed``, the rope tables ``cos_t`` / ``sin_t`` of the single sequence, its layers
    (``_init_decode_stage``), ``has_image`` where a layer is a cross-attention layer.  Everything else a step reads - caches,
    counters, activation rows, workspaces, the chain state and the flags - ``_init_decode_state()`` allocates and sets.
    What the models do differently is behind two hooks: ``_decode_rope(B)`` -> (cos, sin, shared_len), the rope tables
    [B, T, D] of the batched self-attention and the number of leading keys every sequence reads from slot 0, and
    ``_decode_cross_attn(L, q, att, B)``, the cross-attention launch of layer L for the single sequence (B == 0) or B slots.
    An engine with cross-attention layers that offers speculative decoding (``speculative_supported``) also supplies
    ``_decode_cross_attn_draft(L, q, att, R)``, that launch for the R rows of a speculative step, and ``xsplit``, its split count.
    An engine supplies ``_ensure_graph(chained=)`` with its own graph key (see ``_captured_step``) and checks its own bounds
    in ``decode()`` before ``_decode_ordered``."""

    # Speculative decoding of a batch (spec_batch.py), an engine setting: the SpecConfig an engine was built with
    # (Qwen2VLEngine(batch_speculative=)), stored on the instance only when given; the step's buffers and graphs, on first use.
    batch_speculative: Optional["spec.SpecConfig"] = None
    _spec_batch = None

    @staticmethod
    def check_decode_weights(cfg, decode_weights: str) -> None:
        """Refuse an unknown decode precision, or one the model's shapes do not fit (needs no GPU)."""
        if decode_weights not in ("bf16", "fp8", "mxfp4"):
            raise ValueError("decode_weights must be 'bf16', 'fp8' or 'mxfp4'")
        if decode_weights == "mxfp4":
            dims = {"hidden": cfg.hidden, "heads*head_dim": cfg.heads * cfg.head_dim, "intermediate": cfg.intermediate}
            bad = [f"{n}={v}" for n, v in dims.items() if v % 32]
            if bad:
                raise ValueError("decode_weights='mxfp4' needs MX blocks of 32 inputs: " + ", ".join(bad)
                                 + " must be multiples of 32")

    @staticmethod
    def check_mxfp4_gemm_from(cfg, decode_weights: str, mxfp4_gemm_from) -> None:
        """Refuse a threshold for the MXFP4 MFMA projection that is no integer in 5..64, that comes without
        decode_weights='mxfp4', or that the model's shapes do not fit (needs no GPU)."""
        if mxfp4_gemm_from is None:
            return
        if isinstance(mxfp4_gemm_from, bool) or not isinstance(mxfp4_gemm_from, int) or not 5 <= mxfp4_gemm_from <= 64:
            raise ValueError("mxfp4_gemm_from must be None or an integer in 5..64 (smaller batches are the multi-row GEMV's)")
        if decode_weights != "mxfp4":
            raise ValueError("mxfp4_gemm_from needs decode_weights='mxfp4'")
        dims = {"hidden": cfg.hidden, "heads*head_dim": cfg.heads * cfg.head_dim, "intermediate": cfg.intermediate}
        bad = [f"{n}={v}" for n, v in dims.items() if v % 64]
        if bad:
            raise ValueError("mxfp4_gemm_from needs K-steps of 64 inputs: " + ", ".join(bad) + " must be multiples of 64")

    def _init_decode_state(self, max_batch: int, n_self_layers: int, decode_weights: str = "bf16",
                           mxfp4_gemm_from: Optional[int] = None, decode_splits: int = 0, cross_splits: int = 0,
                           fused_quantised: bool = True, prefill_fp8: bool = False) -> None:
        """Everything a decode step works on that is not model knowledge, allocated and set once from an engine's constructor
        (``cfg``, ``device`` and ``max_ctx`` are set): the per-slot state - self KV caches of ``n_self_layers`` layers, counters,
        token rows, the pick's rows, each with its slot-0 view, slot 0 doubling as the single sequence - the single-sequence
        and the batched activation rows, the attention workspace for the larger of ``nsplit`` (``decode_splits``, or one
        split per hip.DECODE_KEYS_PER_SPLIT keys of context) and ``cross_splits``, what the fused and the fp8 batched steps
        add, the chain state, the flags every step reads (plain attributes: tests and tools set them afterwards) and the
        request counters.  Rows that rely on their pad columns, pad scale blocks or first read being zero are zeroed; the
        rest is uninitialised.  What does not apply is None (``kpad``, ``chain_ws``, ``chain_sync``) or, for the ``b_*`` rows,
        absent.

        ``fused_quantised``: whether VIS_DECODE_FUSED=1 holds whatever ``decode_weights`` is (Qwen2-VL: its fused step carries
        fp8 weights too) or for bf16 weights only (Mllama: a quantised engine's batched step is the stream-K or the rows step).
        ``prefill_fp8``: ``kpad`` is wanted although the batched fp8 step may be off, for an fp8 prompt pass.

        The one rule of ``b_part``, the stream-K partial slabs (16 slots x hip.part_rows(max_batch) rows x the widest
        projection), kept as ``streamk_part``: allocated when a step can read them - max_batch > 1, and not the fused step
        with fp8 weights (every projection of it is one launch), and not MXFP4 weights without ``mxfp4_gemm_from`` (every
        batch size is the rows step's); absent otherwise.  Readers: the stream-K step, and the fused step's long-K bf16 down
        projection at many sequences."""
        cfg, dev, bf = self.cfg, self.device, torch.bfloat16
        Hq, Hkv, D, H, I = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.hidden, cfg.intermediate
        if not 1 <= max_batch <= 64:
            raise ValueError("max_batch must be in 1..64 (one, two or four 16-row MFMA blocks of in-flight sequences)")
        Bm = self.max_batch = max_batch
        self.decode_weights, self.mxfp4_gemm_from = decode_weights, mxfp4_gemm_from
        self.nsplit = decode_splits or max(1, -(-self.max_ctx // hip.DECODE_KEYS_PER_SPLIT))
        # decode-step state is device resident, so the step is one replayable graph
        self.kcache_b = torch.zeros((Bm, n_self_layers, Hkv, self.max_ctx, D), dtype=bf, device=dev)
        self.vcache_b = torch.zeros((Bm, n_self_layers, Hkv, self.max_ctx, D), dtype=bf, device=dev)
        self.step_b = torch.zeros(Bm, dtype=torch.int32, device=dev)
        self.cur_b = torch.zeros(Bm, dtype=torch.int32, device=dev)
        self.tokens_b = torch.zeros((Bm, self.max_ctx), dtype=torch.int32, device=dev)
        self.ws_val = torch.empty(max(256 * Bm, 2048), dtype=torch.float32, device=dev)
        self.ws_idx = torch.empty(max(256 * Bm, 2048), dtype=torch.int32, device=dev)
        self.logits_b = torch.empty((Bm, cfg.vocab), dtype=torch.float32, device=dev)
        self.kcache, self.vcache = self.kcache_b[0], self.vcache_b[0]
        self.step, self.cur_token = self.step_b[0:1], self.cur_b[0:1]
        self.tokens, self.logits = self.tokens_b[0], self.logits_b[0]
        nq = (Hq + 2 * Hkv) * D
        self.d_x = torch.empty((1, H), dtype=bf, device=dev)
        self.d_x2 = torch.empty((1, H), dtype=bf, device=dev)
        self.d_qkv = torch.empty(nq, dtype=bf, device=dev)
        self.d_attn = torch.empty(Hq * D, dtype=bf, device=dev)
        self.d_act = torch.empty(I, dtype=bf, device=dev)
        ns = max(self.nsplit, cross_splits)
        self.part_o = torch.empty(Bm * Hq * ns * D, dtype=torch.float32, device=dev)
        self.part_ml = torch.empty(Bm * Hq * ns * 2, dtype=torch.float32, device=dev)
        if Bm > 1:      # batched-decode activations
            for name, cols in (("b_x", H), ("b_x2", H), ("b_qkv", nq), ("b_attn", Hq * D), ("b_act", I), ("b_xn", H),
                               ("b_xn2", H)):
                setattr(self, name, torch.empty((Bm, cols), dtype=bf, device=dev))
        # Batched decode, r05 experiment (VIS_DECODE_FUSED=1, OFF by default): every projection as ONE launch - stream + split-K
        # reduction + epilogue (vis_decode_proj_*: stream-K ranges with a last-arriver reduction, or whole-K column slabs), the
        # RMSNorm split into the producer's per-column and the consumer's per-row factor; csrc/decode_stream.hip,
        # csrc/decode_colpar.hip.  Correct and tested, but NOT faster: a cross-CU reduction costs three dependent memory round
        # trips wherever it runs, and the finalisation launch it replaces already sits at the ~5 us floor of a dependent
        # load -> store kernel (profiles/r05_decode_step_*.txt: 64 sequences 5.37 -> 6.4 ms per step).
        self.fused_proj = Bm > 1 and H % 128 == 0 and (fused_quantised or decode_weights == "bf16") \
            and os.environ.get("VIS_DECODE_FUSED", "0") == "1"
        # batched decode: the self-attention launch finalises the qkv projection's partial slabs itself (vis_decode_attn_parts,
        # bit-identical to skinny_finalize + decode_attn); VIS_QKV_FOLD=0 keeps the two launches (A/B)
        self.fold_qkv = os.environ.get("VIS_QKV_FOLD", "1") == "1"
        self.streamk_part = Bm > 1 and not (self.fused_proj and decode_weights == "fp8") and \
            (decode_weights != "mxfp4" or mxfp4_gemm_from is not None)
        if self.streamk_part:
            self.b_part = torch.empty(16 * hip.part_rows(Bm) * max(nq, H, 2 * I), dtype=torch.float32, device=dev)
        # the batched fp8 step carries its activations as e4m3 rows too; the fp8 MFMA needs K % 128 == 0, so the down
        # projection's input rows (and its weights: quantize_decode_weights) are zero-padded to kpad columns
        self.fp8_batched = decode_weights == "fp8" and Bm > 1 and H % 128 == 0
        self.kpad = (I + 127) // 128 * 128 if self.fp8_batched or prefill_fp8 else None
        if self.fp8_batched:
            self.b_xq = torch.zeros((Bm, H), dtype=torch.uint8, device=dev)
            self.b_x2q = torch.zeros((Bm, H), dtype=torch.uint8, device=dev)
            self.b_actq = torch.zeros((Bm, self.kpad), dtype=torch.uint8, device=dev)       # pad columns stay 0
            self.b_sx = torch.zeros((3, Bm), dtype=torch.float32, device=dev)
            if self.fused_proj:   # MX blocks: one E8M0 scale byte per row and 32 columns (pad blocks stay 0 = 2^-127 x code 0)
                self.b_xqs = torch.zeros((Bm, H // 32), dtype=torch.uint8, device=dev)
                self.b_x2qs = torch.zeros((Bm, H // 32), dtype=torch.uint8, device=dev)
                self.b_actqs = torch.zeros((Bm, self.kpad // 32), dtype=torch.uint8, device=dev)
        if self.fused_proj:
            self.b_xw = torch.empty((Bm, H), dtype=bf, device=dev)        # x * ln1_w of the next layer (A operand of qkv / lm_head)
            self.b_x2w = torch.empty((Bm, H), dtype=bf, device=dev)       # x2 * ln2_w (A operand of gate/up)
            self.b_ssq1 = torch.zeros((H // hip.SSQ_UNIT, hip.SSQ_LD), dtype=torch.float32, device=dev)
            self.b_ssq2 = torch.zeros((H // hip.SSQ_UNIT, hip.SSQ_LD), dtype=torch.float32, device=dev)
            f8 = self.fp8_batched
            shapes = [(nq, H, f8), (H, Hq * D, False), (2 * I, H, f8), (H, self.kpad if f8 else I, f8), (cfg.vocab, H, f8)]
            need = max(int(hip.load().vis_decode_proj_ws_bytes(Bm, n, k, int(q))) for n, k, q in shapes)
            if need <= 0:
                raise ValueError("vis_decode_proj_ws_bytes refused a projection shape of this model")
            self.b_proj_ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        # Single-sequence decode: the head of every self-attention layer (qkv projection -> rope / append / attention -> o
        # projection) as ONE launch whose stages hand over inside the grid, the lm_head with the pick's first stage in its
        # epilogue (csrc/decode_chain.hip, _decode_step_rows; bit-identical to the launches it replaces); bf16 weights only.
        # Contexts up to chain_ctx_limit cached keys decode on it, longer ones on the four launches (same bits): what must be
        # resident together are the workgroups that wait - projection and merge roles + Hkv attention items per 64 keys of
        # context (7B shapes: 6208 keys, 11B: 1536, whatever the cache size is).  VIS_DECODE_CHAIN=0 keeps the four launches (A/B).
        self.chain_ws = self.chain_sync = None
        self.chain_ctx_limit = 0
        self._chain_launches = 0                       # host-side count of chained launches on the sync block (epoch guard)
        if decode_weights == "bf16" and os.environ.get("VIS_DECODE_CHAIN", "1") != "0" \
                and hip.decode_chain_supported(Hq, Hkv, D, H):
            limit = hip.decode_chain_ctx_limit(Hq, Hkv, H)
            if limit > 0:
                self.chain_ws, self.chain_sync = hip.decode_chain_state(dev, Hq, Hkv, self.nsplit)
                self.chain_ctx_limit = limit
        self.slot_prompt_len = [0] * Bm
        self.prompt_len = self._decoded = self.decode_limit = 0
        self.temperature, self.seed = 0.0, 0
        self.last_timing: dict = {}
        self._prefill_streams: List[torch.cuda.Stream] = []

    def _init_decode_stage(self, layers: Sequence[DecodeLayer], norm_w: torch.Tensor, lm_head: torch.Tensor,
                           q8_head: Optional[tuple] = None, q4_head: Optional[tuple] = None) -> None:
        """The model, described once: its layers in order, the final norm, the lm_head in its formats."""
        self.dec_layers: List[DecodeLayer] = list(layers)
        self.dec_norm_w = norm_w
        self.dec_head = {"bf16": (lm_head,), "fp8": q8_head, "mxfp4": q4_head}
        self.dec_n_self = sum(1 for L in self.dec_layers if not L.cross)     # chained launches per step
        self._init_pick_stage()      # the request switches of the next-token pick (pick.py)
        # several choices per request (generate_batch(.., n=)): while a batch has children, every batched self-attention launch
        # is the forked one and reads these two device tables (one row per slot; a graph captured once serves every layout)
        self.fork_on = False
        self.fork_parent_b: Optional[torch.Tensor] = None
        self.fork_len_b: Optional[torch.Tensor] = None
        # speculative decoding of the single sequence (generate(.., speculative=)): buffers and graphs on first use
        self._spec: Optional[spec.SpecBuffers] = None
        self._spec_cfg: Optional[spec.SpecConfig] = None
        self._spec_pred = False      # the request in flight came with a prediction: its steps end with vis_spec_draft_pred
        self._spec_graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}

    def _attn_share(self, B: int, shared: int) -> dict:
        """How the batched self-attention of B slots names the keys a slot reads from another slot's cache: the fork tables
        while the batch has children (the batch's text prefix is in them too), else the one shared length."""
        if self.fork_on:
            return dict(fork=(self.fork_parent_b[:B], self.fork_len_b[:B]))
        return dict(shared_len=shared)

    def _fork_model_state(self, root: int, child: int) -> None:
        """Hook: copy what the model keeps per slot besides the self KV cache (rope rows, cross-attention keys) from ``root``
        into ``child``."""

    def _fork_choices(self, roots: Sequence[Optional[int]], n: Sequence[int], prefix_len: int, seeds, penalties,
                      shaping) -> List[Optional[List[int]]]:
        """After the prompt passes of a batch (request j in slot roots[j], None = failed): give request j its n[j] - 1 further
        choices.  A child slot gets the rows of its root's prompt behind the fork length (at most 63, torch copies), the
        model's per-slot state, the root's last-row logits and then the SAME first pick a prompt pass ends with - a fresh
        grammar state, stop record and logprob row, the prompt's penalty flags, the request's shaping and ban parameters, its own
        seed (seeds[j] + i) - so every per-slot row is what a prompt pass of its own would have left.  Returns the slots of
        every request's choices and switches the forked attention on when there is a child."""
        live = [j for j in range(len(roots)) if roots[j] is not None]
        lay = fork_layout([self.slot_prompt_len[roots[j]] for j in live], [n[j] for j in live], prefix_len, self.max_batch)
        out: List[Optional[List[int]]] = [None] * len(roots)
        for i, j in enumerate(live):
            if roots[j] != i:
                raise RuntimeError("prompt passes did not fill consecutive slots")
            out[j] = lay.slots[i]
        for child, root, lo, hi in lay.copies:
            j = live[root]
            self.kcache_b[child][:, :, lo:hi].copy_(self.kcache_b[root][:, :, lo:hi])
            self.vcache_b[child][:, :, lo:hi].copy_(self.vcache_b[root][:, :, lo:hi])
            self._fork_model_state(root, child)
            self.logits_b[child].copy_(self.logits_b[root])
            self.step_b[child:child + 1].fill_(hi - 1)
            self.slot_prompt_len[child] = hi
            i = out[j].index(child)
            if seeds is not None:
                self._slot_seed[child] = seeds[j] + i
            if penalties is not None:
                self._slot_pen[child] = penalties[j]
            if shaping is not None:
                self._slot_shape[child] = shaping[j]
            if root in self._slot_ban:      # a further choice inherits its request's bans
                self._slot_ban[child] = self._slot_ban[root]
            self._prompt_pick(child, self._slot_ids[root], self.logits_b[child], self.tokens_b[child],
                              self.cur_b[child:child + 1], self.step_b[child:child + 1])
        if lay.copies:
            check_fork_tables(lay.parent, lay.fork_len, self.max_ctx, lay.holds)
            if self.fork_parent_b is None:
                self.fork_parent_b = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
                self.fork_len_b = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
            nb = len(lay.parent)
            self.fork_parent_b[:nb].copy_(torch.tensor(lay.parent, dtype=torch.int32))
            self.fork_len_b[:nb].copy_(torch.tensor(lay.fork_len, dtype=torch.int32))
            self.fork_on = True
        return out

    def _gather_choices(self, choice_slots: Sequence[Optional[List[int]]], errors: Sequence, outs_by_slot: Sequence[list],
                        starts: Sequence[int], eos, ignore_eos: bool, keep_eos: bool, nested: bool, mask_error) -> list:
        """After the run: cut every choice's tokens (``_finish``), record its logprobs, and shape the results per request - one
        token list (``nested`` False: one choice each, as without ``n``) or a list of them; ``last_finish`` and
        ``last_logprobs`` nest the same way.  A failed request's entry is its exception; a request with a choice the grammar
        mask could not continue gets ``mask_error()``."""
        flat = [s for cs in choice_slots if cs is not None for s in cs]
        cut = dict(zip(flat, self._finish([(s, outs_by_slot[s]) for s in flat], eos, ignore_eos, keep_eos=keep_eos)))
        fin = dict(zip(flat, self.last_finish))
        self._record_logprobs([(s, starts[s], len(cut[s])) for s in flat])
        lps = dict(zip(flat, self.last_logprobs)) if self.last_logprobs is not None else None
        failed = set(self._mask_failed(flat))
        outs, fins, lpo = [], [], []
        for j, cs in enumerate(choice_slots):
            if cs is None:
                outs.append(errors[j])
                fins.append(None)
                lpo.append(None)
                continue
            one = (lambda d: [d[s] for s in cs]) if nested else (lambda d: d[cs[0]])
            lpo.append(one(lps) if lps is not None else None)
            bad = bool(failed.intersection(cs))
            outs.append(mask_error() if bad else one(cut))
            fins.append(None if bad else one(fin))
        self.last_finish = fins
        if lps is not None:
            self.last_logprobs = lpo
        return outs

    # ------------------------------------------------------------------ steps whose projections write their finished rows
    def _decode_step(self, chained: Optional[bool] = None) -> None:
        """One token of the single sequence (slot 0): chained layer heads where asked for (default: where the engine has
        them), the fused GEMVs otherwise."""
        if chained is None:
            chained = self.chain_sync is not None
        self._decode_step_rows(0, chained and self.chain_sync is not None)

    def _decode_step_rows(self, B: int, chained: bool = False) -> None:
        """The step whose projections are fused GEMVs (norm / bias / residual / SwiGLU in the launch, no partial buffers, no
        finalisation launches).  B == 0: the single sequence; ``chained``: the head of every self-attention layer (qkv
        projection -> rope / append / attention -> o projection) as ONE launch (csrc/decode_chain.hip, bit-identical to the
        four it replaces), the first one reading the new token's embedding row itself, and the pick's first stage in the
        lm_head epilogue; a cross-attention layer is skipped while the request has no image.
        B >= 2, a couple of in-flight sequences: the multi-row GEMV (vis_gemv_*_rows) - one pass over the weights for all
        rows (the stream-K projection pays four finalisations per layer); bf16 or e4m3 weights with bf16 activations, every
        sequence bit-identical to decoding alone.  Chosen by _decode_step_batched (VIS_ROWS_GEMV).  MXFP4 weights take this
        step at EVERY batch size: more than 4 sequences issue each projection once per group of 4 rows (the weights are then
        read ceil(B / 4) times per step: slower than the bf16 stream-K step above ~16 sequences); attention, pick and the
        request switches stay one batched launch each."""
        cfg, fmt = self.cfg, self.decode_weights
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        scale, eps = D ** -0.5, cfg.rms_eps
        if B:
            x, x2, qkv, att, act = self.b_x[:B], self.b_x2[:B], self.b_qkv[:B], self.b_attn[:B], self.b_act[:B]
            cur, step, tokens, logits = self.cur_b[:B], self.step_b[:B], self.tokens_b[:B], self.logits_b[:B]
            cos, sin, shared = self._decode_rope(B)
        else:
            x, x2, qkv, att, act = self.d_x[0], self.d_x2[0], self.d_qkv, self.d_attn, self.d_act
            cur, step, tokens, logits = self.cur_token, self.step, self.tokens, self.logits
            cos, sin, shared = self.cos_t, self.sin_t, 0
        gemv, gemv_rows = getattr(hip, _GEMV[fmt]), getattr(hip, _GEMV[fmt] + "_rows")

        def proj(inp, wt, out, residual=None, **kw):
            if not B:
                gemv(inp, *wt, out, residual=residual, **kw)
            elif fmt == "mxfp4":
                for b0 in range(0, B, 4):
                    rows = slice(b0, min(b0 + 4, B))
                    gemv_rows(inp[rows], *wt, out[rows], residual=None if residual is None else residual[rows], **kw)
            else:
                gemv_rows(inp, *wt, out, residual=residual, **kw)

        if not (chained and not self.dec_layers[0].cross):     # else the first layer's launch reads the embedding row itself
            hip.gather_rows(self.w.embed, cur, self.d_x if not B else x)
        for li, L in enumerate(self.dec_layers):
            lw = L.w
            if L.cross:
                if not B and not self.has_image:
                    continue
                q = qkv[..., :Hq * D]
                proj(x, _wt(L, "qkv_w", fmt), q, norm_w=lw.ln1_w, eps=eps)
                self._decode_cross_attn(L, q, att, B)
                proj(att, _wt(L, "o_w", fmt), x2, residual=x)
            else:
                kc, vc = (self.kcache_b[:B, L.idx], self.vcache_b[:B, L.idx]) if B else (self.kcache[L.idx], self.vcache[L.idx])
                if chained:
                    try:   # layer 0 reads the new token's embedding row itself (x_index): no gather launch
                        hip.decode_chain(self.w.embed if li == 0 else x, lw.qkv_w, L.bias, lw.ln1_w, lw.o_w, x2, cos, sin, kc, vc,
                                         step, self.chain_ws, self.chain_sync, Hq, Hkv, D, self.nsplit, scale, eps,
                                         x_index=cur if li == 0 else None, ctx_bound=self.chain_ctx_limit)
                    except hip.ChainRefused as e:
                        # VIS_ERR_UNSUPPORTED and nothing else (a bad argument or a launch error propagates): the grid for
                        # this context length is larger than the device holds resident -> the four launches, same results;
                        # said once.  (Rare: the chain is kept only with a positive decode_chain_ctx_limit, and that bound
                        # is what the launch is given.)
                        if li:
                            raise
                        _LOG.warning("%s - decoding on the four launches per layer head (VIS_MAX_CTX=%d)", e, self.max_ctx)
                        self.chain_sync, self._chain_state, chained = None, None, False
                        hip.gather_rows(self.w.embed, cur, self.d_x)
                if not chained:
                    proj(x, _wt(L, "qkv_w", fmt), qkv, bias=L.bias, norm_w=lw.ln1_w, eps=eps)
                    hip.decode_attn(qkv, cos, sin, kc, vc, step, self.part_o, self.part_ml, att, Hq, Hkv, D, self.nsplit, scale,
                                    **(self._attn_share(B, shared) if B else {}))
                    proj(att, _wt(L, "o_w", fmt), x2, residual=x)
            proj(x2, _wt(L, "gateup_w", fmt), act, norm_w=lw.ln2_w, act=hip.ACT_SWIGLU, eps=eps)
            proj(act, _wt(L, "down_w", fmt), x, residual=x2)
        if chained:     # the pick's first stage rides in the lm_head epilogue
            self._gemv_pick(x, *self.dec_head["bf16"], logits, self.ws_val, self.ws_idx, tokens, cur, step,
                            norm_w=self.dec_norm_w, eps=eps, temperature=self.temperature, seed=self.seed)
        else:
            proj(x, self.dec_head[fmt], logits, norm_w=self.dec_norm_w, eps=eps)
            self._pick(logits, self.ws_val, self.ws_idx, tokens, cur, step, self.temperature, self.seed)
        self._logprobs_after_pick(B or 1)
        self._stop_after_pick(B or 1)
        self._stream_after_pick(B or 1)

    # ---- speculative decode of the single sequence (spec.py): 1..R tokens per weight pass
    def _spec_begin(self, cfg: "spec.SpecConfig", max_new_tokens: int,
                    prediction: Optional[Sequence[int]] = None) -> "spec.SpecBuffers":
        """Behind the prompt pass of a speculative request (its rope rows prepared for max_new_tokens + R - 1 further
        positions): the step's buffers take over the first token and the prompt's ids; ``limit`` is the index of the token
        row the reply's last token goes to, so the reply has exactly max_new_tokens tokens however a step's run ends.
        ``prediction`` (ids): uploaded, and the prediction drafter is issued once behind the prompt pass's pick, so the
        first step already carries drafts; every step of the request then ends with that drafter."""
        cross = self.dec_n_self != len(self.dec_layers)
        if cross and not self.speculative_supported:
            raise ValueError("speculative decoding is not supported on a model with cross-attention layers unless its engine "
                             "was built for it (MllamaEngine(.., speculative=True))")
        spec.check_rows_fit(self.cfg, cfg.rows)
        if cross:
            spec.check_cross_rows_fit(self.cfg, cfg.rows)
        if self._spec is None:      # one attention workspace serves the self and the cross launches: the larger split count
            self._spec = spec.SpecBuffers(self.cfg, max(self.nsplit, self.xsplit) if cross else self.nsplit, self.max_ctx,
                                          self.device)
        self._spec_cfg = cfg
        self._spec_pred = bool(prediction)
        start = self.prompt_len - 1
        self._spec.begin(self.cur_token, self._slot_ids[0], start, min(start + max_new_tokens - 1, self.max_ctx - 2),
                         prediction)
        if cfg.sampled:      # the row seed the prompt pass's pick just drew with (PickStage._seed_slot's choice for slot 0)
            self._spec.set_params(self.temperature, self._slot_seed.get(0, self.seed))
        if cfg.grammar:      # the prompt pass's pick was vis_schema_mask's; from here on the rows launch owns the DFA state
            if not self.schema_on:
                raise ValueError("speculative: 'grammar' needs a JSON Schema on the request (json_schema=)")
            self._schema.begin_rows(start, cfg.schema_drafts)
        if self._spec_pred:
            self._spec_draft_pred(cfg.k)
        if cfg.schema_drafts:
            self._schema.draft(self.tokens, self.step, cfg.k, self._spec.draft, self._spec.n_draft)
        return self._spec

    def _spec_draft_pred(self, k: int) -> None:
        sp, c = self._spec, self._spec_cfg
        hip.spec_draft_pred(sp.prompt, sp.prompt_len, self.tokens, sp.gen_start, self.step, k, c.lookup_max, c.lookup_min,
                            self.cfg.vocab, sp.pred, sp.pred_len, sp.pred_state, sp.draft, sp.n_draft)

    def _decode_step_spec(self, R: int, propose: bool = True) -> None:
        """One speculative step of the single sequence: rows [cur, draft 0 .. draft R-2] at positions step .. step + R - 1
        through the multi-row GEMVs (one pass over the weights, every row the single-row kernel's bits), the draft
        attention (row r = the plain launch at step + r, bit for bit; a cross-attention layer: the q projection into the
        leading columns of the packed rows and ``_decode_cross_attn_draft``, row r = the plain cross launch on row r, skipped
        while the request has no image as in the plain step), the lm_head into [R, V] f32, then vis_spec_accept -
        which keeps the drafts the picks confirm and advances ``step`` by 1..R (vis_spec_accept_sampled, the same with the
        sampled pick, when the request's configuration opted in; the only launch that differs) - and vis_spec_draft for the next step
        (vis_spec_draft_pred instead when the request came with a prediction).  A configuration with ``grammar``: vis_schema_mask_rows
        ahead of the accept, vis_spec_accept_masked in its place, and with ``schema_drafts`` vis_spec_draft_schema behind the drafter.
        Never the chained launch: the chain is bit-identical to the four launches, so the tokens are the chained step's.
        ``propose`` False leaves the draft row and its count alone (a test plants them)."""
        cfg, fmt, sp = self.cfg, self.decode_weights, self._spec
        Hq, Hkv, D = cfg.heads, cfg.kv_heads, cfg.head_dim
        scale, eps = D ** -0.5, cfg.rms_eps
        x, x2, qkv, att, act, logits = sp.x[:R], sp.x2[:R], sp.qkv[:R], sp.attn[:R], sp.act[:R], sp.logits[:R]
        gemv_rows = getattr(hip, _GEMV[fmt] + "_rows")
        hip.gather_rows(self.w.embed, sp.ids[:R], x)
        for L in self.dec_layers:
            lw = L.w
            if L.cross:
                if not self.has_image:
                    continue
                q = qkv[:, :Hq * D]
                gemv_rows(x, *_wt(L, "qkv_w", fmt), q, norm_w=lw.ln1_w, eps=eps)
                self._decode_cross_attn_draft(L, q, att, R)
            else:
                gemv_rows(x, *_wt(L, "qkv_w", fmt), qkv, bias=L.bias, norm_w=lw.ln1_w, eps=eps)
                hip.decode_attn_draft(qkv, self.cos_t, self.sin_t, self.kcache[L.idx], self.vcache[L.idx], self.step,
                                      sp.part_o, sp.part_ml, att, Hq, Hkv, D, self.nsplit, scale)
            gemv_rows(att, *_wt(L, "o_w", fmt), x2, residual=x)
            gemv_rows(x2, *_wt(L, "gateup_w", fmt), act, norm_w=lw.ln2_w, act=hip.ACT_SWIGLU, eps=eps)
            gemv_rows(act, *_wt(L, "down_w", fmt), x, residual=x2)
        gemv_rows(x, *self.dec_head[fmt], logits, norm_w=self.dec_norm_w, eps=eps)
        if self._spec_cfg.grammar:      # row r's pick under the schema's mask in front of row r: the plain masked pick at step + r
            allow = self._schema.mask_rows(self.tokens, self.step, sp.draft, sp.n_draft, R)
            hip.spec_accept_masked(logits, sp.draft, sp.n_draft, sp.limit, sp.ws_val, sp.ws_idx, self.tokens, sp.cur, self.step,
                                   sp.counters, allow, sp.params if self._spec_cfg.sampled else None)
        elif self._spec_cfg.sampled:      # row r's pick: the plain loop's sampled pick at step + r; 1 / T and the seed from params
            hip.spec_accept_sampled(logits, sp.draft, sp.n_draft, sp.limit, sp.ws_val, sp.ws_idx, self.tokens, sp.cur,
                                    self.step, sp.counters, sp.params)
        else:
            hip.spec_accept(logits, sp.draft, sp.n_draft, sp.limit, sp.ws_val, sp.ws_idx, self.tokens, sp.cur, self.step,
                            sp.counters)
        if propose and R > 1 and self._spec_pred:
            self._spec_draft_pred(R - 1)
        elif propose and R > 1:
            c = self._spec_cfg
            hip.spec_draft(sp.prompt, sp.prompt_len, self.tokens, sp.gen_start, self.step, R - 1, c.lookup_max, c.lookup_min,
                           cfg.vocab, sp.draft, sp.n_draft)
        if propose and R > 1 and self._spec_cfg.schema_drafts:      # the bytes the schema forces replace the lookup's drafts
            self._schema.draft(self.tokens, self.step, R - 1, sp.draft, sp.n_draft)

    def _decode_cross_attn_draft(self, L: DecodeLayer, q: torch.Tensor, att: torch.Tensor, R: int) -> None:
        """Hook: the cross-attention of layer L for the R rows q [R, Hq * D] (a column view of the packed rows) into att[:R],
        with the step's workspace ``self._spec.part_o`` / ``part_ml``; every row bit-identical to ``_decode_cross_attn`` alone."""
        raise NotImplementedError("this engine has no draft form of its cross-attention")

    def _spec_graph(self, R: int) -> torch.cuda.CUDAGraph:
        """The captured speculative step, keyed by (R, weight format, the lookup window, whether the cross-attention layers run,
        "pred" when the step ends with the prediction drafter, "sampled" when its accept is the sampled one, "grammar" /
        "schema_drafts" when the schema's launches are in it): its launches
        read everything else - the prediction, its length, the drafter's state, the inverse temperature and the seed - from
        device memory.  The warm-up step advances the request's counters; they are put back before the capture."""
        c = self._spec_cfg
        cross = (("image" if self.has_image else "text"),) if self.dec_n_self != len(self.dec_layers) else ()
        key = ("spec", R, self.decode_weights, c.lookup_max, c.lookup_min) + cross + (("pred",) if self._spec_pred else ()) + \
            (("sampled",) if c.sampled else ()) + (("grammar",) if c.grammar else ()) + \
            (("schema_drafts",) if c.schema_drafts else ())
        if key in self._spec_graphs:
            return self._spec_graphs[key]
        sp = self._spec
        saved = (self.step_b.clone(), sp.ids.clone(), sp._ints.clone())
        start = max(0, min(int(self.step.item()), self.tokens.numel() - R))      # the token row entries the warm-up may write
        row = self.tokens[start:start + R].clone()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._decode_step_spec(R)
        torch.cuda.current_stream().wait_stream(side)
        self.step_b.copy_(saved[0])
        sp.ids.copy_(saved[1])
        sp._ints.copy_(saved[2])
        self.tokens[start:start + R].copy_(row)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._decode_step_spec(R)
        if len(self._spec_graphs) >= 4:
            self._spec_graphs.pop(next(iter(self._spec_graphs)))
        self._spec_graphs[key] = g
        return g

    def _decode_steps_spec(self, n_steps: int, R: int, use_graph: bool) -> None:
        if use_graph:
            g = self._spec_graph(R)
            for _ in range(n_steps):
                g.replay()
        else:
            for _ in range(n_steps):
                self._decode_step_spec(R)

    # ---- batched decode: B in-flight sequences (slots 0..B-1) share every weight read of a step
    def _decode_step_batched(self, B: int) -> None:
        """Every projection = gemm_decode (weights streamed once for all B sequences, split-K f32 partials) +
        skinny_finalize (row-wise: sum, bias/residual/SwiGLU, and the RMSNorm of the NEXT projection); self-attention and
        cross-attention take the sequence index on the grid."""
        kind = self._batched_step_kind(B)
        if kind == "rows":
            self._decode_step_rows(B)
        elif kind == "fused":
            self._decode_step_fused(B)
        else:
            self._decode_step_streamk(B)

    def _batched_step_kind(self, B: int) -> str:
        """Which step B in-flight sequences take: "rows" (the multi-row GEMV), "fused" or "streamk"."""
        # VIS_ROWS_GEMV=<n> (default 0 = off): batches of 2..n (<= 4) sequences decode on the multi-row GEMV instead.  Measured
        # at exact 7B shapes (tools/probes/rows_ab.sh): 2 sequences 3.66 -> 3.20 ms per step (bf16), 2.83 -> 2.65 (e4m3
        # weights); at 3 and 4 the four-row kernel LOSES to the stream-K projection (4.2-4.3 vs 3.7-3.8 ms; fp8 3.8-4.0 vs
        # 2.9: four LDS reads + four dot products per weight chunk, one workgroup per CU on the down projection).  Off by
        # default because it trades an invariant for those 6-13 %: a sequence decoded in a batch of 2 would then follow the
        # single-sequence arithmetic and in a batch of 3+ the stream-K arithmetic - its tokens could depend on the batch size
        # at near-ties (tests/test_fullsize_gpu.py::test_7b_batch_invariance_and_reproducibility).  A model with
        # cross-attention layers ignores VIS_ROWS_GEMV; with MXFP4 weights it takes the multi-row step like any other (the
        # cross layer's q projection writes the leading columns of the packed row, a strided [B, Hq * D] view).
        if self.decode_weights == "mxfp4":
            # the multi-row GEMV at every batch size, unless mxfp4_gemm_from hands the larger ones to the MFMA projection
            # (the other arithmetic family, see Qwen2VLEngine.__init__)
            return "rows" if self.mxfp4_gemm_from is None or B < self.mxfp4_gemm_from else "streamk"
        rows_max = int(os.environ.get("VIS_ROWS_GEMV", "0")) if self.dec_n_self == len(self.dec_layers) else 0
        if 2 <= B <= min(rows_max, 4) and max(self.cfg.intermediate, self.cfg.hidden) * 2 * (2 if B <= 2 else 4) <= 152 * 1024:
            return "rows"
        return "fused" if self.fused_proj else "streamk"

    def _decode_step_streamk(self, B: int) -> None:
        """The stream-K batched step.  The first half of a projection writes partial slabs: hip.decode_gemm on the bf16
        weights, hip.decode_gemm_mxfp4 on the FP4 codes (decode_weights="mxfp4" from mxfp4_gemm_from sequences on), or
        hip.decode_gemm_fp8 on e4m3 weights AND activations (BASELINE configs[4]); the finalisation owns the row.  In the fp8
        form every finalisation also emits the next projection's input as e4m3 + row scale (so the activation quantiser
        costs no extra launch), and the o projection stays bf16: its input comes from the attention combine, which does not
        own whole rows."""
        cfg, fmt = self.cfg, self.decode_weights
        if fmt == "fp8" and not self.fp8_batched:
            fmt = "bf16"
        fp8 = fmt == "fp8"
        Hq, Hkv, D, H = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.hidden
        scale, eps = D ** -0.5, cfg.rms_eps
        x, x2, qkv, att, act = self.b_x[:B], self.b_x2[:B], self.b_qkv[:B], self.b_attn[:B], self.b_act[:B]
        xn, xn2, part = self.b_xn[:B], self.b_xn2[:B], self.b_part
        step, nq = self.step_b[:B], qkv.shape[1]
        cos, sin, shared = self._decode_rope(B)
        # a_*: the A operand(s) of a projection; to_*: where the finalisation that produces that operand writes it
        if fp8:
            xq, x2q, aq = self.b_xq[:B], self.b_x2q[:B], self.b_actq[:B]
            sxq, sx2q, saq = self.b_sx[0, :B], self.b_sx[1, :B], self.b_sx[2, :B]
            a_x, a_x2, a_act = (xq, sxq), (x2q, sx2q), (aq, saq)
            to_x, to_x2, to_act = dict(yn=xn, yq=xq, yq_scale=sxq), dict(yn=xn2, yq=x2q, yq_scale=sx2q), dict(yq=aq, yq_scale=saq)
            gemm, finalize = hip.decode_gemm_fp8, hip.skinny_finalize_fp8
        else:
            a_x, a_x2, a_act = (xn,), (xn2,), (act,)
            to_x, to_x2, to_act = dict(yn=xn), dict(yn=xn2), {}
            gemm, finalize = hip.decode_gemm_mxfp4 if fmt == "mxfp4" else hip.decode_gemm, hip.skinny_finalize
        gemm_o, fmt_o = (gemm, fmt) if not fp8 else (hip.decode_gemm, "bf16")

        def scales(a, wt):     # the fp8 finalisation multiplies the row and column scales back in
            return dict(sx=a[1], sw=wt[1]) if fp8 else {}

        hip.gather_rows(self.w.embed, self.cur_b[:B], x)
        if fp8:
            hip.quant_rows_fp8(x, xq, sxq, norm_w=self.dec_layers[0].w.ln1_w, eps=eps)
        else:
            hip.rmsnorm(x, self.dec_layers[0].w.ln1_w, eps, out=xn)
        for li, L in enumerate(self.dec_layers):
            lw = L.w
            wt = _wt(L, "qkv_w", fmt)
            ks = gemm(*a_x, *wt, part=part)
            if L.cross:
                q = qkv[:, :Hq * D]
                finalize(part, ks, q, Hq * D, eps=eps, **scales(a_x, wt))
                self._decode_cross_attn(L, q, att, B)
            elif self.fold_qkv:    # the attention workgroups finalise the qkv columns they read (same bits, one launch less)
                hip.decode_attn_parts(part, ks, cos, sin, self.kcache_b[:B, L.idx], self.vcache_b[:B, L.idx], step, self.part_o,
                                      self.part_ml, att, Hq, Hkv, D, self.nsplit, scale, bias=L.bias,
                                      **self._attn_share(B, shared), **scales(a_x, wt))
            else:
                finalize(part, ks, qkv, nq, bias=L.bias, eps=eps, **scales(a_x, wt))
                hip.decode_attn(qkv, cos, sin, self.kcache_b[:B, L.idx], self.vcache_b[:B, L.idx], step, self.part_o,
                                self.part_ml, att, Hq, Hkv, D, self.nsplit, scale, **self._attn_share(B, shared))
            ks = gemm_o(att, *_wt(L, "o_w", fmt_o), part=part)
            finalize(part, ks, x2, H, residual=x, norm_w=lw.ln2_w, eps=eps, **to_x2)
            wt = _wt(L, "gateup_w", fmt)
            ks = gemm(*a_x2, *wt, part=part)
            finalize(part, ks, act, 2 * cfg.intermediate, swiglu=True, eps=eps, **scales(a_x2, wt), **to_act)
            wt = L.q8.get("down_w_pad", L.q8["down_w"]) if fp8 else _wt(L, "down_w", fmt)
            ks = gemm(*a_act, *wt, part=part)
            next_norm = self.dec_layers[li + 1].w.ln1_w if li + 1 < len(self.dec_layers) else self.dec_norm_w
            finalize(part, ks, x, H, residual=x2, norm_w=next_norm, eps=eps, **scales(a_act, wt), **to_x)
        gemm(*a_x, *self.dec_head[fmt], out=self.logits_b[:B])
        self._pick(self.logits_b[:B], self.ws_val, self.ws_idx, self.tokens_b[:B], self.cur_b[:B], step, self.temperature,
                   self.seed)
        self._logprobs_after_pick(B)
        self._stop_after_pick(B)
        self._stream_after_pick(B)

    def _decode_step_fused(self, B: int, projections_only: bool = False) -> int:
        """One decode step for B in-flight sequences, every projection ONE launch (r05, csrc/decode_stream.hip): the stream-K
        weight pass, the fixed-order sum of a cut tile's segments by the last workgroup to arrive, and the epilogue - bias (qkv),
        SwiGLU (gate/up), residual + the NEXT norm's weight + the tile's sum of squares (o, down); the consumer of a normed row
        applies rs[b] = rsqrt(mean(x^2) + eps) to its finished sums (the RMSNorm, TF modeling_qwen2_vl.py:96-110, split into a
        per-column and a per-row factor).  5 launches per layer (r04: 9).  fp8 (configs[4]): activations travel as MX blocks
        written by the producing epilogue.  The tanh gates of Mllama's cross-attention layers are folded into o_w / down_w at
        load time, so both layer kinds share the sequence.  ``projections_only``: bench.py's replay of the weight-streaming
        launches alone.  Returns the number of projection launches.  Opt-in (VIS_DECODE_FUSED=1): _init_decode_state has
        the measurements that keep it off by default."""
        cfg = self.cfg
        Hq, Hkv, D, H = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.hidden
        scale, eps = D ** -0.5, cfg.rms_eps
        x, x2, qkv, att, act = self.b_x[:B], self.b_x2[:B], self.b_qkv[:B], self.b_attn[:B], self.b_act[:B]
        xw, x2w, s1, s2, ws = self.b_xw[:B], self.b_x2w[:B], self.b_ssq1, self.b_ssq2, self.b_proj_ws
        fp8 = self.decode_weights == "fp8" and self.fp8_batched
        if fp8:
            xq, xqs, x2q, x2qs = self.b_xq[:B], self.b_xqs[:B], self.b_x2q[:B], self.b_x2qs[:B]
            aq, aqs = self.b_actq[:B], self.b_actqs[:B]
        # Long-K, few-column projections at many sequences (7B down at 33+ sequences: K = 18944, 28 column tiles) keep the
        # r02-r04 pair - stream-K slabs + the row-owning finalisation, which then also applies the next RMSNorm itself (xw holds
        # the NORMALISED row, its consumer takes no row factor): a column slab per workgroup would stream 2.4 MB of x each, and
        # the in-kernel reduction of the stream-K form costs more than the finalisation launch it saves (64 vs 33 + 5 us,
        # profiles/r05_decode_step_b64_streamk.txt).  VIS_DOWN_PAIR=0 forces the single launch (A/B).
        down_pair = (not fp8) and self.streamk_part and os.environ.get("VIS_DOWN_PAIR", "1") != "0" and \
            hip.decode_proj_form(B, H, cfg.intermediate, hip.DP_RESID_NORMW, False, False) == "streamk"
        s1_in = None if down_pair else s1
        layers = self.dec_layers
        if not projections_only:
            cos, sin, shared = self._decode_rope(B)
            if down_pair:
                hip.gather_rows(self.w.embed, self.cur_b[:B], x)
                hip.rmsnorm(x, layers[0].w.ln1_w, eps, out=xw)
            else:
                hip.decode_prep_rows(self.w.embed, self.cur_b[:B], layers[0].w.ln1_w, x, None if fp8 else xw, s1,
                                     xq if fp8 else None, xqs if fp8 else None)
        for li, L in enumerate(layers):
            lw = L.w
            next_norm = layers[li + 1].w.ln1_w if li + 1 < len(layers) else self.dec_norm_w
            q = qkv[:, :Hq * D] if L.cross else qkv
            if fp8:
                hip.decode_proj_fp8(xq, xqs, *L.q8["qkv_w"], ws, hip.DP_PLAIN, out=q, bias=L.bias, ssq_in=s1, norm_dim=H, eps=eps)
            else:
                hip.decode_proj(xw, lw.qkv_w, ws, hip.DP_PLAIN, out=q, bias=L.bias, ssq_in=s1_in, norm_dim=H, eps=eps)
            if projections_only:
                pass
            elif L.cross:
                self._decode_cross_attn(L, q, att, B)
            else:
                hip.decode_attn(qkv, cos, sin, self.kcache_b[:B, L.idx], self.vcache_b[:B, L.idx], self.step_b[:B], self.part_o,
                                self.part_ml, att, Hq, Hkv, D, self.nsplit, scale, **self._attn_share(B, shared))
            if fp8:     # the o projection keeps bf16 weights (its input comes from the attention kernel); its epilogue writes MX
                hip.decode_proj(att, lw.o_w, ws, hip.DP_RESID_NORMW, out=x2, out_q=x2q, out_qs=x2qs, residual=x,
                                norm_w=lw.ln2_w, ssq_out=s2)
                hip.decode_proj_fp8(x2q, x2qs, *L.q8["gateup_w"], ws, hip.DP_SWIGLU, out_q=aq, out_qs=aqs, ssq_in=s2,
                                    norm_dim=H, eps=eps)
                hip.decode_proj_fp8(aq, aqs, *L.q8.get("down_w_pad", L.q8["down_w"]), ws, hip.DP_RESID_NORMW, out=x, out_q=xq,
                                    out_qs=xqs, residual=x2, norm_w=next_norm, ssq_out=s1)
                continue
            hip.decode_proj(att, lw.o_w, ws, hip.DP_RESID_NORMW, out=x2, out_w=x2w, residual=x, norm_w=lw.ln2_w, ssq_out=s2)
            hip.decode_proj(x2w, lw.gateup_w, ws, hip.DP_SWIGLU, out=act, ssq_in=s2, norm_dim=H, eps=eps)
            if down_pair:
                ks = hip.decode_gemm(act, lw.down_w, part=self.b_part)
                if not projections_only:
                    hip.skinny_finalize(self.b_part, ks, x, H, residual=x2, norm_w=next_norm, yn=xw, eps=eps)
            else:
                hip.decode_proj(act, lw.down_w, ws, hip.DP_RESID_NORMW, out=x, out_w=xw, residual=x2, norm_w=next_norm,
                                ssq_out=s1)
        if fp8:
            hip.decode_proj_fp8(xq, xqs, *self.dec_head["fp8"], ws, hip.DP_PLAIN, out=self.logits_b[:B], ssq_in=s1, norm_dim=H,
                                eps=eps)
        else:
            hip.decode_proj(xw, *self.dec_head["bf16"], ws, hip.DP_PLAIN, out=self.logits_b[:B], ssq_in=s1_in, norm_dim=H, eps=eps)
        if not projections_only:
            self._pick(self.logits_b[:B], self.ws_val, self.ws_idx, self.tokens_b[:B], self.cur_b[:B], self.step_b[:B],
                       self.temperature, self.seed)
            self._logprobs_after_pick(B)
            self._stop_after_pick(B)
            self._stream_after_pick(B)
        return 4 * len(layers) + 1

    # ------------------------------------------------------------------ graphs
    def _captured_step(self, cache: dict, capacity: int, key: tuple, B: int, chained: bool) -> torch.cuda.CUDAGraph:
        """The graph of one step - batched for B sequences, or (B == 0) the single-sequence step - under ``key`` in ``cache``,
        a FIFO of ``capacity`` graphs; captured on first use.  Whatever a step's launches take as plain arguments
        (temperature, seed, the batch size, what the pick's keys name) belongs in ``key``."""
        if key in cache:
            return cache[key]
        step_fn = (lambda: self._decode_step_batched(B)) if B else (lambda: self._decode_step(chained))
        # warm the kernels outside capture, then restore the counters the warm-up advanced
        saved = (self.step_b.clone(), self.cur_b.clone())
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        self._graph_warmup = True
        try:
            with torch.cuda.stream(side):
                step_fn()
        finally:
            self._graph_warmup = False
        torch.cuda.current_stream().wait_stream(side)
        self.step_b.copy_(saved[0])
        self.cur_b.copy_(saved[1])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):     # another agent's thread may be allocating
            step_fn()
        # capture does not execute; state is unchanged
        if len(cache) >= capacity:
            cache.pop(next(iter(cache)))
        cache[key] = g
        return g

    def _decode_steps(self, n_steps: int, use_graph: bool, chained: bool = False) -> None:
        if use_graph:
            g = self._ensure_graph(chained=chained)
            if chained and self.chain_sync is None:      # the warm-up met a refusal: the captured step is the unchained one
                g = self._ensure_graph(chained=False)
            for _ in range(n_steps):
                g.replay()
        else:
            for _ in range(n_steps):
                self._decode_step(chained)

    # ------------------------------------------------------------------ the chained decode of a device, in order
    def _decode_ordered(self, n_steps: int, use_graph: bool) -> None:
        """n_steps further tokens of the single sequence (the engine's decode() has checked its bounds): on the chained
        launches while the context stays within ``chain_ctx_limit`` cached keys, on the four launches per layer head from
        there on (same bits)."""
        base = self.prompt_len + self._decoded       # step k of this call sees base + k cached keys
        self._decoded += n_steps
        n_chain = max(0, min(n_steps, self.chain_ctx_limit - base)) if self.chain_sync is not None else 0
        if n_chain:
            # Chained launches wait inside the grid for workgroups of the SAME launch, which only works while that launch can
            # have its whole grid resident (860 of the device's 1024 slots at 7B shapes).  Two engines decoding on two streams
            # at once could strand each other (each holding slots the other's producers need; the bounded waits would then
            # raise).  So the chained decode calls of a device are ordered on the GPU: a call waits for the previous call's
            # last launch (an event, no host blocking), whatever engine, stream or thread they come from.  Decode is
            # HBM-bound: nothing is lost.
            self._chain_epoch_guard(n_chain)
            with _chain_order_lock(self.device.index):
                cur = torch.cuda.current_stream(self.device)
                prev = _CHAIN_LAST.get(self.device.index)
                if prev is not None:
                    cur.wait_event(prev)
                self._decode_steps(n_chain, use_graph, True)
                ev = torch.cuda.Event()
                ev.record(cur)
                _CHAIN_LAST[self.device.index] = ev
        if n_steps > n_chain:       # no chain, or the context has outgrown the chained grid
            self._decode_steps(n_steps - n_chain, use_graph, False)

    def _chain_epoch_guard(self, n_steps: int) -> None:
        """The granule tag of a chained launch is the sync block's 32-bit launch counter + 1.  Long before it can wrap
        (2^31 launches = ~2.6 days of continuous single-sequence decode) workspace and sync block are zeroed on the stream,
        between two decode calls - no launch of this engine is in flight then (same stream), and the kernel itself skips
        tag 0, the mark of a never-written granule (tests/test_kernels_gpu.py::test_decode_chain_epoch_wrap)."""
        self._chain_launches += n_steps * self.dec_n_self
        if self._chain_launches >= (1 << 31):
            self.chain_sync.zero_()
            self.chain_ws.zero_()
            self._chain_launches = n_steps * self.dec_n_self

    def generated(self, n: int) -> List[int]:
        s = self.prompt_len - 1          # the token generated at step i is stored at index (its position - 1)
        toks = self.tokens[s:s + n].cpu().tolist()
        self.check_chain()
        return toks

    def check_chain(self) -> None:
        """Raise if a bounded wait inside a chained layer-head launch gave up (its results are invalid); the sync block is
        zeroed so that the engine stays usable.  Called after the token D2H, i.e. when the stream has drained."""
        if self.chain_sync is not None and int(self.chain_sync[hip.CHAIN_STATUS_WORD].item()) != 0:
            self.chain_sync.zero_()
            self.chain_ws.zero_()
            self._chain_launches = 0
            raise hip.ChainStalled("vis_decode_chain: a hand-off wait inside the launch timed out (decode results invalid)")
