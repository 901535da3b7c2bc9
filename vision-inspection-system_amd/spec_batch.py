"""Lossless n-gram speculative decoding of a BATCH: B in-flight sequences with R = 1 + k rows each - the current token and up
to k drafted ones - run as B * R rows of the stream-K batched step, one pass over the weights.  An engine setting
(``Qwen2VLEngine(batch_speculative=)``, VIS_SPECULATIVE_BATCH), not a request keyword: a batch speculates where it can
(``eligible``) and runs the plain step otherwise, and the replies are the plain replies token for token either way.

Why it is lossless without new arithmetic: a row of the stream-K projection is bit-invariant to the number of rows and to
its position among them, vis_skinny_finalize owns whole rows, and vis_decode_attn_draft_batch gives row (b, r) the bits of the
plain batched attention launch at step[b] + r.  Row (b, r)'s logits therefore are the logits the plain step of sequence b
would have computed behind the drafts in front of it, and vis_spec_accept_batch keeps exactly the drafts the picks confirm.

The step and its loop work on the engine (a decode_stage.DecodeStage): ``step`` is DecodeStage._decode_step_streamk with B * R
rows and the step's own buffers, ``run`` the batch's counterpart of Generation._run_single_spec."""
from __future__ import annotations

import os
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import hip, spec
from .sampling import SLOT_SEED_STRIDE

MAX_ROWS = 64      # rows of one stream-K step (four 16-row MFMA blocks): B * R may not exceed it, nor the engine's max_batch


def check_setting(setting) -> Optional[spec.SpecConfig]:
    """The engine setting -> SpecConfig or None (off): None, the integer k or spec.check_speculative's dict; ``sampled`` may
    be set (a batch at a temperature keeps speculating), ``grammar`` may not: the schema's rows are single-sequence state."""
    cfg = spec.check_speculative(setting)
    if cfg is not None and cfg.grammar:
        raise ValueError("batch_speculative: 'grammar' is not supported (the schema's row masks serve one sequence)")
    return cfg


def from_env() -> Optional[spec.SpecConfig]:
    """VIS_SPECULATIVE_BATCH=k (1..3; unset, empty or 0 = off; anything else: ValueError): the client builds the Qwen2-VL
    engines with batch_speculative=k.  VIS_SPECULATIVE_SAMPLED=1 next to it adds ``sampled``."""
    sampled = spec.sampled_from_env()
    v = os.environ.get("VIS_SPECULATIVE_BATCH", "").strip()
    if v in ("", "0"):
        return None
    try:
        k = int(v)
    except ValueError:
        k = -1
    if not 1 <= k <= spec.MAX_K:
        raise ValueError(f"VIS_SPECULATIVE_BATCH must be an integer in 0..{spec.MAX_K}")
    return check_setting({"num_speculative_tokens": k, "sampled": sampled})


def eligible(n_req: int, n_live: int, rows: int, max_batch: int, plain_step: str, attn_streams: bool,
             switches: Iterable[str], temperature: float, sampled: bool) -> bool:
    """Whether a batch of ``n_req`` requests, ``n_live`` of which got a slot, takes the speculative step of ``rows`` rows per
    sequence.  ``plain_step``: the step B plain sequences would take ("streamk", "rows" or "fused",
    DecodeStage._batched_step_kind) - only the stream-K step has the row invariance the scheme rests on; ``attn_streams``:
    vis_decode_attn_streams for B sequences (the streaming attention has no draft form); ``switches``: the names of what the
    group switched on besides ``seeds`` (every one is a per-step state of the pick); a temperature needs ``sampled``."""
    return (n_live == n_req and n_req >= 2 and n_req * rows <= min(MAX_ROWS, max_batch) and plain_step == "streamk"
            and not attn_streams and not list(switches) and (sampled or not temperature))


def switches_on(eng, ns) -> List[str]:
    """What the running group switched on besides ``seeds``, read from the pick stage's own flags."""
    flags = (("logprobs", eng.lp_k is not None), ("json_mode", eng.json_on), ("json_schema", eng.schema_on),
             ("top_p", eng.top_p is not None), ("penalties", eng.pen_on), ("shaping", eng.shape_on), ("ban", eng.ban_on),
             ("stop", eng.stop_on), ("on_stream", eng.stream_on), ("n", ns is not None))
    return [name for name, on in flags if on]


def plan(eng, n_req: int, ns, temperature: float) -> Optional[spec.SpecConfig]:
    """In front of a batch's prompt passes: the engine's configuration when the batch may speculate if every request turns
    out live, else None.  (The prompt passes then prepare rope rows for R - 1 further positions.)"""
    cfg = eng.batch_speculative
    if cfg is None or not eligible(n_req, n_req, cfg.rows, eng.max_batch, eng._batched_step_kind(n_req),
                                   hip.decode_attn_streams(eng.cfg.kv_heads, n_req), switches_on(eng, ns), temperature,
                                   cfg.sampled):
        return None
    return cfg


class SpecBatchBuffers:
    """What the batched speculative step of one engine owns, for up to ``rows`` = min(64, max_batch) packed rows: activation
    rows in the formats the stream-K step carries (bf16, and e4m3 + row scales for an fp8 engine), the attention workspace, the
    f32 logits, the pick workspace, and per sequence the draft row [3], its count, the limit, the prompt's ids and length, the
    start of the reply in the token row, the counters (steps, proposed, accepted) and the sampled accept's parameters."""

    def __init__(self, cfg, nsplit: int, max_ctx: int, rows: int, fp8: bool, kpad: Optional[int], device):
        bf, dev, n, seqs = torch.bfloat16, device, rows, max(1, rows // 2)
        H, I, Hq, D = cfg.hidden, cfg.intermediate, cfg.heads, cfg.head_dim
        nq = (Hq + 2 * cfg.kv_heads) * D
        for name, cols in (("x", H), ("x2", H), ("qkv", nq), ("act", I), ("xn", H), ("xn2", H)):
            setattr(self, name, torch.empty((n, cols), dtype=bf, device=dev))
        self.attn = torch.zeros((n, Hq * D), dtype=bf, device=dev)      # a row past the cache is never written
        if fp8:      # pad columns of the down projection's input rows stay 0
            self.xq = torch.zeros((n, H), dtype=torch.uint8, device=dev)
            self.x2q = torch.zeros((n, H), dtype=torch.uint8, device=dev)
            self.actq = torch.zeros((n, kpad), dtype=torch.uint8, device=dev)
            self.sx = torch.zeros((3, n), dtype=torch.float32, device=dev)
        self.logits = torch.empty((n, cfg.vocab), dtype=torch.float32, device=dev)
        self.part_o = torch.empty(n * Hq * nsplit * D, dtype=torch.float32, device=dev)
        self.part_ml = torch.empty(n * Hq * nsplit * 2, dtype=torch.float32, device=dev)
        self.ws_val = torch.empty(256 * n, dtype=torch.float32, device=dev)
        self.ws_idx = torch.empty(256 * n, dtype=torch.int32, device=dev)
        self.prompt = torch.zeros((seqs, max_ctx), dtype=torch.int32, device=dev)
        # one int32 block, so that a request's start and a graph warm-up's undo are one copy: per sequence draft [3],
        # n_draft, limit, prompt_len, gen_start, counters [3], params [2] (the bits of the f32 inv_temp, the uint32 seed)
        self._ints = torch.zeros(12 * seqs, dtype=torch.int32, device=dev)
        cut = lambda i, w: self._ints[i * seqs:(i + w) * seqs]      # noqa: E731
        self.draft, self.n_draft, self.limit = cut(0, 3).view(seqs, 3), cut(3, 1), cut(4, 1)
        self.prompt_len, self.gen_start = cut(5, 1), cut(6, 1)
        self.counters, self.params = cut(7, 3).view(seqs, 3), cut(10, 2).view(seqs, 2)
        self.seqs = seqs
        self.graphs: dict = {}      # the captured steps (graph())

    def begin(self, prompts: Sequence[torch.Tensor], starts: Sequence[int], limits: Sequence[int],
              inv_temp: float, seeds: Sequence[int]) -> None:
        """A batch starts behind its prompt passes: every sequence's prompt ids, where its reply starts and may end, no
        drafts, counters at zero, and its inverse temperature (as hip.argmax forms it; 0 = greedy) and seed modulo 2^32."""
        B, S = len(prompts), self.seqs
        host = np.zeros((12, S), dtype=np.int32)
        for b, ids in enumerate(prompts):
            self.prompt[b, :ids.numel()].copy_(ids)
            host[5, b] = ids.numel()
        host[4, :B], host[6, :B] = limits, starts
        par = np.zeros((S, 2), dtype=np.uint32)
        par[:B, 0] = np.float32(inv_temp).view(np.uint32)
        par[:B, 1] = [int(s) & 0xFFFFFFFF for s in seeds]
        flat = host.reshape(-1)
        flat[10 * S:] = par.view(np.int32).reshape(-1)
        self._ints.copy_(torch.from_numpy(flat))

    def read_counters(self, B: int) -> List[List[int]]:
        return [[int(v) for v in row] for row in self.counters[:B].cpu().tolist()]


def buffers(eng) -> SpecBatchBuffers:
    """The engine's buffers of the step, allocated on first use."""
    if eng._spec_batch is None:
        eng._spec_batch = SpecBatchBuffers(eng.cfg, eng.nsplit, eng.max_ctx, min(MAX_ROWS, eng.max_batch), eng.fp8_batched,
                                           eng.kpad, eng.device)
    return eng._spec_batch


def draft(eng, cfg: spec.SpecConfig, B: int) -> None:
    """vis_spec_draft_batch for the next step: sequence b's prompt lookup over its prompt and its reply so far."""
    sb = eng._spec_batch
    hip.spec_draft_batch(sb.prompt[:B], sb.prompt_len[:B], eng.tokens_b[:B], sb.gen_start[:B], eng.step_b[:B], cfg.k,
                         cfg.lookup_max, cfg.lookup_min, eng.cfg.vocab, sb.draft[:B], sb.n_draft[:B])


def step(eng, cfg: spec.SpecConfig, B: int, propose: bool = True) -> None:
    """One speculative step of slots 0 .. B - 1: DecodeStage._decode_step_streamk with B * R rows.  vis_spec_gather_batch
    packs [cur, draft 0 .. draft R-2] of every sequence; each layer's qkv projection is finalised into packed rows for
    vis_decode_attn_draft_batch (the unfolded pair, bit-identical to the plain step's folded launch); the other projections
    and the lm_head are the plain step's; then vis_spec_accept_batch - which keeps the drafts the picks confirm and advances
    step[b] by 1..R - and vis_spec_draft_batch for the next step.  ``propose`` False leaves the drafts alone (tests plant them)."""
    from .decode_stage import _wt
    mc, sb, R = eng.cfg, eng._spec_batch, cfg.rows
    fmt = eng.decode_weights
    if fmt == "fp8" and not eng.fp8_batched:
        fmt = "bf16"
    fp8 = fmt == "fp8"
    Hq, Hkv, D, H = mc.heads, mc.kv_heads, mc.head_dim, mc.hidden
    scale, eps, n = D ** -0.5, mc.rms_eps, B * R
    x, x2, qkv, att, act, xn, xn2 = sb.x[:n], sb.x2[:n], sb.qkv[:n], sb.attn[:n], sb.act[:n], sb.xn[:n], sb.xn2[:n]
    part, seq_step, nq = eng.b_part, eng.step_b[:B], qkv.shape[1]
    cos, sin, _ = eng._decode_rope(B)      # the split attention reads every slot's own copy of a shared prefix
    if fp8:
        xq, x2q, aq = sb.xq[:n], sb.x2q[:n], sb.actq[:n]
        sxq, sx2q, saq = sb.sx[0, :n], sb.sx[1, :n], sb.sx[2, :n]
        a_x, a_x2, a_act = (xq, sxq), (x2q, sx2q), (aq, saq)
        to_x, to_x2, to_act = dict(yn=xn, yq=xq, yq_scale=sxq), dict(yn=xn2, yq=x2q, yq_scale=sx2q), dict(yq=aq, yq_scale=saq)
        gemm, finalize = hip.decode_gemm_fp8, hip.skinny_finalize_fp8
    else:
        a_x, a_x2, a_act = (xn,), (xn2,), (act,)
        to_x, to_x2, to_act = dict(yn=xn), dict(yn=xn2), {}
        gemm, finalize = hip.decode_gemm_mxfp4 if fmt == "mxfp4" else hip.decode_gemm, hip.skinny_finalize
    gemm_o, fmt_o = (gemm, fmt) if not fp8 else (hip.decode_gemm, "bf16")

    def scales(a, wt):
        return dict(sx=a[1], sw=wt[1]) if fp8 else {}

    layers = eng.dec_layers
    hip.spec_gather_batch(eng.w.embed, eng.cur_b[:B], sb.draft[:B], x)
    if fp8:
        hip.quant_rows_fp8(x, xq, sxq, norm_w=layers[0].w.ln1_w, eps=eps)
    else:
        hip.rmsnorm(x, layers[0].w.ln1_w, eps, out=xn)
    for li, L in enumerate(layers):
        lw = L.w
        wt = _wt(L, "qkv_w", fmt)
        ks = gemm(*a_x, *wt, part=part)
        finalize(part, ks, qkv, nq, bias=L.bias, eps=eps, **scales(a_x, wt))
        hip.decode_attn_draft_batch(qkv, cos, sin, eng.kcache_b[:B, L.idx], eng.vcache_b[:B, L.idx], seq_step, sb.part_o,
                                    sb.part_ml, att, Hq, Hkv, D, eng.nsplit, scale)
        ks = gemm_o(att, *_wt(L, "o_w", fmt_o), part=part)
        finalize(part, ks, x2, H, residual=x, norm_w=lw.ln2_w, eps=eps, **to_x2)
        wt = _wt(L, "gateup_w", fmt)
        ks = gemm(*a_x2, *wt, part=part)
        finalize(part, ks, act, 2 * mc.intermediate, swiglu=True, eps=eps, **scales(a_x2, wt), **to_act)
        wt = L.q8.get("down_w_pad", L.q8["down_w"]) if fp8 else _wt(L, "down_w", fmt)
        ks = gemm(*a_act, *wt, part=part)
        next_norm = layers[li + 1].w.ln1_w if li + 1 < len(layers) else eng.dec_norm_w
        finalize(part, ks, x, H, residual=x2, norm_w=next_norm, eps=eps, **scales(a_act, wt), **to_x)
    logits = sb.logits[:n]
    gemm(*a_x, *eng.dec_head[fmt], out=logits)
    hip.spec_accept_batch(logits, sb.draft[:B], sb.n_draft[:B], sb.limit[:B], sb.ws_val, sb.ws_idx, eng.tokens_b[:B],
                          eng.cur_b[:B], seq_step, sb.counters[:B], sb.params[:B] if cfg.sampled else None)
    if propose and R > 1:
        draft(eng, cfg, B)


def graph(eng, cfg: spec.SpecConfig, B: int) -> torch.cuda.CUDAGraph:
    """The captured step, keyed by ("spec_batch", B, R, weight format, the lookup window, sampled): everything else - the
    drafts, the limits, the prompts, the inverse temperatures and seeds - is device memory.  The warm-up step advances the
    batch's counters and writes token rows; both are put back before the capture."""
    key = ("spec_batch", B, cfg.rows, eng.decode_weights, cfg.lookup_max, cfg.lookup_min, cfg.sampled)
    sb = buffers(eng)
    cache = sb.graphs
    if key in cache:
        return cache[key]
    saved = (eng.step_b.clone(), eng.cur_b.clone(), sb._ints.clone(), eng.tokens_b[:B].clone())
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(eng, cfg, B)
    torch.cuda.current_stream().wait_stream(side)
    eng.step_b.copy_(saved[0])
    eng.cur_b.copy_(saved[1])
    sb._ints.copy_(saved[2])
    eng.tokens_b[:B].copy_(saved[3])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step(eng, cfg, B)
    if len(cache) >= 4:
        cache.pop(next(iter(cache)))
    cache[key] = g
    return g


def run(eng, cfg: spec.SpecConfig, B: int, starts: Sequence[int], max_new_tokens: int, eos: set, ignore_eos: bool,
        use_graph: bool, check_every: int, temperature: float):
    """The decode loop of a batch behind its prompt passes, with speculative steps: ``check_every`` steps are issued ahead,
    then the poll reads the step counters and the token rows - a step has given every sequence 1..R tokens.  Sequence b's own
    ``limit`` cuts its last step's run at max_new_tokens tokens, and steps issued past it change nothing of b.  Ends when
    every sequence has an EOS or its full length.  Returns (token lists per slot, steps issued, the ``spec_*`` timing keys:
    sums over the sequences, and ``spec_sequences`` = every sequence's own [steps, proposed, accepted])."""
    sb = buffers(eng)
    limits = [min(s + max_new_tokens - 1, eng.max_ctx - 2) for s in starts]
    sb.begin([eng._slot_ids[b] for b in range(B)], starts, limits, (1.0 / temperature) if temperature > 0 else 0.0,
             [eng._slot_seed.get(b, eng.seed + SLOT_SEED_STRIDE * b) for b in range(B)])      # PickStage._seed_slot's choice
    draft(eng, cfg, B)      # behind the prompt passes' picks: the first step already carries drafts

    def poll():      # two D2H: the step counters, then the token rows they cover
        st = eng.step_b[:B].cpu().tolist()
        t = eng.tokens_b[:B].cpu()
        return [t[b, starts[b]:starts[b] + min(st[b] - starts[b], max_new_tokens)].tolist() for b in range(B)]

    def open_(toks):
        return len(toks) < max_new_tokens and (ignore_eos or not any(t in eos for t in toks))

    outs, steps = poll(), 0
    g = graph(eng, cfg, B) if use_graph else None
    while any(open_(t) for t in outs):
        n = min(check_every, max(max_new_tokens - len(t) for t in outs if open_(t)))
        for _ in range(n):
            if g is not None:
                g.replay()
            else:
                step(eng, cfg, B)
        steps += n
        outs = poll()
    per = sb.read_counters(B)
    tot = [sum(c[i] for c in per) for i in range(3)]
    return outs, steps, {"spec_steps": tot[0], "spec_proposed": tot[1], "spec_accepted": tot[2], "spec_sequences": per}


def simulate(plain_reply: Sequence[int], prompt: Sequence[int], k: int, lookup_max: int = 4, lookup_min: int = 2,
             max_new_tokens: Optional[int] = None, vocab: Optional[int] = None) -> dict:
    """What ONE sequence of a speculative batch run to its full length (ignore_eos) must report, without a model: the scheme
    is lossless, so the pick behind any accepted prefix is the plain reply's next token.  Walks the steps as
    vis_spec_accept_batch takes them, with ``spec.propose`` over prompt + reply behind the prompt pass and behind every step
    (ids clamped into [0, vocab)); the limit cuts the last step's run.  Returns {"reply", "spec_steps", "spec_proposed",
    "spec_accepted"}."""
    plain = [int(t) for t in plain_reply]
    N = len(plain) if max_new_tokens is None else min(len(plain), max_new_tokens)

    def lookup(reply):
        d = spec.propose(list(prompt) + reply, k, lookup_max, lookup_min)
        return d if vocab is None else [min(max(t, 0), vocab - 1) for t in d]

    reply = plain[:1]
    d = lookup(reply)
    steps = proposed = accepted = 0
    while len(reply) < N:
        n, a = len(reply), 0
        while a < len(d) and n + a < N - 1 and d[a] == plain[n + a]:
            a += 1
        reply = plain[:n + a + 1]
        steps, proposed, accepted = steps + 1, proposed + len(d), accepted + a
        d = lookup(reply)
    return {"reply": reply, "spec_steps": steps, "spec_proposed": proposed, "spec_accepted": accepted}
