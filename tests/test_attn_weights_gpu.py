"""Softmax weights of every attention kernel, exactly: power-of-two weights that differ for the queries of a wave, a q-block
and a GQA group, checked against the float64 reference of tests/attn_weights.py inside a derived slack of
(6 A + 16) * 2^-23 relative (A = keys of non-zero weight) - far below one bf16 ulp.  Every output element of every query is
checked, plus |out| < 64 (poison keys, NaN workspaces) and, in decode, the appended K / V cache row bit for bit.

Can the first key tile of a prefill work item be fully masked for a query (its reference would become -1e30 and the next
tile's scores +1e30)?  No: a work item's tile grid starts at k0 & ~63, so tile 0 holds key k0 itself, and k0 <= q0 for every
list the library builds (make_attn_work / plan_attn_items*: k0 = the segment's start; make_attn_pairs and a row offset: keys
from 0; the second half of a key-split item: k0 = the cut, a multiple of 64, non-causal).  Key k0 is valid for every row of
the item - also under the causal rule, k0 <= q0 <= q - and rows past the item's end are computed with clamped q and never
stored.  What tile 0 CAN do is move the reference down; with a first tile entirely below -128 log2 units the rescale factor
exp2(-d) of that move overflowed to inf and turned the still-zero accumulators into NaN (every bg_first query here showed it);
the factor is now clamped to 1.
"""
import pytest
import torch

import attn_weights as W
from test_attn_coverage_gpu import _nan, _vt

pytestmark = pytest.mark.gpu

HD = 128


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


# ----------------------------------------------------------------------------- prefill
def _prefill_check(c, out, what):
    o = out.float().cpu()
    for kv, u in enumerate(c.units):
        W.check(u, W.prefill_got(c, o, kv), f"{what}: {c.name} kv head {kv}")


def _blank(rows, cols, device):
    return torch.full((rows, cols), float("nan"), dtype=torch.bfloat16, device=device)


@pytest.mark.parametrize("Hq,Hkv", W.PREFILL_HEADS)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", W.PREFILL_S)
def test_prefill128(hip, device, S, causal, Hq, Hkv):
    """attn_prefill_kernel<128> (and attn_prefill_pair_kernel on the causal cases): two, three and six key tiles, ragged last
    tile and q-block.  The (2, 2) non-causal S = 130 case holds the two-direction queries."""
    c = W.prefill128(S, causal, Hq, Hkv)
    Q, K, vt = c.Q.to(device), c.K.to(device), _vt(hip, c.V.to(device), device)
    out = _blank(S, Hq * HD, device)
    hip.attn_prefill(Q, K, vt, out, hip.make_attn_work(c.segments, causal, device, heads=Hq), causal, W.SCALE)
    _prefill_check(c, out, "attn_prefill")
    if causal:
        out = _blank(S, Hq * HD, device)
        hip.attn_prefill_pairs(Q, K, vt, out, hip.make_attn_pairs(0, S, device), W.SCALE)
        _prefill_check(c, out, "attn_prefill_pairs")


@pytest.mark.parametrize("Hq,Hkv", W.PREFILL_HEADS)
def test_prefill128_row_offset(hip, device, Hq, Hkv):
    """vis_attn_prefill_rows and the pairs kernel with q_row0 = 65 over S = 130: the causal diagonal sits at 65 + row."""
    P, S = 65, 130
    c = W.prefill128(S, True, Hq, Hkv, P=P)
    Q, K, vt = c.Q.to(device), c.K.to(device), _vt(hip, c.V.to(device), device)
    work = torch.tensor([(q0, min(128, S - q0), 0, S) for q0 in range(P, S, 128)], dtype=torch.int32, device=device)
    out = _blank(S - P, Hq * HD, device)
    hip.attn_prefill(Q, K, vt, out, work.reshape(-1, 4).contiguous(), True, W.SCALE, q_row0=P)
    _prefill_check(c, out, "attn_prefill rows")
    out = _blank(S - P, Hq * HD, device)
    hip.attn_prefill_pairs(Q, K, vt, out, hip.make_attn_pairs(P, S, device), W.SCALE, q_row0=P)
    _prefill_check(c, out, "attn_prefill_pairs rows")


@pytest.mark.parametrize("pairs,causal", [(False, False), (False, True), (True, True)])
def test_prefill128_many_requests(hip, device, pairs, causal):
    """attn_prefill_many / attn_prefill_pairs_many: three requests in one launch, each with its own columns and V rows, in
    cache blocks of 192 rows whose rows past the 130 keys are poison."""
    Hq, Hkv, S, T, k = 4, 1, 130, 192, 3
    cases = [W.prefill128(S, causal, Hq, Hkv, T=T, salt=j + 1) for j in range(k)]
    slots = [2, 0, 3]
    kc = torch.zeros((4, Hkv, T, HD), dtype=torch.bfloat16, device=device)
    vt = torch.zeros((k, Hkv, HD, T), dtype=torch.bfloat16, device=device)
    q = torch.zeros((k, Hq, S, HD), dtype=torch.bfloat16, device=device)
    for j, c in enumerate(cases):
        q[j], kc[slots[j]], vt[j] = c.Q.to(device), c.K.to(device), _vt(hip, c.V.to(device), device)
    kv_off = [s * kc.stride(0) for s in slots]
    out = _blank(k * S, Hq * HD, device)
    if pairs:
        hip.attn_prefill_pairs_many(q, kc, vt, out, hip.make_attn_pairs(0, S, device), W.SCALE, kv_off, T)
    else:
        items = [[(q0, min(128, S - q0), 0, S) for q0 in range(0, S, 128)] for _ in range(k)]
        work = torch.tensor(items, dtype=torch.int32, device=device).reshape(k, -1, 4).contiguous()
        hip.attn_prefill_many(q, kc, vt, out, work, causal, W.SCALE, kv_off, T)
    for j, c in enumerate(cases):
        _prefill_check(c, out[j * S:(j + 1) * S], f"many request {j} pairs {pairs}")


def test_prefill80_vit_segments(hip, device):
    """attn_vit32_kernel through the plan the engines build: S = 320 in segments (64, 192, 64), 3 heads."""
    c = W.prefill80(False)
    plan = hip.make_vit_attn_plan(c.segments, device, 3)
    assert plan.n_pairs == 0
    out = _blank(320, 3 * 80, device)
    hip.attn_prefill_plan(c.Q.to(device), c.K.to(device), _vt(hip, c.V.to(device), device), out, plan, W.SCALE)
    _prefill_check(c, out, "attn_prefill_plan")


def test_prefill80_narrow_kernel(hip, device):
    """attn_prefill_kernel<80> - the 16-wide form with f32 lane sums for the denominator (MFMA_SUM false) - through its causal
    instantiation, the one a launch reaches whatever the process environment says."""
    c = W.prefill80(True)
    out = _blank(320, 3 * 80, device)
    hip.attn_prefill(c.Q.to(device), c.K.to(device), _vt(hip, c.V.to(device), device), out,
                     hip.make_attn_work(c.segments, True, device, heads=3), True, W.SCALE)
    _prefill_check(c, out, "attn_prefill d80 causal")


def test_prefill80_key_split(hip, device):
    """vis_attn_prefill_split at the smallest S whose plan splits (read from the plan): columns peak in the first half
    (max_first, rise*, one_tile ..), in the second (bg_first) and in both (two_max); the halves merge with a_s / a_o."""
    S = 128 * (hip.ATTN_SPLIT_MIN_BLOCKS - 1) + 1
    assert hip.make_vit_attn_plan([(0, S - 1)], device, 3).n_pairs == 0
    plan = hip.make_vit_attn_plan([(0, S)], device, 3)
    w = plan.work.cpu().tolist()
    cuts = {it[3] for it in w if (it[1] >> 8) & 1 and not (it[1] >> 9) & 1}
    assert plan.n_pairs > 0 and S == W.SPLIT_S and cuts == {W.SPLIT_MID}
    c = W.prefill80_split(S, W.SPLIT_MID)
    out = _blank(S, 3 * 80, device)
    hip.attn_prefill_plan(c.Q.to(device), c.K.to(device), _vt(hip, c.V.to(device), device), out, plan, W.SCALE)
    _prefill_check(c, out, "attn_prefill_plan key-split")


# ----------------------------------------------------------------------------- prefill: operands inside poisoned buffers
# The cases above again, with the memory AROUND the operands hostile.  K is a contiguous view whose last head is followed, in
# the same allocation, by GUARD_ROWS rows of bf16 NaN - what a ragged last key tile brings into LDS if its load reaches past the
# head (tests/test_buffer_range_gpu.py measures whether it does); Q is followed by NaN rows too; `out` is a view (rows
# GUARD_ROWS .., the first Hq * D columns) of a wider and taller buffer filled with a canary word.  The V^T pad columns stay
# ZERO: csrc/rope.hip documents that vis_qkv_rope_split zeroes them and the kernels rely on it (the probability of a masked key
# is 0, and 0 x pad must stay 0), so that is a contract of the input, not memory behind it.
# Pinned: masking stays a SELECT (an additive mask would turn a NaN score into a NaN output), and a launch writes its own rows
# and columns of `out` and nothing else.
GUARD_ROWS = 64
CANARY = 0x4B1D                  # as bf16 about 1.0e7: an output element left unwritten also fails check's |out| < 64


def _nan_tailed(t, device):
    """t [H, n, D] -> the same values as a contiguous view at the start of one allocation whose last GUARD_ROWS x D are NaN."""
    H, n, D = t.shape
    flat = torch.full(((H * n + GUARD_ROWS) * D,), float("nan"), dtype=torch.bfloat16, device=device)
    flat[:H * n * D] = t.to(device).reshape(-1)
    assert bool(flat[H * n * D:].isnan().all())
    return flat[:H * n * D].view(H, n, D)


def _embedded(hip, device, c, launch, what):
    """launch(Q, K, vt, out) on the plain layout, then on the embedded one: same `check`, same bits, canary untouched."""
    Hq, S, D = c.Q.shape
    vt = _vt(hip, c.V.to(device), device)
    plain = _blank(S, Hq * D, device)
    launch(c.Q.to(device), c.K.to(device), vt, plain)
    _prefill_check(c, plain, f"{what}, plain layout")
    buf = torch.full((S + 2 * GUARD_ROWS, Hq * D + 64), CANARY, dtype=torch.int16, device=device)
    out = buf.view(torch.bfloat16)[GUARD_ROWS:GUARD_ROWS + S, :Hq * D]
    launch(_nan_tailed(c.Q, device), _nan_tailed(c.K, device), vt, out)
    _prefill_check(c, out, f"{what}, operands inside poisoned buffers")
    assert torch.equal(out.contiguous().view(torch.int16), plain.view(torch.int16)), f"{what}: bits differ from the plain-layout run"
    guard = buf.clone()
    guard[GUARD_ROWS:GUARD_ROWS + S, :Hq * D] = CANARY
    touched = int((guard != CANARY).sum())
    assert touched == 0, f"{what}: {touched} canary words outside `out` were written"


def test_prefill80_poisoned_surroundings(hip, device):
    """attn_vit32_kernel on the head_dim 80 case whose key count is no multiple of 64 (S = 2945 through the key-split plan: the
    whole items and the second halves end in a tile with ONE key and 63 rows past the head)."""
    c = W.prefill80_split(W.SPLIT_S, W.SPLIT_MID)
    assert W.SPLIT_S % 64 == 1
    plan = hip.make_vit_attn_plan([(0, W.SPLIT_S)], device, 3)
    assert plan.n_pairs > 0
    _embedded(hip, device, c, lambda Q, K, vt, out: hip.attn_prefill_plan(Q, K, vt, out, plan, W.SCALE), "attn_prefill_plan key-split")


@pytest.mark.parametrize("entry", ["rows", "pairs"])
def test_prefill128_causal_poisoned_surroundings(hip, device, entry):
    """The smallest causal head_dim 128 case, S = 65 (heads 2 / 2: the first head's ragged tile reaches into the second head's
    rows, the second head's into the NaN rows), through vis_attn_prefill_rows and through attn_prefill_pair_kernel."""
    S = W.PREFILL_S[0]
    assert S % 64 and S == min(W.PREFILL_S)
    c = W.prefill128(S, True, 2, 2)
    if entry == "rows":
        work = hip.make_attn_work(c.segments, True, device, heads=2)
        launch = lambda Q, K, vt, out: hip.attn_prefill(Q, K, vt, out, work, True, W.SCALE)
    else:
        work = hip.make_attn_pairs(0, S, device)
        launch = lambda Q, K, vt, out: hip.attn_prefill_pairs(Q, K, vt, out, work, W.SCALE)
    _embedded(hip, device, c, launch, f"attn_prefill {entry}")


# ----------------------------------------------------------------------------- decode
def _decode_launch(hip, device, c, T, seqs, batched, shared_len=0, fork=None, parts=None):
    """seqs: the sequences of case c to run (one launch).  -> (out [len(seqs), Hq * D], k cache, v cache after)."""
    B, Hq, Hkv = len(seqs), c.Hq, c.Hkv
    ns = T // hip.DECODE_KEYS_PER_SPLIT
    idx = torch.tensor(seqs)
    kc, vc = c.K[idx].to(device).contiguous(), c.V[idx].to(device).contiguous()
    qkv = c.qkv[idx].to(device).contiguous()
    cos, sin = torch.ones((T, HD), device=device), torch.zeros((T, HD), device=device)
    po, pml = _nan(B * Hq * ns * HD, device), _nan(B * Hq * ns * 2, device)
    step = torch.tensor([c.ctxs[b] - 1 for b in seqs], dtype=torch.int32, device=device)
    if not batched:
        assert B == 1
        out = torch.full((Hq * HD,), float("nan"), dtype=torch.bfloat16, device=device)
        k1, v1 = kc[0].contiguous(), vc[0].contiguous()
        hip.decode_attn(qkv[0].contiguous(), cos, sin, k1, v1, step, po, pml, out, Hq, Hkv, HD, ns, W.SCALE)
        return out[None], k1[None], v1[None]
    out = torch.full((B, Hq * HD), float("nan"), dtype=torch.bfloat16, device=device)
    cosb, sinb = cos.expand(B, -1, -1), sin.expand(B, -1, -1)
    if parts is not None:
        nq = qkv.shape[1]
        rows = hip.part_rows(B)
        part = torch.full((rows * nq,), float("nan"), dtype=torch.float32, device=device)
        part.view(rows, nq)[:B] = qkv.float()                # ksplit 1: the slab IS the row; fp8 form: unit scales
        sx = torch.ones(B, dtype=torch.float32, device=device) if parts == "fp8" else None
        sw = torch.ones(nq, dtype=torch.float32, device=device) if parts == "fp8" else None
        hip.decode_attn_parts(part, 1, cosb, sinb, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, W.SCALE, sx=sx, sw=sw)
    else:
        hip.decode_attn(qkv, cosb, sinb, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, W.SCALE, shared_len=shared_len, fork=fork)
    return out, kc, vc


def _decode_check(c, seqs, out, kc, vc, what):
    o = out.float().cpu()
    kc, vc = kc.float().cpu(), vc.float().cpu()
    for j, b in enumerate(seqs):
        n = c.ctxs[b]
        for kv in range(c.Hkv):
            G = c.Hq // c.Hkv
            got = o[j].reshape(c.Hq, HD)[kv * G:(kv + 1) * G].double().numpy()
            W.check(c.units[b * c.Hkv + kv], got, f"{what}: {c.name[:48]} seq {b} ctx {n} kv head {kv}")
        assert torch.equal(kc[j, :, n - 1], c.knew[b]) and torch.equal(vc[j, :, n - 1], c.vnew[b]), \
            f"{what}: seq {b}: appended K / V row"


@pytest.mark.parametrize("mode", ["0", "2"])
@pytest.mark.parametrize("Hq,Hkv", W.DECODE_HEADS)
def test_decode_single_and_batched(hip, device, monkeypatch, Hq, Hkv, mode):
    """vis_decode_attn, split + combine (0) and streaming (2), G = 7, 4, 2: every context alone through the single-sequence
    form, then all of them as one batch."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    T = 512
    c = W.decode_case(Hq, Hkv, T, W.DECODE_CTXS)
    for b in range(len(c.ctxs)):
        out, kc, vc = _decode_launch(hip, device, c, T, [b], batched=False)
        _decode_check(c, [b], out, kc, vc, f"decode single mode {mode}")
    seqs = list(range(len(c.ctxs)))
    out, kc, vc = _decode_launch(hip, device, c, T, seqs, batched=True)
    _decode_check(c, seqs, out, kc, vc, f"decode batched mode {mode}")


@pytest.mark.parametrize("mode", ["0", "2"])
def test_decode_past_the_combine_preload(hip, device, monkeypatch, mode):
    """T = 4608, context 4161: active keys on both sides of key 4096 and in the last split - past the 64 splits the combine
    preloads."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    c = W.decode_case(8, 2, 4608, (4161,))
    assert all((u.s[:, 4096:] > W.BG).any() for u in c.units)
    out, kc, vc = _decode_launch(hip, device, c, 4608, [0], batched=False)
    _decode_check(c, [0], out, kc, vc, f"decode long mode {mode}")


def test_decode_shared_prefix(hip, device, monkeypatch):
    """vis_decode_attn_shared, P = 64 (streaming form at Hkv * B = 128): sequences b > 0 weight sequence 0's actives in the
    shared rows together with their own behind them."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", "1")
    c = W.shared_case()
    seqs = list(range(len(c.ctxs)))
    out, kc, vc = _decode_launch(hip, device, c, 512, seqs, batched=True, shared_len=W.SHARED_P)
    _decode_check(c, seqs, out, kc, vc, "decode shared")


@pytest.mark.parametrize("mode", ["0", "2"])
def test_decode_forked(hip, device, monkeypatch, mode):
    """vis_decode_attn_forked: the children's own copies of the parent's 64 rows are poison."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    c = W.shared_case(True)
    B = len(c.ctxs)
    fork = (torch.zeros(B, dtype=torch.int32, device=device),
            torch.tensor([0] + [W.SHARED_P] * (B - 1), dtype=torch.int32, device=device))
    seqs = list(range(B))
    out, kc, vc = _decode_launch(hip, device, c, 512, seqs, batched=True, fork=fork)
    _decode_check(c, seqs, out, kc, vc, f"decode forked mode {mode}")


@pytest.mark.parametrize("parts,mode", [("bf16", "0"), ("bf16", "2"), ("fp8", "0"), ("fp8", "2")])
def test_decode_parts(hip, device, monkeypatch, parts, mode):
    """vis_decode_attn_parts: the partial slab finalises to exactly the 8 e_d rows (one slab; unit scales in the fp8 form)."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    c = W.decode_case(28, 4, 512, W.DECODE_CTXS)
    seqs = list(range(len(c.ctxs)))
    out, kc, vc = _decode_launch(hip, device, c, 512, seqs, batched=True, parts=parts)
    _decode_check(c, seqs, out, kc, vc, f"decode parts {parts} mode {mode}")


@pytest.mark.parametrize("mode", ["0", "2"])
def test_decode_cross_attn(hip, device, monkeypatch, mode):
    """vis_decode_cross_attn and _batch, Tk = 448.  The q-norm runs inside: with eps = 1/2 and unit weights the raw query 8 e_d
    has mean square 1/2, rstd = rsqrt(1) and the normalised bf16 query is 8 e_d again (a 1-ulp rsqrt still rounds to 8)."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv, Tk = 32, 8, 448
    c = W.decode_case(Hq, Hkv, Tk, (1, 63, 64, 65, 200, 448), append=False, seed=3)
    B = len(c.ctxs)
    ns = -(-Tk // hip.DECODE_KEYS_PER_SPLIT)
    K, V = c.K.to(device), c.V.to(device)
    q = c.q.reshape(B, -1).to(torch.bfloat16).to(device)
    w = torch.ones(HD, dtype=torch.bfloat16, device=device)
    G = Hq // Hkv

    def verify(o, seqs, what):
        o = o.float().cpu()
        for j, b in enumerate(seqs):
            for kv in range(Hkv):
                W.check(c.units[b * Hkv + kv], o[j].reshape(Hq, HD)[kv * G:(kv + 1) * G].double().numpy(),
                        f"{what} mode {mode}: seq {b} nkeys {c.ctxs[b]} kv head {kv}")

    for b, n in enumerate(c.ctxs):
        po, pml = _nan(Hq * ns * HD, device), _nan(Hq * ns * 2, device)
        out = torch.full((Hq * HD,), float("nan"), dtype=torch.bfloat16, device=device)
        hip.decode_cross_attn(q[b].contiguous(), w, K[b].contiguous(), V[b].contiguous(),
                              torch.tensor([n - 1], dtype=torch.int32, device=device), po, pml, out, Hq, Hkv, HD, ns, W.SCALE, 0.5)
        verify(out[None], [b], "cross single")
    po, pml = _nan(B * Hq * ns * HD, device), _nan(B * Hq * ns * 2, device)
    out = torch.full((B, Hq * HD), float("nan"), dtype=torch.bfloat16, device=device)
    hip.decode_cross_attn_batch(q, w, K, V, torch.tensor([n - 1 for n in c.ctxs], dtype=torch.int32, device=device), po, pml, out,
                                Hq, Hkv, HD, ns, W.SCALE, 0.5)
    verify(out, list(range(B)), "cross batch")


def test_decode_draft_rows(hip, device):
    """vis_decode_attn_draft, R = 4 at step 62 (contexts 63 .. 66 straddle a split): row r weights cache keys, the rows 0 .. r - 1
    this launch appended and its own; the rows after it are poison in its direction."""
    c = W.draft_case()
    Hq, Hkv, T, R = 8, 2, 512, 4
    ns = T // hip.DECODE_KEYS_PER_SPLIT
    kc, vc = c.K.to(device), c.V.to(device)
    cos, sin = torch.ones((T, HD), device=device), torch.zeros((T, HD), device=device)
    po, pml = _nan(R * Hq * ns * HD, device), _nan(R * Hq * ns * 2, device)
    out = torch.full((R, Hq * HD), float("nan"), dtype=torch.bfloat16, device=device)
    hip.decode_attn_draft(c.qkv.to(device), cos, sin, kc, vc, torch.tensor([c.step], dtype=torch.int32, device=device), po, pml,
                          out, Hq, Hkv, HD, ns, W.SCALE)
    o = out.float().cpu()
    G = Hq // Hkv
    for r in range(R):
        for kv in range(Hkv):
            W.check(c.units[r * Hkv + kv], o[r].reshape(Hq, HD)[kv * G:(kv + 1) * G].double().numpy(), f"draft row {r} kv head {kv}")
        assert torch.equal(kc[:, c.step + r].float().cpu(), c.knew[r]) and torch.equal(vc[:, c.step + r].float().cpu(), c.vnew[r]), \
            f"draft row {r}: appended K / V row"
