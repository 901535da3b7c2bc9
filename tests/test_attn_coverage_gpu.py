"""Key coverage of every attention kernel: which keys each query attended, exactly, at tile, split, segment and cache edges.

Inputs come from tests/attn_needles.py: probe queries e_d, needle keys C e_d whose weights are exactly 1 (every other weight
underflows to 0 in f32), V rows of multiples of 1/8 that encode (key, sequence / request), and poison keys (C e_d, V = 4096)
everywhere a probe must not look.  A probe's output is then one V row or the exact mean of two / four, and each probe is
checked against a float64 softmax over exactly its valid keys to 1 bf16 ulp, plus |out| < 64 (no poison, no NaN from the
NaN-filled workspaces).  Outputs of non-probe rows are checked against the same float64 reference at the tolerances of
tests/test_kernels_gpu.py (their P is rounded to bf16 before P * V).
"""
import pytest
import torch

import attn_needles as N

pytestmark = pytest.mark.gpu

HD = 128
SCALE = HD ** -0.5
CTXS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _nan(n, device):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=device)


def _decode_edges(n):
    # 16-key steps, 64-key splits, the combine's 2 x CB_PRE = 64 preloaded splits (4096 keys), the last split / step
    return (16, 64, 128, 4096, (n - 1) // 64 * 64, (n - 1) // 16 * 16)


# ----------------------------------------------------------------------------- decode self-attention
def _decode_inputs(device, Hq, Hkv, T, ctxs, groups, shared_len=0, seed=0):
    """Caches [B, Hkv, T, D] + qkv [B, nq] for needle sets groups[b][h] (key rows < ctx[b]; ctx[b] - 1 = the appended key).
    Cache rows at and past ctx[b] - 1 (the slot the step overwrites: a stale row of a longer request) are poison."""
    B, G = len(ctxs), Hq // Hkv
    dirs = N.probe_dirs(G, HD)
    gen = torch.Generator(device=device).manual_seed(seed)
    K = N.background((B, Hkv, T, HD), gen, dirs)
    V = torch.empty((B, Hkv, T, HD), device=device)
    for b in range(B):
        for kv in range(Hkv):
            V[b, kv] = N.v_rows(torch.arange(T, device=device), HD, salt=b * Hkv + kv)
    knew = N.background((B, Hkv, HD), gen, dirs)
    vnew = torch.empty((B, Hkv, HD), device=device)
    for b, n in enumerate(ctxs):
        for h in range(Hq):
            kv, d = h // G, dirs[h % G]
            for p in groups[b][h]:
                assert 0 <= p < n
                if p == n - 1:
                    knew[b, kv, d] = N.C_NEEDLE
                else:
                    K[b, kv, p, d] = N.C_NEEDLE
        for kv in range(Hkv):
            vnew[b, kv] = N.v_rows(torch.tensor([n - 1], device=device), HD, salt=b * Hkv + kv)[0]
        K[b, :, n - 1:, dirs] = N.C_NEEDLE
        V[b, :, n - 1:] = N.POISON_V
    if shared_len:
        K[1:, :, :shared_len] = K[0:1, :, :shared_len]
        V[1:, :, :shared_len] = V[0:1, :, :shared_len]
    q = torch.zeros((B, Hq, HD), device=device)
    for h in range(Hq):
        q[:, h, dirs[h % G]] = 1.0
    qkv = torch.cat((q, knew, vnew), 1).reshape(B, -1).to(torch.bfloat16)
    return K.to(torch.bfloat16), V.to(torch.bfloat16), qkv, q, knew, vnew


def _decode_check(out, K, V, q, knew, vnew, ctxs, Hq, Hkv, what, kc_after=None, vc_after=None):
    G = Hq // Hkv
    out = out.reshape(len(ctxs), Hq, HD)
    N.assert_no_poison(out, what)
    for b, n in enumerate(ctxs):
        kr, vr = K[b, :, :n].float().clone(), V[b, :, :n].float().clone()
        kr[:, n - 1], vr[:, n - 1] = knew[b], vnew[b]
        for kv in range(Hkv):
            hs = slice(kv * G, (kv + 1) * G)
            valid = torch.ones((G, n), dtype=torch.bool, device=K.device)
            ref = N.attn_ref(q[b, hs], kr[kv], vr[kv], valid, SCALE)
            N.assert_within_ulp(out[b, hs], ref, f"{what}: seq {b} (ctx {n}) kv head {kv}")
        if kc_after is not None:
            assert torch.equal(kc_after[b, :, n - 1].float(), knew[b]) and torch.equal(vc_after[b, :, n - 1].float(), vnew[b]), \
                f"{what}: seq {b}: appended K / V row"


def _groups_for(ctxs, Hq, rot=0):
    return [[N.needle_groups(n, _decode_edges(n))[(h + rot * b) % len(N.needle_groups(n, _decode_edges(n)))]
             for h in range(Hq)] for b, n in enumerate(ctxs)]


def _run_decode(hip, device, Hq, Hkv, T, ctxs, groups, batched, shared_len=0):
    K, V, qkv, q, knew, vnew = _decode_inputs(device, Hq, Hkv, T, ctxs, groups, shared_len)
    B = len(ctxs)
    ns = T // hip.DECODE_KEYS_PER_SPLIT
    cos = torch.ones((T, HD), device=device)
    sin = torch.zeros((T, HD), device=device)
    po, pml = _nan(B * Hq * ns * HD, device), _nan(B * Hq * ns * 2, device)
    step = torch.tensor([n - 1 for n in ctxs], dtype=torch.int32, device=device)
    kc, vc = K.clone(), V.clone()
    if batched:
        out = torch.full((B, Hq * HD), float("nan"), dtype=torch.bfloat16, device=device)
        hip.decode_attn(qkv, cos.expand(B, -1, -1), sin.expand(B, -1, -1), kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, SCALE,
                        shared_len=shared_len)
    else:
        assert B == 1
        out = torch.full((Hq * HD,), float("nan"), dtype=torch.bfloat16, device=device)
        kc, vc = kc[0].contiguous(), vc[0].contiguous()
        hip.decode_attn(qkv[0].contiguous(), cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, SCALE)
        kc, vc = kc[None], vc[None]
    return out, (K, V, q, knew, vnew), kc, vc


@pytest.mark.parametrize("mode", ["0", "2"])
@pytest.mark.parametrize("T", [4608, 6144])
def test_decode_single_every_edge(hip, device, monkeypatch, mode, T):
    """One sequence, split + combine (0) and streaming (2): every context of CTXS plus T - 1 and T (the new key lands in the last
    cache row), each head with its own needle set (first / last / appended key, both sides of every 16-key step, 64-key split,
    the combine's 4096-key preload edge; two and four equal needles in different splits, one past split 64)."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv = 28, 4
    for n in CTXS + (T - 1, T):
        groups = _groups_for([n], Hq)
        ng = len(N.needle_groups(n, _decode_edges(n)))
        assert ng <= Hq, "every needle set of this context gets a head"
        out, (K, V, q, kn, vn), kc, vc = _run_decode(hip, device, Hq, Hkv, T, [n], groups, batched=False)
        _decode_check(out, K, V, q, kn, vn, [n], Hq, Hkv, f"decode single ctx {n} T {T} mode {mode}", kc, vc)


@pytest.mark.parametrize("mode,B", [("0", 16), ("2", 16), ("1", 32)])
@pytest.mark.parametrize("T", [4608, 6144])
def test_decode_batched_ragged_contexts(hip, device, monkeypatch, mode, B, T):
    """Batch of ragged contexts (CTXS + T - 1, T) in one launch: split + combine, forced streaming, and the natural choice at
    Hkv * B >= 128 (streaming).  V rows encode the sequence: a read of another sequence's rows shows."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv = 28, 4
    ctxs = [(CTXS + (T - 1, T))[i % 16] for i in range(B)]
    groups = _groups_for(ctxs, Hq, rot=5)
    out, (K, V, q, kn, vn), kc, vc = _run_decode(hip, device, Hq, Hkv, T, ctxs, groups, batched=True)
    _decode_check(out, K, V, q, kn, vn, ctxs, Hq, Hkv, f"decode batch {B} T {T} mode {mode}", kc, vc)


@pytest.mark.parametrize("mode", ["0", "2"])
def test_decode_gqa4_batched(hip, device, monkeypatch, mode):
    """The mllama self-attention grouping (32 / 8 heads) over the same edges."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv, T = 32, 8, 4608
    ctxs = list(CTXS + (T - 1, T))
    groups = _groups_for(ctxs, Hq, rot=3)
    out, (K, V, q, kn, vn), kc, vc = _run_decode(hip, device, Hq, Hkv, T, ctxs, groups, batched=True)
    _decode_check(out, K, V, q, kn, vn, ctxs, Hq, Hkv, f"decode gqa4 mode {mode}", kc, vc)


@pytest.mark.parametrize("mode", ["0", "2"])
def test_decode_rope_at_a_real_position(hip, device, monkeypatch, mode):
    """Real rope at the new token's position: q and k are given pre-rotated by the inverse angle, the kernel's rotation (f32,
    rounded to bf16) lands them near e_d; the reference rotates them the same way in float64 and rounds to bf16."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv, T, n = 28, 4, 4608, 4097
    singles = [g for g in N.needle_groups(n, _decode_edges(n)) if len(g) == 1]      # a rotated key's score is not exactly C
    groups = [[singles[h % len(singles)] for h in range(Hq)]]
    groups[0][0] = (n - 1,)                                  # the appended (rotated) key as a needle
    K, V, _, q, knew, vnew = _decode_inputs(device, Hq, Hkv, T, [n], groups)
    g = torch.Generator().manual_seed(11)
    ang = torch.rand((HD // 2,), generator=g) * 6.28
    cos, sin = torch.ones((T, HD), device=device), torch.zeros((T, HD), device=device)
    cos[n - 1] = torch.cat((ang, ang)).cos().to(device)
    sin[n - 1] = torch.cat((ang, ang)).sin().to(device)

    def unrotate(x):                                         # R^-1 x, rounded to bf16 (the projection's output)
        h = HD // 2
        c, s = cos[n - 1, :h], sin[n - 1, :h]
        a, b = x[..., :h], x[..., h:]
        return torch.cat((a * c + b * s, b * c - a * s), -1).to(torch.bfloat16).float()

    q_in, k_in = unrotate(q[0]), unrotate(knew[0])
    qkv = torch.cat((q_in, k_in, vnew[0]), 0).reshape(-1).to(torch.bfloat16)
    q_rot = N.rope_bf16(q_in, cos[n - 1], sin[n - 1])[None]
    k_rot = N.rope_bf16(k_in, cos[n - 1], sin[n - 1])[None]
    ns = T // hip.DECODE_KEYS_PER_SPLIT
    po, pml = _nan(Hq * ns * HD, device), _nan(Hq * ns * 2, device)
    step = torch.tensor([n - 1], dtype=torch.int32, device=device)
    kc, vc = K[0].clone(), V[0].clone()
    out = torch.full((Hq * HD,), float("nan"), dtype=torch.bfloat16, device=device)
    hip.decode_attn(qkv, cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, SCALE)
    N.assert_within_ulp(kc[:, n - 1], k_rot[0], "rotated appended key")
    _decode_check(out, K, V, q_rot, k_rot, vnew, [n], Hq, Hkv, f"decode rope mode {mode}")


@pytest.mark.parametrize("P", [64, 960])
def test_decode_shared_prefix_edges(hip, device, P):
    """shared_len = P (streaming form at Hkv * B >= 128): sequence 0 steps at P with its rows past P poisoned - the others must
    read them from their own copies; a needle at P - 1 in every copy (the shared prefix), a needle at P in sequences b > 0
    (their own row), needles on both sides of the other sequences' edges."""
    Hq, Hkv, T, B = 28, 4, 4608, 32
    others = [P + 1, P + 2, P + 16, P + 64, P + 65, 4095, 4096, 4097, T - 1, T]
    ctxs = [P + 1] + [others[i % len(others)] for i in range(B - 1)]
    groups = []
    for b, n in enumerate(ctxs):
        row = []
        for h in range(Hq):
            if b == 0:
                row.append((P - 1,) if h % 2 == 0 else (P,))       # P = sequence 0's appended key
            elif h % 2 == 0:
                row.append((P - 1, P) if h % 4 == 0 else (P - 1,))  # the shared row, + sequence b's own row P
            else:
                own = [g for g in N.needle_groups(n, _decode_edges(n) + (P,)) if min(g) >= P]
                row.append(own[(h + b) % len(own)])
        groups.append(row)
    out, (K, V, q, kn, vn), kc, vc = _run_decode(hip, device, Hq, Hkv, T, ctxs, groups, batched=True, shared_len=P)
    _decode_check(out, K, V, q, kn, vn, ctxs, Hq, Hkv, f"decode shared prefix {P}", kc, vc)


@pytest.mark.parametrize("fp8,mode,B", [(False, "0", 16), (False, "2", 16), (True, "0", 16), (False, "1", 32)])
def test_decode_attn_parts_edges(hip, device, monkeypatch, fp8, mode, B):
    """vis_decode_attn_parts with ksplit 1: the slab holds the wanted qkv row as f32 (bf16 partials: sum = the row; fp8 form
    with unit scales: sum * 1 * 1), so the finalised row is the needle row and the same edges apply."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv, T = 28, 4, 4608
    ctxs = [(CTXS + (T - 1, T))[i % 16] for i in range(B)]
    groups = _groups_for(ctxs, Hq, rot=2)
    K, V, qkv, q, knew, vnew = _decode_inputs(device, Hq, Hkv, T, ctxs, groups)
    nq = qkv.shape[1]
    rows = hip.part_rows(B)
    part = torch.full((rows * nq,), float("nan"), dtype=torch.float32, device=device)
    part.view(rows, nq)[:B] = qkv.float()
    sx = torch.ones(B, dtype=torch.float32, device=device) if fp8 else None
    sw = torch.ones(nq, dtype=torch.float32, device=device) if fp8 else None
    ns = T // hip.DECODE_KEYS_PER_SPLIT
    po, pml = _nan(B * Hq * ns * HD, device), _nan(B * Hq * ns * 2, device)
    step = torch.tensor([n - 1 for n in ctxs], dtype=torch.int32, device=device)
    cos = torch.ones((T, HD), device=device).expand(B, -1, -1)
    sin = torch.zeros((T, HD), device=device).expand(B, -1, -1)
    kc, vc = K.clone(), V.clone()
    out = torch.full((B, Hq * HD), float("nan"), dtype=torch.bfloat16, device=device)
    hip.decode_attn_parts(part, 1, cos, sin, kc, vc, step, po, pml, out, Hq, Hkv, HD, ns, SCALE, sx=sx, sw=sw)
    _decode_check(out, K, V, q, knew, vnew, ctxs, Hq, Hkv, f"decode parts fp8={fp8} mode {mode}", kc, vc)


# ----------------------------------------------------------------------------- decode cross-attention (mllama)
def _cross_inputs(device, Hq, Hkv, Tk, nkeys, rot, seed=1):
    B, G = len(nkeys), Hq // Hkv
    dirs = N.probe_dirs(G, HD)
    gen = torch.Generator(device=device).manual_seed(seed)
    K = N.background((B, Hkv, Tk, HD), gen, dirs)
    V = torch.empty((B, Hkv, Tk, HD), device=device)
    for b, n in enumerate(nkeys):
        for kv in range(Hkv):
            V[b, kv] = N.v_rows(torch.arange(Tk, device=device), HD, salt=100 + b * Hkv + kv)
        gs = N.needle_groups(n, _decode_edges(n))
        for h in range(Hq):
            for p in gs[(h + rot * b) % len(gs)]:
                K[b, h // G, p, dirs[h % G]] = N.C_NEEDLE
        K[b, :, n:, dirs] = N.C_NEEDLE
        V[b, :, n:] = N.POISON_V
    qraw = torch.zeros((B, Hq, HD), device=device)
    for h in range(Hq):
        qraw[:, h, dirs[h % G]] = 1.0
    w = (0.5 + torch.rand((HD,), generator=torch.Generator().manual_seed(seed))).to(torch.bfloat16).float().to(device)
    qn = N.qnorm_bf16(qraw, w, 1e-5)
    return K.to(torch.bfloat16), V.to(torch.bfloat16), qraw.to(torch.bfloat16), w.to(torch.bfloat16), qn


def _cross_check(out, K, V, qn, nkeys, Hq, Hkv, what):
    G = Hq // Hkv
    out = out.reshape(len(nkeys), Hq, HD)
    N.assert_no_poison(out, what)
    for b, n in enumerate(nkeys):
        for kv in range(Hkv):
            hs = slice(kv * G, (kv + 1) * G)
            assert N.log2_margin(N.C_NEEDLE, float(qn[b, hs].max(-1).values.min()), SCALE) > 150
            ref = N.attn_ref(qn[b, hs], K[b, kv, :n].float(), V[b, kv, :n].float(),
                             torch.ones((G, n), dtype=torch.bool, device=K.device), SCALE)
            N.assert_within_ulp(out[b, hs], ref, f"{what}: seq {b} nkeys {n} kv head {kv}")


def _nkeys_for(Tk):
    return [n for n in (1, 63, 64, 65, 4096, 4097) if n < Tk] + [Tk]


@pytest.mark.parametrize("mode", ["0", "2"])
@pytest.mark.parametrize("Tk", [448, 6464])
def test_decode_cross_attn_single_nkeys_edges(hip, device, monkeypatch, mode, Tk):
    """vis_decode_cross_attn (one token): static keys, q-norm inside; keys at and past nkeys are poison."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv = 32, 8
    ns = -(-Tk // hip.DECODE_KEYS_PER_SPLIT)
    for n in _nkeys_for(Tk):
        K, V, q, w, qn = _cross_inputs(device, Hq, Hkv, Tk, [n], rot=0)
        po, pml = _nan(Hq * ns * HD, device), _nan(Hq * ns * 2, device)
        out = torch.full((Hq * HD,), float("nan"), dtype=torch.bfloat16, device=device)
        hip.decode_cross_attn(q[0].reshape(-1).contiguous(), w, K[0].contiguous(), V[0].contiguous(),
                              torch.tensor([n - 1], dtype=torch.int32, device=device), po, pml, out, Hq, Hkv, HD, ns, SCALE, 1e-5)
        _cross_check(out, K, V, qn, [n], Hq, Hkv, f"cross single Tk {Tk} mode {mode}")


@pytest.mark.parametrize("mode", ["0", "2"])
@pytest.mark.parametrize("Tk", [448, 6464])
def test_decode_cross_attn_batch_nkeys_edges(hip, device, monkeypatch, mode, Tk):
    """vis_decode_cross_attn_batch: every sequence its own keys and key count (V rows encode the sequence)."""
    monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", mode)
    Hq, Hkv = 32, 8
    nkeys = _nkeys_for(Tk) * 2
    B = len(nkeys)
    ns = -(-Tk // hip.DECODE_KEYS_PER_SPLIT)
    K, V, q, w, qn = _cross_inputs(device, Hq, Hkv, Tk, nkeys, rot=3)
    po, pml = _nan(B * Hq * ns * HD, device), _nan(B * Hq * ns * 2, device)
    out = torch.full((B, Hq * HD), float("nan"), dtype=torch.bfloat16, device=device)
    hip.decode_cross_attn_batch(q.reshape(B, -1).contiguous(), w, K, V, torch.tensor([n - 1 for n in nkeys], dtype=torch.int32,
                                device=device), po, pml, out, Hq, Hkv, HD, ns, SCALE, 1e-5)
    _cross_check(out, K, V, qn, nkeys, Hq, Hkv, f"cross batch Tk {Tk} mode {mode}")


# ----------------------------------------------------------------------------- prefill
def _seg_valid(segments, causal, T, device):
    """valid(pos [n]) -> bool [n, T]: same segment (and key <= query when causal)."""
    seg = torch.full((T,), -1, dtype=torch.int64, device=device)
    for i, sg in enumerate(segments):
        seg[sg[0]:sg[1]] = i
    keys = torch.arange(T, device=device)

    def valid(pos):
        pos = torch.as_tensor(pos, device=device)
        v = seg[pos][:, None] == seg[None, :]
        return v & (keys[None, :] <= pos[:, None]) if causal else v
    return valid


def _probe_plan(segments, causal, cap, lo=0):
    """Probe positions (>= lo): each segment's first and last row and the first / last rows of its 64- and 128-row tiles, the
    diagonal of causal rows; never two adjacent rows (a causal probe's next key is its poison)."""
    pri = []
    for sg in segments:
        s, e = sg[0], sg[1]
        pri += [max(s, lo), e - 1]
    for sg in segments:
        s, e = sg[0], sg[1]
        for t in range(s + 64, e, 64):
            pri += [t, t - 1]
    rows = []
    for r in pri:
        if r >= lo and r not in rows and all(abs(r - x) > 1 for x in rows) and len(rows) < cap:
            rows.append(r)
    return rows


def _prefill_inputs(device, Hq, Hkv, D, T, pos, probe_pos, segments, causal, valid, seed, salt=0, extra_edges=()):
    """Q [Hq, S, D] for query positions pos, K / V [Hkv, T, D]; probe i at position probe_pos[i]: head h = direction
    dirs[i G + h % G] with its needle set, every key its row must not see poisoned in that direction."""
    G = Hq // Hkv
    dirs = N.probe_dirs(len(probe_pos) * G, D)
    gen = torch.Generator(device=device).manual_seed(seed)
    needles, poison, expect_groups = {}, {}, []
    vm = valid(probe_pos).cpu()
    for i, r in enumerate(probe_pos):
        keys = torch.nonzero(vm[i]).flatten().tolist()
        k0, n = keys[0], len(keys)
        assert keys == list(range(k0, k0 + n))
        gs = N.needle_groups(n, (16, 32, 64, 128, (n - 1) // 64 * 64, (n - 1) // 32 * 32) + tuple(x - k0 for x in extra_edges))
        for g in range(G):
            grp = tuple(k0 + p for p in gs[(i * 3 + g) % len(gs)])
            needles[dirs[i * G + g]] = grp
            poison[dirs[i * G + g]] = torch.nonzero(~vm[i]).flatten().tolist()
    K, V = zip(*[N.build_keys(T, D, dirs, needles, poison, gen, salt=salt * Hkv + kv) for kv in range(Hkv)])
    K, V = torch.stack(K), torch.stack(V)
    Q = N.background((Hq, len(pos), D), gen, dirs)
    row_of = {p: j for j, p in enumerate(pos)}
    for i, r in enumerate(probe_pos):
        j = row_of[r]
        Q[:, j] = 0.0
        for h in range(Hq):
            Q[h, j, dirs[i * G + h % G]] = 1.0
    return Q.to(torch.bfloat16), K.to(torch.bfloat16), V.to(torch.bfloat16)


def _vt(hip, V, device):
    T = V.shape[-2]
    ld = (T + 63) // 64 * 64
    vt = torch.zeros(V.shape[:-2] + (V.shape[-1], ld), dtype=torch.bfloat16, device=device)
    vt[..., :T] = V.transpose(-1, -2)
    return vt[..., hip.vt_key_order(ld, device)].contiguous()


def _prefill_check(out, Q, K, V, pos, probe_pos, valid, what, full_heads=None):
    """Probe rows, every head: float64 reference to 1 bf16 ulp and no poison; heads full_heads, every row: the float64
    reference at the tolerances of test_kernels_gpu (non-probe rows round P to bf16)."""
    Hq, S, D = Q.shape
    G = Hq // K.shape[0]
    scale = D ** -0.5
    o = out.reshape(S, Hq, D)
    row_of = {p: j for j, p in enumerate(pos)}
    rows = [row_of[r] for r in probe_pos]
    vm = valid(probe_pos)
    for h in range(Hq):
        got = o[rows, h]
        N.assert_no_poison(got, f"{what}: head {h}")
        ref = N.attn_ref(Q[h, rows], K[h // G].float(), V[h // G].float(), vm, scale)
        N.assert_within_ulp(got, ref, f"{what}: probe rows {probe_pos} head {h}")
    vall = valid(pos)
    for h in (full_heads if full_heads is not None else (0, Hq - 1)):
        ref = N.attn_ref(Q[h], K[h // G].float(), V[h // G].float(), vall, scale)
        err = (o[:, h].double() - ref).abs()
        bad = err > 2e-2 + 2e-2 * ref.abs()
        assert not bad.any(), f"{what}: head {h}: {int(bad.sum())} elements out of tolerance, max err {float(err.max())}"


SMALL_S = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)


@pytest.mark.parametrize("causal", [True, False])
def test_prefill_d128_every_length(hip, device, causal):
    """attn_prefill, head_dim 128 (GQA 4 / 2): every S of SMALL_S, probes on the first / last rows of the 64-key tiles and
    128-row blocks, needles on the diagonal, at the first key and either side of every tile edge."""
    Hq, Hkv, D = 4, 2, 128
    for S in SMALL_S:
        segs = [(0, S)]
        valid = _seg_valid(segs, causal, S, device)
        probes = _probe_plan(segs, causal, cap=D // (Hq // Hkv))
        Q, K, V = _prefill_inputs(device, Hq, Hkv, D, S, list(range(S)), probes, segs, causal, valid, seed=S)
        out = torch.full((S, Hq * D), float("nan"), dtype=torch.bfloat16, device=device)
        hip.attn_prefill(Q, K, _vt(hip, V, device), out, hip.make_attn_work(segs, causal, device, heads=Hq), causal, D ** -0.5)
        _prefill_check(out, Q, K, V, list(range(S)), probes, valid, f"prefill d128 S {S} causal {causal}")


@pytest.mark.parametrize("causal", [True, False])
def test_prefill_d128_llm_length(hip, device, causal):
    """S = 2249 at the production head count (28 / 4)."""
    Hq, Hkv, D, S = 28, 4, 128, 2249
    segs = [(0, S)]
    valid = _seg_valid(segs, causal, S, device)
    probes = _probe_plan(segs, causal, cap=D // (Hq // Hkv))
    Q, K, V = _prefill_inputs(device, Hq, Hkv, D, S, list(range(S)), probes, segs, causal, valid, seed=7)
    out = torch.full((S, Hq * D), float("nan"), dtype=torch.bfloat16, device=device)
    hip.attn_prefill(Q, K, _vt(hip, V, device), out, hip.make_attn_work(segs, causal, device, heads=Hq), causal, D ** -0.5)
    _prefill_check(out, Q, K, V, list(range(S)), probes, valid, f"prefill d128 S {S} causal {causal}")


D80_CASES = [(S, 2, [(0, S)]) for S in SMALL_S] + [
    (356, 4, [(0, 100), (100, 356)]),                        # unaligned segment edge
    (320, 4, [(i * 64, (i + 1) * 64) for i in range(5)]),    # 64-row windows
    (4900, 16, [(0, 4900)]),
    (6432, 3, [(0, 6404), (6404, 6432)]),
]


@pytest.mark.parametrize("S,H,segs", D80_CASES)
def test_prefill_d80_segments_and_windows(hip, device, S, H, segs):
    """attn_prefill, head_dim 80, non-causal (the ViT kernel): every S of SMALL_S, unaligned segments, 64-row windows, the
    Qwen ViT length and the mllama canvas; keys of the other segments / windows are poison."""
    D = 80
    valid = _seg_valid(segs, False, S, device)
    probes = _probe_plan(segs, False, cap=min(24, D))
    Q, K, V = _prefill_inputs(device, H, H, D, S, list(range(S)), probes, segs, False, valid, seed=S + 1)
    out = torch.full((S, H * D), float("nan"), dtype=torch.bfloat16, device=device)
    hip.attn_prefill(Q, K, _vt(hip, V, device), out, hip.make_attn_work(segs, False, device, heads=H), False, D ** -0.5)
    _prefill_check(out, Q, K, V, list(range(S)), probes, valid, f"prefill d80 S {S} segments {len(segs)}")


@pytest.mark.parametrize("S,H", [(3200, 3), (4900, 16)])
def test_prefill_plan_key_split_halves(hip, device, S, H):
    """attn_prefill_plan with key-split items (two workgroups over the two key halves, the later one merges): probes in split
    blocks hold equal needles in both halves (the merge must give their exact mean) and needles either side of the cut."""
    D = 80
    segs = [(0, S)]
    plan = hip.make_vit_attn_plan(segs, device, H)
    assert plan.n_pairs > 0
    mid = (S // 2 + 32) // 64 * 64
    w = plan.work.cpu()
    split_rows = [int(it[0]) for it in w if int(it[1]) >> 8]
    assert split_rows
    valid = _seg_valid(segs, False, S, device)
    probes = list(dict.fromkeys([split_rows[0], split_rows[-1] + 64, split_rows[0] + 127, 0, S - 1, mid - 1, mid]))
    Q, K, V = _prefill_inputs(device, H, H, D, S, list(range(S)), probes, segs, False, valid, seed=31, extra_edges=(mid,))
    # equal needles in both key halves for the first two probes (rows of split blocks)
    dirs = N.probe_dirs(len(probes), D)
    for i in range(2):
        d = dirs[i]
        Kf = K.float()
        Kf[:, :, d] = 0.0
        for p in ((mid - 1, mid) if i == 0 else (5, mid - 64, mid + 64, S - 2)):
            Kf[:, p, d] = N.C_NEEDLE
        K = Kf.to(torch.bfloat16)
    out = torch.full((S, H * D), float("nan"), dtype=torch.bfloat16, device=device)
    hip.attn_prefill_plan(Q, K, _vt(hip, V, device), out, plan, D ** -0.5)
    _prefill_check(out, Q, K, V, list(range(S)), probes, valid, f"key-split plan S {S}")


@pytest.mark.parametrize("P,S", [(100, 357), (960, 1289), (65, 66)])
def test_prefill_rows_and_pairs_row_offset(hip, device, P, S):
    """attn_prefill with q_row0 = P (not a multiple of 64; rows P.. of a causal pass over keys 0..) and attn_prefill_pairs
    over the same rows: the causal diagonal sits at P + row."""
    Hq, Hkv, D = 4, 2, 128
    segs = [(0, S)]
    valid = _seg_valid(segs, True, S, device)
    pos = list(range(P, S))
    probes = _probe_plan(segs, True, cap=D // 2, lo=P)
    Q, K, V = _prefill_inputs(device, Hq, Hkv, D, S, pos, probes, segs, True, valid, seed=P)
    vt = _vt(hip, V, device)
    items = [(q0, min(128, S - q0), 0, S) for q0 in range(P, S, 128)]
    work = torch.tensor(items, dtype=torch.int32, device=device).reshape(-1, 4).contiguous()
    out = torch.full((S - P, Hq * D), float("nan"), dtype=torch.bfloat16, device=device)
    hip.attn_prefill(Q, K, vt, out, work, True, D ** -0.5, q_row0=P)
    _prefill_check(out, Q, K, V, pos, probes, valid, f"prefill rows q_row0 {P}")
    out2 = torch.full_like(out, float("nan"))
    hip.attn_prefill_pairs(Q, K, vt, out2, hip.make_attn_pairs(P, S, device), D ** -0.5, q_row0=P)
    _prefill_check(out2, Q, K, V, pos, probes, valid, f"prefill pairs q_row0 {P}")


@pytest.mark.parametrize("S", [17, 129, 257, 2249])
def test_prefill_pairs_from_row_zero(hip, device, S):
    Hq, Hkv, D = 28, 4, 128
    segs = [(0, S)]
    valid = _seg_valid(segs, True, S, device)
    probes = _probe_plan(segs, True, cap=D // 7)
    Q, K, V = _prefill_inputs(device, Hq, Hkv, D, S, list(range(S)), probes, segs, True, valid, seed=S + 3)
    out = torch.full((S, Hq * D), float("nan"), dtype=torch.bfloat16, device=device)
    hip.attn_prefill_pairs(Q, K, _vt(hip, V, device), out, hip.make_attn_pairs(0, S, device), D ** -0.5)
    _prefill_check(out, Q, K, V, list(range(S)), probes, valid, f"prefill pairs S {S}")


@pytest.mark.parametrize("pairs,causal", [(False, False), (False, True), (True, True)])
def test_prefill_many_requests(hip, device, pairs, causal):
    """attn_prefill_many / attn_prefill_pairs_many: k requests in one launch, each over its own cache block (kv_off) with its own
    key count; V rows encode the request, the other requests' blocks hold their own needles."""
    Hq, Hkv, D, S, T, k = 8, 2, 128, 200, 640, 3
    P = 64 if pairs else 0
    nkeys = [P + S if (pairs or causal) else n for n in (200, 457, 640)]
    slots = [2, 0, 3]
    kc = torch.zeros((4, Hkv, T, D), dtype=torch.bfloat16, device=device)
    ld = (T + 63) // 64 * 64
    vt = torch.zeros((k, Hkv, D, ld), dtype=torch.bfloat16, device=device)
    q = torch.zeros((k, Hq, S, D), dtype=torch.bfloat16, device=device)
    cases = []
    for j in range(k):
        segs = [(0, nkeys[j])] if not causal else [(0, P + S)]
        valid = _seg_valid(segs, causal, T, device)
        pos = list(range(P, P + S))
        probes = _probe_plan([(P, P + S)], causal, cap=D // 4, lo=P)
        Qj, Kj, Vj = _prefill_inputs(device, Hq, Hkv, D, T, pos, probes, segs, causal, valid, seed=90 + j, salt=j + 1)
        q[j], kc[slots[j]], vt[j] = Qj, Kj, _vt(hip, Vj, device)
        cases.append((Qj, Kj, Vj, pos, probes, valid))
    kv_off = [s * kc.stride(0) for s in slots]
    out = torch.full((k * S, Hq * D), float("nan"), dtype=torch.bfloat16, device=device)
    if pairs:
        hip.attn_prefill_pairs_many(q, kc, vt, out, hip.make_attn_pairs(P, P + S, device), D ** -0.5, kv_off, T, q_row0=P)
    else:
        items = [[(q0, min(128, S - q0), 0, nkeys[j]) for q0 in range(0, S, 128)] for j in range(k)]
        work = torch.tensor(items, dtype=torch.int32, device=device).reshape(k, -1, 4).contiguous()
        hip.attn_prefill_many(q, kc, vt, out, work, causal, D ** -0.5, kv_off, T)
    for j, (Qj, Kj, Vj, pos, probes, valid) in enumerate(cases):
        _prefill_check(out[j * S:(j + 1) * S], Qj, Kj, Vj, pos, probes, valid, f"many request {j} pairs {pairs} causal {causal}")
