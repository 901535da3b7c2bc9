"""Exact operands for the single-row (and 1..4-row) GEMV tests: inputs for which an f32 sum is exact in ANY order, so the
kernels (vis_gemv_bf16 / _rows / _argmax, vis_gemv_fp8w / _rows) must give the float64 result bit for bit and one dropped,
doubled or misplaced 16-byte chunk shows as a wrong integer.

* bf16 weights: x and W are integers in [-8, 8]; every partial sum in any order is an integer bounded by
  sum_k |w x| <= 64 K < 2^24 (K <= 30720).
* fp8 weights: W bytes are the 50 e4m3 codes whose values are multiples of 1/4 with |w| <= 8 (steps of 1/4 up to 4 and of 1/2 up
  to 8 - e4m3 has three mantissa bits - in both signs, both zeros included), x is an
  integer in [-4, 4], per-row scales are 2^-2 .. 2^2 (period 5 in the row index); in units of 1/4 every partial sum is at
  most 128 K < 2^24.
* bias and residual are multiples of 1/4 in [-3, 3]; the builders ASSERT on the actual operands that the bound holds
  (`(|W| @ |x|).max() < 2^24` in the right unit) and that every stage of the epilogue `(sum * scale + bias) + R` is exact
  in f32, and that the weight draw uses every allowed value (as many of them as the matrix has elements).
* SwiGLU: gate rows have one or two non-zeros on columns where x = +-1 and sum (times the scale) to -2 .. 2; up rows are
  dense, with eight of those columns adjusted so that the up sum of output i is non-zero and congruent to i modulo 32 (in
  units of 1, fp8: 1/4): any 32 consecutive outputs have different up values, so a wrong gate-up pairing or output index is
  off by far more than the one bf16 ulp silu_fast is allowed.
* fused RMSNorm: x = +-c with c a power of two and integer norm weights, so that the staged row is sign * norm_w exactly
  whatever rsqrtf's last bit (`norm_operands`, shared with tests/mxfp4_exact.py).
* `walk` restates the kernels' task walk (p_begin / p_end, nseg, the A / B register ring) so that the CPU tests can check
  that every shape reaches the edge it was chosen for.

CPU only: float64 torch, never the library under test.
"""
import functools

import numpy as np
import torch

SENTINEL = 7.0
NAN_BF16 = 0x7FC1
NAN_E4M3 = 0x7F
K_MAX = 30720            # the launchers' limit (60 KiB of bf16 in LDS) = GV_STAGE_MAX * 256 * 8

# (N, K): the edge each shape reaches is stated in tests/test_gemv_exact_gpu.py and checked in tests/test_gemv_exact.py
BF16_SHAPES = [(1, 8), (7, 704), (6, 4096), (6, 4104), (5, 18944), (6, 30720), (1001, 256), (8202, 4104), (16400, 64),
               (24583, 64)]
BF16_SWIGLU_SHAPES = [(32, 64), (1440, 520), (16448, 64)]
FP8_SHAPES_2x8 = [(1, 16), (7, 1424), (6, 8192), (6, 8208), (5, 18944), (6, 30720), (1001, 256)]
FP8_SHAPES_4x4 = [(8197, 64), (8198, 4112), (16402, 128), (40962, 64)]
FP8_SHAPES = FP8_SHAPES_2x8 + FP8_SHAPES_4x4
FP8_SWIGLU_SHAPES = [(64, 256), (16448, 64)]
ROWS_BF16_SHAPES = [(7, 704), (6, 4104)]
ROWS_FP8_SHAPES = [(7, 1424), (8197, 64)]
ARGMAX_SHAPES = [(1001, 256), (8203, 64)]
PICK_K = [4104, 520]
ONE_HOT_SHAPE = (6, 4104)
ONE_HOT_K = [0, 7, 8, 511, 512, 4095, 4096, 4103]
PADDED_MAX_N = 1001      # shapes up to this N repeat with a padded weight (ldw > K)


# ----------------------------------------------------------------------------- the kernels' task walk, restated
def grid_blocks(n_units):
    """Workgroups of gemv_bf16_launch / gemv_fp8w_launch for n_units row pairs (fp8: row groups)."""
    blocks = (n_units + 3) // 4
    if blocks > 1024:
        blocks = 1024 + (blocks - 1024) // 8
    return min(blocks, 2048)


def fp8_task_shape(N, K, swiglu=False):
    """(ROWS, SEG) gemv_fp8w_launch picks (VIS_GEMV8_SHAPE unset)."""
    n_out = N // 2 if swiglu else N
    return (2, 8) if (K >= 8192 or n_out <= 8192) else (4, 4)


def walk(kind, N, K, swiglu=False):
    """The task walk of one launch.  kind "bf16": a unit is a row pair, a weight chunk 8 elements, 8 chunks per lane and
    segment; "fp8": a unit is ROWS rows (SwiGLU: ROWS / 2 outputs), a chunk 16 elements, SEG chunks per lane and segment.
    Returns a dict: rows (per unit), n_units, blocks, nch, nseg, tail_chunks (live chunks of the last segment),
    begin [n_waves + 1] (wave w owns units begin[w] .. begin[w + 1]), max_units (per wave), idle_waves and crossings: the
    ring buffers a wave goes through from the last segment of one unit to the first segment of its next ("AB", "BA")."""
    if kind == "bf16":
        rows, seg, nch = 2, 8, K // 8
        n_units = N // 2 if swiglu else (N + 1) // 2
    else:
        rows, seg = fp8_task_shape(N, K, swiglu)
        nch = K // 16
        n_out = N // 2 if swiglu else N
        n_units = n_out // (rows // 2) if swiglu else (n_out + rows - 1) // rows
    blocks = grid_blocks(n_units)
    n_waves = blocks * 4
    nseg = ((nch + 63) // 64 + seg - 1) // seg
    begin = np.arange(n_waves + 1, dtype=np.int64) * n_units // n_waves
    per = np.diff(begin)
    crossings = set()
    for j in range(1, int(per.max())):
        crossings.add("AB"[(j * nseg - 1) % 2] + "AB"[(j * nseg) % 2])
    return dict(rows=rows, seg=seg, n_units=n_units, blocks=blocks, nch=nch, nseg=nseg,
                tail_chunks=nch - (nseg - 1) * seg * 64, begin=begin, max_units=int(per.max()), crossings=crossings,
                idle_waves=int((per == 0).sum()))


def unit_wave(w, unit):
    """Global wave index (4 per workgroup) that owns `unit`."""
    return int(np.searchsorted(w["begin"], unit, side="right") - 1)


# ----------------------------------------------------------------------------- number formats
E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().double()      # value of every byte
E4M3_FINITE = [b for b in range(256) if b not in (0x7F, 0xFF)]
_q = E4M3 * 4
FP8_CODES = torch.tensor([b for b in E4M3_FINITE if abs(float(E4M3[b])) <= 8 and float(_q[b]) == int(_q[b])], dtype=torch.uint8)
assert FP8_CODES.numel() == 50 and 0x80 in FP8_CODES.tolist()         # 24 magnitudes x 2 signs + the two zeros
BF16_VALUES = torch.arange(-8, 9, dtype=torch.float64)


def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (float64 tensor)."""
    e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))[1] - 1
    return torch.ldexp(torch.ones_like(ref), e - 7)


def _exact_f32(t, what):
    assert torch.equal(t, t.float().double()), f"{what} is not exact in f32"
    return t


def _draw(values, shape, rng):
    """Uniform draw from `values` with every value forced in at least once (as many as there are elements)."""
    n = int(np.prod(shape))
    idx = rng.integers(0, len(values), n)
    m = min(n, len(values))
    idx[rng.permutation(n)[:m]] = rng.permutation(len(values))[:m]
    out = values[torch.from_numpy(idx)].reshape(shape)
    assert len(torch.unique(out)) == m, "the draw does not use every allowed value"
    return out


def _matvec(w, x):
    """w [N, K] @ x [B, K]^T -> [B, N] in float64, by row blocks (w may be bf16 / f32 / f64)."""
    xd = x.double().t().contiguous()
    return torch.cat([w[i:i + 2048].double() @ xd for i in range(0, w.shape[0], 2048)]).t().contiguous()


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _quarters(shape, rng):
    return torch.from_numpy(rng.integers(-12, 13, shape).astype(np.float64)) / 4


def _epilogue(acc, scale, bias, R):
    """(sum * scale + bias) + R in float64, every stage asserted exact in f32."""
    v = _exact_f32(acc * scale[None, :] if scale is not None else acc, "sum * scale")
    v = _exact_f32(v + bias[None, :], "+ bias")
    return _exact_f32(v + R, "+ residual")


# ----------------------------------------------------------------------------- plain cases
@functools.lru_cache(maxsize=None)
def bf16_case(N, K, B=1):
    """dict: x [B, K] bf16, W [N, K] bf16, bias [N] bf16, R [B, N] bf16, ref [B, N] float64 (no epilogue),
    ref_br [B, N] float64 (with bias and residual)."""
    rng = _rng(1, N, K, B)
    w = _draw(BF16_VALUES, (N, K), rng).to(torch.bfloat16)
    x = _draw(BF16_VALUES, (B, K), rng)
    assert float(_matvec(w.float().abs(), x.abs()).max()) < 2 ** 24         # any partial sum, any order
    acc = _matvec(w, x)
    bias, R = _quarters((N,), rng), _quarters((B, N), rng)
    return dict(x=x.to(torch.bfloat16), W=w, bias=bias.to(torch.bfloat16), R=R.to(torch.bfloat16),
                ref=_exact_f32(acc, "sum"), ref_br=_epilogue(acc, None, bias, R))


def fp8_scales(N):
    return torch.ldexp(torch.ones(N, dtype=torch.float64), (torch.arange(N) * 3 + 1) % 5 - 2)


@functools.lru_cache(maxsize=None)
def fp8_case(N, K, B=1):
    """As bf16_case, with Wq [N, K] uint8 (e4m3 codes), scale [N] f32; ref = (Wq x) * scale."""
    rng = _rng(2, N, K, B)
    wq = _draw(FP8_CODES, (N, K), rng)
    deq = E4M3[wq.long()]
    x = _draw(torch.arange(-4, 5, dtype=torch.float64), (B, K), rng)
    assert float(_matvec(deq.abs(), x.abs()).max()) * 4 < 2 ** 24          # in units of 1/4
    acc = _matvec(deq, x)
    scale = fp8_scales(N)
    assert len(torch.unique(scale)) == min(N, 5)
    bias, R = _quarters((N,), rng), _quarters((B, N), rng)
    zero = torch.zeros_like(bias)
    return dict(x=x.to(torch.bfloat16), Wq=wq, deq=deq, scale=scale.float(), bias=bias.to(torch.bfloat16),
                R=R.to(torch.bfloat16), ref=_epilogue(acc, scale, zero, torch.zeros_like(R)),
                ref_br=_epilogue(acc, scale, bias, R))


def padded(w, pad):
    """[N, K] -> the [:, :K] view of a [N, K + pad] buffer whose padding holds NaN (bf16) / the e4m3 NaN byte."""
    N, K = w.shape
    if w.dtype == torch.bfloat16:
        wide = torch.full((N, K + pad), NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    else:
        wide = torch.full((N, K + pad), NAN_E4M3, dtype=torch.uint8)
    wide[:, :K] = w
    return wide


# ----------------------------------------------------------------------------- exact RMSNorm prologue
NORM_EPS = 1e-6


def norm_operands(K, B, rng):
    """Operands for which the fused RMSNorm prologue (gv_stage_x_rmsnorm) stages an EXACT row: x[b, k] = +-c_b with c_b a
    power of two (1, 2, 1/2, 4 by row), norm_w integers in [-8, 8] (zeros included).  The sum of squares K c^2 is exact in
    any order (every partial sum is n c^2, n <= K < 2^24), so is the division by K; rstd = rsqrt(c^2 + eps) misses 1 / c by
    eps / 2 c^3 and a few f32 ulps, so x * rstd is +-1 up to far less than half a bf16 ulp (2^-9 below 1) - proved here in
    float64 with 16 f32 ulps of slack for rsqrtf, the division and the product - and the staged row is sign * norm_w exactly.
    Returns x [B, K] bf16, norm_w [K] bf16, staged [B, K] float64 (pairwise different sign patterns)."""
    c = torch.tensor([1.0, 2.0, 0.5, 4.0], dtype=torch.float64)[torch.arange(B) % 4]
    while True:
        sign = torch.from_numpy(rng.integers(0, 2, (B, K)) * 2.0 - 1)
        if len({r.numpy().tobytes() for r in sign}) == B:
            break
    nw = _draw(BF16_VALUES, (K,), rng)
    x = sign * c[:, None]
    ssq = (x * x).sum(1)
    assert K < 2 ** 24 and torch.equal(ssq, K * c * c) and torch.equal((ssq.float() / float(K)).double(), c * c)
    eps32 = float(np.float32(NORM_EPS))
    rstd = 1.0 / torch.sqrt((c * c + eps32).float().double())       # the f32 argument, then float64
    off = (c * rstd - 1.0).abs() + 16 * 2.0 ** -24
    assert float(off.max()) < 2.0 ** -12, "x * rstd could leave the bf16 rounding interval of +-1"
    assert torch.equal((x * rstd[:, None]).to(torch.bfloat16).double(), sign)
    staged = sign * nw[None, :]
    assert torch.equal(staged.to(torch.bfloat16).double(), staged)
    return x.to(torch.bfloat16), nw.to(torch.bfloat16), staged


@functools.lru_cache(maxsize=None)
def bf16_norm_case(N, K, B=1):
    """bf16_case behind the exact RMSNorm prologue: ref / ref_br = W @ (sign * norm_w) (+ bias + R), float64."""
    rng = _rng(6, N, K, B)
    w = _draw(BF16_VALUES, (N, K), rng).to(torch.bfloat16)
    x, nw, staged = norm_operands(K, B, rng)
    assert float(_matvec(w.float().abs(), staged.abs()).max()) < 2 ** 24
    acc = _matvec(w, staged)
    bias, R = _quarters((N,), rng), _quarters((B, N), rng)
    return dict(x=x, norm_w=nw, W=w, bias=bias.to(torch.bfloat16), R=R.to(torch.bfloat16), ref=_exact_f32(acc, "sum"),
                ref_br=_epilogue(acc, None, bias, R))


@functools.lru_cache(maxsize=None)
def fp8_norm_case(N, K, B=1):
    """fp8_case behind the exact RMSNorm prologue."""
    rng = _rng(7, N, K, B)
    wq = _draw(FP8_CODES, (N, K), rng)
    deq = E4M3[wq.long()]
    x, nw, staged = norm_operands(K, B, rng)
    assert float(_matvec(deq.abs(), staged.abs()).max()) * 4 < 2 ** 24
    acc = _matvec(deq, staged)
    scale = fp8_scales(N)
    bias, R = _quarters((N,), rng), _quarters((B, N), rng)
    zero = torch.zeros_like(bias)
    return dict(x=x, norm_w=nw, Wq=wq, scale=scale.float(), bias=bias.to(torch.bfloat16), R=R.to(torch.bfloat16),
                ref=_epilogue(acc, scale, zero, torch.zeros_like(R)), ref_br=_epilogue(acc, scale, bias, R))


BF16_NORM_SHAPE = (6, 4104)      # 513 x-chunks: the re-reading loop of gv_stage_x_rmsnorm<false> (more than 512 chunks)
FP8_NORM_SHAPE = (6, 8208)       # 1026 x-chunks: five passes of that loop


# ----------------------------------------------------------------------------- f32 evaluation in a given order
def f32_sum(w, x, chunk, reverse):
    """sum_k w[:, k] x[k] accumulated in f32, one product at a time: forward, or with the `chunk`-element chunks taken last
    to first.  w [N, K] and x [K] hold the VALUES (any float dtype)."""
    wt = np.ascontiguousarray(w.float().numpy().T)
    xv = x.float().numpy()
    order = np.arange(wt.shape[0]).reshape(-1, chunk)
    if reverse:
        order = order[::-1]
    acc = np.zeros(wt.shape[1], dtype=np.float32)
    for k in order.reshape(-1):
        acc += wt[k] * xv[k]
    assert acc.dtype == np.float32
    return torch.from_numpy(acc).double()


# ----------------------------------------------------------------------------- SwiGLU
def interleave16(gate, up):
    """[I, K] x 2 -> [2 I, K], rows g0..g15, u0..u15, g16.. (weights.interleave_gate_up; the CPU tests compare the two)."""
    I, K = gate.shape
    return torch.stack((gate.reshape(I // 16, 16, K), up.reshape(I // 16, 16, K)), 1).reshape(2 * I, K).contiguous()


@functools.lru_cache(maxsize=None)
def swiglu_case(kind, N, K):
    """dict: x [K] bf16, W [N, K] (bf16, or e4m3 codes + scale [N] f32) in the 16-interleaved layout, gate / up [N / 2]
    float64 (the exact pre-activations), ref [N / 2] float64 = silu(gate) * up."""
    fp8 = kind == "fp8"
    I = N // 2
    rng = _rng(3, N, K, int(fp8))
    unit = 0.25 if fp8 else 1.0                                  # the weight grid
    xmax = 4 if fp8 else 8
    x = torch.from_numpy(rng.integers(-xmax, xmax + 1, K).astype(np.float64))
    ucols = np.sort(rng.permutation(K)[:8])                      # columns with x = +-1
    x[ucols] = torch.from_numpy(rng.integers(0, 2, 8) * 2.0 - 1)
    xu = x[ucols]
    rows = torch.arange(I)
    if fp8:                                                      # gate scale by row, up scale by 32 outputs
        sg = torch.ldexp(torch.ones(I, dtype=torch.float64), rows % 5 - 2)
        su = torch.ldexp(torch.ones(I, dtype=torch.float64), (rows // 32 + 2) % 5 - 2)
        allowed = set((E4M3[FP8_CODES.long()] * 4).long().tolist())
    else:
        sg = su = torch.ones(I, dtype=torch.float64)
        allowed = set(range(-8, 9))
    ok = torch.zeros(129, dtype=torch.bool)
    ok[[a + 64 for a in allowed]] = True
    # gate: target t in -2 .. 2 (every value used), raw sum q = t / scale on two of the unit columns
    t = torch.from_numpy(((np.arange(I) * 7 + rng.integers(0, 5)) % 5 - 2).astype(np.float64))
    q = t / sg / unit                                            # in grid units, |q| <= 32
    c1, c2 = rng.integers(0, 8, I), rng.integers(1, 8, I)
    c2 = (c1 + c2) % 8                                           # a different column
    a = torch.from_numpy(rng.integers(-8, 9, I).astype(np.float64))
    r = (q - a * xu[c1]) * xu[c2]
    bad = (r.abs() > 64) | ~ok[(r.clamp(-64, 64) + 64).long()]
    a[bad] = 0.0
    r = (q - a * xu[c1]) * xu[c2]
    assert bool(ok[(r + 64).long()].all()) and bool(ok[(a + 64).long()].all())
    gate_w = torch.zeros((I, K), dtype=torch.float64)
    gate_w[rows, torch.from_numpy(ucols[c1])] = a * unit
    gate_w[rows, torch.from_numpy(ucols[c2])] = r * unit
    # up: dense draw, the unit columns then adjusted so that sum / unit = i (mod 32), non-zero
    up_w = E4M3[_draw(FP8_CODES, (I, K), rng).long()] if fp8 else _draw(BF16_VALUES, (I, K), rng).clone()
    up_w[:, ucols] = 0.0
    s = (up_w @ x) / unit
    d = (rows.double() - s) % 32                                 # 0 .. 31
    d = torch.where(d >= 16, d - 32, d)                          # -16 .. 15
    d = torch.where(s + d == 0, d + 32, d)                       # -16 .. 47, sum of eight steps of at most 8
    for j in range(8):                                           # (fp8: |w| <= 2 there, where every multiple of 1/4 is a code)
        take = d.clamp(-8, 8)
        up_w[:, ucols[j]] = take * xu[j] * unit
        d = d - take
    assert bool((d == 0).all()), "up adjustment out of range"
    w = interleave16(gate_w, up_w)
    gate, up = (gate_w @ x) * sg, (up_w @ x) * su
    assert torch.equal(gate, t) and len(torch.unique(gate)) == 5
    raw_up = (up_w @ x) / unit
    assert bool((raw_up != 0).all()) and torch.equal(raw_up % 32, rows.double() % 32)
    win = up[:I // 32 * 32].reshape(-1, 32)
    assert bool((win.sort(1).values.diff(dim=1) != 0).all()), "up values repeat inside a group of 32 outputs"
    assert float(w.abs().max()) <= 8 and float((w.abs() @ x.abs()).max()) / unit < 2 ** 24
    _exact_f32(gate, "gate"), _exact_f32(up, "up")
    out = dict(x=x.to(torch.bfloat16), gate=gate, up=up, ref=gate * torch.sigmoid(gate) * up, gate_w=gate_w, up_w=up_w)
    if fp8:
        wq = w.float().to(torch.float8_e4m3fn)
        assert torch.equal(wq.float().double(), w)
        out.update(Wq=wq.view(torch.uint8), scale=interleave16(sg[:, None], su[:, None]).reshape(N).float())
    else:
        assert torch.equal(w.to(torch.bfloat16).double(), w)
        out.update(W=w.to(torch.bfloat16))
    return out


def swiglu_tolerance(ref):
    """One bf16 ulp at the rounded reference: silu_fast (v_exp_f32, v_rcp_f32) is a few f32 ulps off, which can only move
    the result across one bf16 rounding boundary."""
    return bf16_ulp(ref.to(torch.bfloat16).double())


# ----------------------------------------------------------------------------- position pick
@functools.lru_cache(maxsize=None)
def pick_case(K):
    """W = I[perm] (K x K), x = K distinct normal bf16 values of both signs: y = x[perm] exactly."""
    rng = _rng(4, K)
    perm = torch.from_numpy(rng.permutation(K))
    bits = 0x3800 + torch.arange(K, dtype=torch.int32)
    assert int(bits.max()) < 0x7F00
    bits = torch.where(torch.arange(K) % 3 == 1, bits | 0x8000, bits)
    x = torch.from_numpy(bits.numpy().astype(np.uint16).view(np.int16)).view(torch.bfloat16)[torch.from_numpy(rng.permutation(K))]
    assert len(torch.unique(x.view(torch.int16))) == K and bool(torch.isfinite(x.float()).all())
    w = torch.zeros((K, K), dtype=torch.bfloat16)
    w[torch.arange(K), perm] = 1.0
    return dict(x=x, W=w, perm=perm)


# ----------------------------------------------------------------------------- argmax ties
@functools.lru_cache(maxsize=None)
def argmax_case(N, K):
    """bf16_case-like operands whose exact maximum logit occurs in `ties` (ascending rows, >= 5 of them): the champion row
    sign(x) * 8 scores 8 sum |x|, which no other integer row in [-8, 8] reaches unless it equals the champion wherever
    x != 0.  `labels[j]` says what ties[j] shares with ties[j - 1] (the levels of the first-index rule)."""
    rng = _rng(5, N, K)
    x = _draw(BF16_VALUES, (1, K), rng)[0]
    w = _draw(BF16_VALUES, (N, K), rng).clone()
    wk = walk("bf16", N, K)
    begin, per = wk["begin"], np.diff(wk["begin"])

    def live(v):                                                # the first wave from v on that owns a pair
        return next(u for u in range(v, per.size) if per[u] > 0)

    first = 3                                                   # the first workgroup with ties (not workgroup 0)
    ties, labels = [], []                                       # labels[j]: what ties[j] shares with ties[j - 1]
    if wk["max_units"] >= 2:                                    # a wave that walks two pairs, from workgroup 3 on
        wv = int(np.nonzero((per >= 2) & (np.arange(per.size) >= 4 * first))[0][0])
        first, p = wv // 4, int(begin[wv])
        ties += [2 * p + 1, 2 * p + 2, 2 * p + 3]
        labels += ["first", "two pairs of one wave", "two rows of one pair"]
    else:
        wv = live(4 * first)
        p = int(begin[wv])
        ties += [2 * p, 2 * p + 1]
        labels += ["first", "two rows of one pair"]
    other = live(wv + 1)
    assert other // 4 == wv // 4
    ties += [2 * int(begin[other])]
    labels += ["two waves of one workgroup"]
    if wk["blocks"] > first + 256:                              # entries `first` and `first + 256` of ONE merging thread
        ties += [2 * int(begin[live(4 * (first + 256) + 2)])]
        labels += ["two workgroups"]
    ties += [2 * int(begin[live(4 * (wk["blocks"] * 3 // 4) + 1)]) + 1]
    labels += ["two workgroups"]
    assert N % 2 == 1
    ties += [N - 1]                                             # its pair's second row is a clamped duplicate
    labels += ["last row of an odd N"]
    assert ties == sorted(set(ties)) and len(ties) >= 5
    champion = torch.sign(x) * 8
    for r in ties:
        w[r] = champion
    assert float(_matvec(w.abs(), x.abs()[None]).max()) < 2 ** 24
    logits = _exact_f32(_matvec(w, x[None])[0], "logits")
    top = float(logits.max())
    assert top == 8 * float(x.abs().sum()) and torch.nonzero(logits == top).flatten().tolist() == ties
    return dict(x=x.to(torch.bfloat16), W=w.to(torch.bfloat16), logits=logits, ties=ties, labels=labels, walk=wk)


def allow_mask(N, cleared):
    """int64 [ceil(N / 64)], bit i of word i // 64 set for every row but `cleared`."""
    bits = np.ones(((N + 63) // 64) * 64, dtype=np.uint8)
    bits[N:] = 0
    bits[list(cleared)] = 0
    return torch.from_numpy(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.int64).reshape(-1).copy())
