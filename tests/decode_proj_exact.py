"""Exact operands, float64 references and the restated launch geometry for the batched decode projection in both forms
(vis_decode_proj_bf16 / _fp8: csrc/decode_stream.hip; vis_decode_proj_colpar_bf16 / _fp8: csrc/decode_colpar.hip; the shared
epilogue ds_epilogue and the deferred norm's ds_row_factors: csrc/decode_proj_common.hip.h).  The pattern of
tests/gemv_exact.py: inputs for which an f32 sum is exact in ANY order, so a segment summed twice, a stale segment block, a
K-step of another ring slot or a clamped row that leaks is a wrong integer, whatever the tolerance of the older tests hides.

Restated geometry (checked against the library's own workspace size on the GPU, against the quoted edges on the CPU):
* streamk_geometry: ds_geometry (decode_stream.hip:380-403: the `per < 4` floor, the halving of `wg` while a tile would be
  cut into more than DS_MAX_SEGS segments, `lcm` clipped to total + 1, nblocks = tiles + nwg), seg_geom (:216-219),
  seg_block / ds_seg_id (:220-224, decode_proj_common.hip.h:41), DsGeom::{DEPTH, NSEG, GRP} (:40-43), ds_rows (:405), the
  workspace formula (:417).
* colpar_geometry: cp_geometry (decode_colpar.hip:212-218), the u0 / cnt split (:62-64), narrow (:66), per / stage_bytes /
  depth (:72-77).

Operands
* bf16: x [64, K] and W [N, K] integers in [-8, 8] (every value used, in row 0 of x too; rows of x pairwise different);
  asserted (|W| @ |x|^T).max() < 2^24.  A test with B rows takes x[:B].
* fp8: activations = e4m3 codes of the integers -4 .. 4 times one E8M0 scale 2^e per (row, 32-column block), e = 0 .. smax with
  (row + block + block // 4) % (smax + 1): neighbouring blocks and rows differ, the four blocks of a K-step too (smax = 3);
  weights from gemv_exact.FP8_CODES (multiples of 1/4 up to 8) with sw[n] = 2^-2 .. 2^2.  In units of 1/4 a partial sum is at
  most 128 * 2^smax * K: smax = 3 up to K = 16383, 2 up to 32767, 1 up to 65535 (K = 37888: 1) - and the builder asserts the
  bound on the actual operands.
* a planted column n* = N // 2: W[n*] = one-hot 1.0 at k* = K // 3 and x[b, k*] a power of two, so acc[b, n*] is a power of
  two and out[b, n*] / acc[b, n*] IS the f32 factor rs[b] the kernel used.
* PLAIN: bias in quarters; acc (* sw) + bias asserted exact in f32.  RESID_NORMW: R in quarters, nw a bf16 draw of both
  signs, all 7 mantissa bits, exponents -1 .. 0; acc + R asserted exact in f32; y = RNE_bf16(acc + R), yw = RNE_bf16(y * nw)
  (a product of two bf16 values is exact in f32: one rounding) - both bit for bit.
* SWIGLU: gemv_exact.swiglu_case generalised to 64 rows on one 16-interleaved weight: row 0 is that construction (gate sums
  -2 .. 2 on two of eight columns where x = +-1, up sums non-zero and congruent to the output index modulo 32: any 32
  consecutive outputs differ), rows 1 .. 63 are independent exact draws.  Tolerance gemv_exact.swiglu_tolerance (one bf16
  ulp, for silu_fast); outputs with gate 0 are exactly 0.

Tolerances (the only three)
* one bf16 ulp for silu_fast (above).
* ssq_out[u][b] = sum of the 32 squares of the written y of unit u (y is bit-exact, so the reference's y): each square of a
  bf16 value is exact in f32 (16 bits), so the only errors are the 31 additions of non-negative terms, each with relative
  error <= u = 2^-24 on a partial sum <= the total: |got - sum| <= gamma(31) * sum, gamma(n) = n u / (1 - n u) (Higham,
  Accuracy and Stability of Numerical Algorithms, section 4.2), whatever the order (8 lane-local terms, then 4 lanes).
* rs[b] (ds_row_factors): tot is an exact integer (integer partials, < 2^24), inv = fl(1 / norm_dim) (relative error <= u),
  the argument a = fl(fl(tot * inv) + eps) or fma(tot, inv, eps): at most three roundings, relative error <= 3 u + O(u^2) of
  tot / norm_dim + eps (eps the f32 the library receives), which rsqrt halves: 1.5 u.  On top comes v_rsq_f32.  The ISA
  description available to this project gives no accuracy figure for it, so the figure is measured: RS_MEASURED_REL below
  is the worst |r_b / rsqrt64 - 1| over all rows of test_deferred_norm on an MI355X (8.847e-08 at tiles_in = 3, 7.2e-08 /
  8.0e-08 / 8.5e-08 / 7.0e-08 at 32 / 33 / 112 / 128: about 1.5 u, i.e. the argument's roundings with v_rsq_f32 itself
  inside one ulp), and the test allows twice that (RS_REL_BOUND).  test_deferred_norm prints the figure of its run.
  Part (a) of the check is exact and independent of it: every element of row b is fl32(acc * r_b) for ONE f32 r_b.

v_mfma_scale_f32_16x16x128_f8f6f4 sums these operands exactly when the four block scales inside one instruction differ
(dense rows, scales 2^0 .. 2^3, products in quarters): every dense fp8 sum of the GPU tests equals float64 bit for bit in
both forms on an MI355X, so the dense-sum tests keep the varied scales.

CPU only: float64 torch / numpy, never the library under test.
"""
import functools
import math

import numpy as np
import torch

import gemv_exact as G

BN, CNT_BYTES, MAX_WG, MAX_SEGS = 128, 16384, 256, 16
CP_MAX_UNITS, CP_MAX_DEPTH, CP_RING_BYTES = 5, 10, 150 * 1024
PLAIN, SWIGLU, RESID = 0, 1, 2
U32 = 2.0 ** -24
RS_MEASURED_REL = 8.85e-8         # worst relative error of rs[b] against float64 measured on an MI355X (see the docstring)
RS_REL_BOUND = 2 * RS_MEASURED_REL
TILES_IN = [3, 32, 33, 112, 128]
BATCHES = [1, 16, 17, 32, 33, 64]

# (N, K in bf16 terms - fp8 doubles it, batch sizes, modes, what it reaches)
STREAMK_SHAPES = [
    (128, 64, BATCHES, "all", "one-tile-one-step"),
    (128, 256, BATCHES, "all", "one-range-ring-never-refilled"),
    (128, 1280, BATCHES, "all", "ns5-partial-second-gather-round"),
    (128, 4096, BATCHES, "all", "ns16-max-gather-rounds"),
    (128, 6400, BATCHES, "all", "wg-halved-spb7-ns15-lcm-clipped"),
    (384, 640, BATCHES, "all", "seams-inside-tiles-ns3-lcm-inside"),
    (256, 704, BATCHES, "all", "ns3-and-ns4-lcm-clipped"),
    (1000, 192, BATCHES, "plain", "ragged-N"),
    (6144, 128, BATCHES, "all", "uncut-two-tiles-per-range"),
    (262272, 64, [4, 17, 33], "all", "overflow-path-uncut"),
    (262272, 192, [17, 64], "plain_f32", "overflow-path-cut-tiles"),
    (3584, 18944, [4, 64], "resid", "long-K-ns9-10"),
]
COLPAR_N = [(32, "one-unit"), (512, "16-wg-of-one-unit"), (9600, "cnt2-and-cnt1-narrow"), (19200, "cnt3-and-cnt2"),
            (35200, "cnt5-and-cnt4-has1"), (40960, "all-cnt5-limit")]
COLPAR_K_512 = [64, 576, 640, 704, 3584]


def rows_of(B):
    return 16 if B <= 16 else 32 if B <= 32 else 64


def stream_consts(B):
    """DsGeom<FP8, MB>: DEPTH, NSEG, GRP for the kernel B rows run on."""
    MB = rows_of(B) // 16
    return dict(MB=MB, DEPTH=6 if MB == 4 else 7, NSEG=6 if MB == 4 else 8, GRP=16 // (MB * 2) * 2)


# ----------------------------------------------------------------------------- geometry, restated
@functools.lru_cache(maxsize=None)
def streamk_geometry(N, K, fp8=False):
    nk = K // (128 if fp8 else 64)
    tiles = (N + BN - 1) // BN
    total = tiles * nk
    wg = MAX_WG
    while True:
        per = (total + wg - 1) // wg
        if per < 4:
            per = total if total < 4 else 4
        t = np.arange(tiles, dtype=np.int64)
        first = t * nk // per
        ns = ((t + 1) * nk - 1) // per - first + 1
        if int(ns.max()) <= MAX_SEGS or wg == 1:
            break
        wg //= 2
    nwg = (total + per - 1) // per
    lcm = nk // math.gcd(nk, per) * per
    if lcm > total:
        lcm = total + 1
    s0 = np.arange(nwg, dtype=np.int64) * per
    s1 = np.minimum(s0 + per, total)
    wg_tiles = (s1 - 1) // nk - s0 // nk + 1                      # tiles each workgroup's range touches
    ids = []                                                       # ds_seg_id of every segment of every cut tile
    for tt in np.nonzero(ns > 1)[0]:
        w = first[tt] + np.arange(ns[tt])
        start = np.maximum(tt * nk, w * per)
        ids.append(start // nk + start // per - start // lcm)
    nblocks = tiles + nwg
    return dict(nk=nk, tiles=tiles, total=total, wg=wg, spb=int(per), nwg=int(nwg), lcm=int(lcm), nblocks=int(nblocks), ns=ns,
                first=first, wg_tiles=wg_tiles, seg_ids=np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64),
                ws_bytes={r: CNT_BYTES + nblocks * r * BN * 4 for r in (16, 32, 64)})


@functools.lru_cache(maxsize=None)
def colpar_geometry(N, K, B, fp8=False):
    """None when the form does not cover N; else nk, nwg, cnt [nwg], and per distinct cnt: narrow, stage_bytes, per, depth."""
    if N <= 0 or N % 32:
        return None
    units = N // 32
    nwg = min(units, 256)
    if (units + nwg - 1) // nwg > CP_MAX_UNITS:
        return None
    MB = rows_of(B) // 16
    XI = 2 if MB == 4 else 1
    base, extra = units // nwg, units % nwg
    w = np.arange(nwg)
    cnt = base + (w < extra)
    u0 = w * base + np.minimum(w, extra)
    assert int(cnt.sum()) == units and np.array_equal(u0, np.concatenate(([0], np.cumsum(cnt)[:-1])))
    kinds = {}
    for c in sorted(set(cnt.tolist())):
        stage = XI * 32 * 128 + c * 4096 + (1024 if fp8 else 0)
        per = XI + c + (1 if fp8 else 0)
        depth = min(CP_RING_BYTES // stage, CP_MAX_DEPTH)
        if (depth - 2) * per > 63:
            depth = 63 // per + 2
        assert depth * stage <= CP_RING_BYTES + 4096
        kinds[c] = dict(narrow=MB == 4 and c == 1, stage_bytes=stage, per=per, depth=depth, has1=c == CP_MAX_UNITS)
    return dict(nk=K // (128 if fp8 else 64), units=units, nwg=nwg, cnt=cnt, kinds=kinds, MB=MB)


def colpar_nks(N, B, fp8):
    """K-steps a column-parallel test of N runs at B rows: 1, and one below / at / one above the ring depth of every unit
    count of the launch (N = 512: the issue's list 1, 9, 10, 11, 56 - the one-unit depth is 10)."""
    if N == 512:
        return [k // 64 for k in COLPAR_K_512]
    g = colpar_geometry(N, 64, B, fp8)
    nks = {1}
    for kind in g["kinds"].values():
        nks |= {kind["depth"] - 1, kind["depth"], kind["depth"] + 1}
    return sorted(nks)


# ----------------------------------------------------------------------------- draws
def _draw_ints(values, shape, rng):
    """int16 draw from the int list `values`, every value forced into the first elements (as many as there are)."""
    values = np.asarray(values, dtype=np.int16)
    out = values[rng.integers(0, len(values), shape, dtype=np.int8 if len(values) < 128 else np.int16)]
    flat = out.reshape(-1)
    m = min(flat.size, len(values))
    head = min(flat.size, 4096)
    flat[rng.permutation(head)[:m]] = rng.permutation(values)[:m]
    return out


def _uses_all(arr, values):
    """Every value of `values` occurs (large arrays: among the first 4096 elements, where _draw_ints forces them in)."""
    flat = arr.reshape(-1)
    return np.array_equal(np.unique(flat if flat.size <= (1 << 20) else flat[:4096]), np.unique(values))


_Q = np.arange(-32, 33)
_Q_BYTES = (torch.from_numpy(_Q / 4.0).float().to(torch.float8_e4m3fn)).view(torch.uint8).numpy()      # quarters -> e4m3 byte


def _quarter_bytes(wi):
    """int16 quarters (on the e4m3 grid) -> e4m3 bytes, by table."""
    return torch.from_numpy(_Q_BYTES[wi + 32])


def _e4m3_bytes(vals):
    """float64 values representable in e4m3 -> their bytes."""
    q = vals.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.float().double(), vals.double()), "not an e4m3 value"
    return q.view(torch.uint8)


FP8_GRID = sorted(set((G.E4M3[G.FP8_CODES.long()] * 4).long().tolist()))       # weight values in quarters: 49 of them
BF16_GRID = list(range(-8, 9))


def fp8_smax(K):
    smax = min(3, int(math.floor(math.log2((2 ** 24 - 1) / (128.0 * K)))))
    assert smax >= 1, "K too long for varied block scales"
    return smax


def _x_rows(K, fp8, rng, small_cols=None, smax=None):
    """64 pairwise different activation rows: (values float64 [64, K], codes uint8 or None, scale bytes uint8 or None).
    small_cols: columns where every row holds -1, 0 or 1; smax: the largest block-scale exponent (default fp8_smax(K))."""
    vals = list(range(-4, 5)) if fp8 else BF16_GRID
    pw = np.array([1, 2, 4] if fp8 else [1, 2, 4, 8], dtype=np.int16)
    while True:
        xi = np.concatenate((_draw_ints(vals, (1, K), rng), _draw_ints(vals, (63, K), rng)))
        xi[:, K // 3] = pw[np.arange(64) % len(pw)] * np.where(np.arange(64) % 2, -1, 1)    # the planted column's operand
        if small_cols is not None:
            xi[:, small_cols] = rng.integers(-1, 2, (64, len(small_cols)))
        if len({r.tobytes() for r in xi}) == 64 and _uses_all(xi[0], vals):                 # (planting may take a value out)
            break
    x = torch.from_numpy(xi.astype(np.float64))
    if not fp8:
        return x, None, None
    smax = fp8_smax(K) if smax is None else smax
    b, blk = np.arange(64)[:, None], np.arange(K // 32)[None, :]
    e = (b + blk + (blk // 4 if smax >= 2 else 0)) % (smax + 1)
    assert bool((np.diff(e, axis=1) != 0).all()) and bool((np.diff(e, axis=0) != 0).all())
    codes = _e4m3_bytes(x)
    scale = torch.from_numpy(np.repeat(2.0 ** e, 32, axis=1))
    return x * scale, codes, torch.from_numpy((127 + e).astype(np.uint8))


def _nw_draw(N, rng):
    bits = (rng.integers(0, 2, N) << 15) | (rng.integers(126, 128, N) << 7) | ((np.arange(N) * 37 + rng.integers(0, 128)) % 128)
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def _abs_bound(w_abs, x_abs, unit):
    worst = float(G._matvec(w_abs, x_abs).max()) / unit
    assert worst < 2 ** 24, f"a partial sum could reach {worst} units"
    return worst


# ----------------------------------------------------------------------------- plain / residual cases
@functools.lru_cache(maxsize=8)
def case(kind, N, K):
    """Operands for 64 rows (a test with B rows takes [:B]).  kind "bf16": x bf16, W bf16; "fp8": xq / xs / Wq uint8, sw f32.
    acc [64, N] float64 = x W^T (* sw), exact in f32; bias [N], R [64, N], nw [N] bf16; nstar = the planted column."""
    fp8 = kind == "fp8"
    rng = G._rng(21, N, K, int(fp8))
    grid = FP8_GRID if fp8 else BF16_GRID
    nstar = N // 2
    while True:
        wi = _draw_ints(grid, (N, K), rng)
        wi[nstar] = 0
        wi[nstar, K // 3] = 4 if fp8 else 1
        if _uses_all(wi, grid):
            break
    xv, xq, xs = _x_rows(K, fp8, rng)
    unit = 0.25 if fp8 else 1.0
    if fp8:
        wq = _quarter_bytes(wi)
        w_val = torch.from_numpy(wi.astype(np.float16) / np.float16(4))  # f16 holds multiples of 1/4 up to 8 exactly
        sw = G.fp8_scales(N)
    else:
        w_val = torch.from_numpy(wi.astype(np.float32)).to(torch.bfloat16)
        sw = torch.ones(N, dtype=torch.float64)
    del wi
    _abs_bound(w_val.abs(), xv.abs(), unit)
    raw = G._exact_f32(G._matvec(w_val, xv), "sum")
    acc = G._exact_f32(raw * sw[None, :], "sum * sw")
    a_star = acc[:, nstar].abs()
    assert bool((a_star > 0).all()) and torch.equal(torch.frexp(a_star)[0], torch.full((64,), 0.5, dtype=torch.float64))
    bias, R, nw = G._quarters((N,), rng), G._quarters((64, N), rng), _nw_draw(N, rng)
    G._exact_f32(acc + bias[None, :], "+ bias"), G._exact_f32(acc + R, "+ residual")
    y = (acc + R).float().to(torch.bfloat16)
    yw = G._exact_f32(y.double() * nw.double()[None, :], "y * nw").float().to(torch.bfloat16)
    out = dict(kind=kind, N=N, K=K, acc=acc, bias=bias.to(torch.bfloat16), R=R.to(torch.bfloat16), nw=nw, y=y, yw=yw,
               nstar=nstar, sw=sw.float())
    if fp8:
        out.update(xq=xq, xs=xs, Wq=wq)
    else:
        out.update(x=xv.to(torch.bfloat16), W=w_val)
    return out


def ssq_ref(y, B):
    """[ceil(N / 32), B] float64: per 32-column unit, the sum of the squares of y [>= B, N] (bf16)."""
    N = y.shape[1]
    pad = torch.zeros((B, (N + 31) // 32 * 32), dtype=torch.float64)
    pad[:, :N] = y[:B].double() ** 2
    return pad.view(B, -1, 32).sum(-1).t().contiguous()


def ssq_tolerance(ref):
    g31 = 31 * U32 / (1 - 31 * U32)
    return g31 * ref


# ----------------------------------------------------------------------------- deferred norm
@functools.lru_cache(maxsize=None)
def norm_case(tiles_in, seed=0):
    """big [tiles_in + 3, 64] f32, NaN outside [:tiles_in, :]; the caller NaNs columns >= B.  tot [64] exact integers,
    r64 [64] = rsqrt(tot / norm_dim + eps32) in float64."""
    rng = G._rng(31, tiles_in, seed)
    part = rng.integers(1, 2000, (tiles_in, 64)).astype(np.float64)
    part[:, 1] = rng.integers(1, 4, tiles_in)                      # rows of very different norms
    part[:, 2] = rng.integers(100000, 130000, tiles_in)
    tot = part.sum(0)
    assert float(tot.max()) < 2 ** 24
    big = torch.full((tiles_in + 3, 64), float("nan"), dtype=torch.float32)
    big[:tiles_in] = torch.from_numpy(part).float()
    norm_dim, eps = 32 * tiles_in, 1e-6
    eps32 = float(np.float32(eps))
    r64 = 1.0 / np.sqrt(tot / norm_dim + eps32)
    return dict(big=big, tiles_in=tiles_in, norm_dim=norm_dim, eps=eps, tot=torch.from_numpy(tot), r64=torch.from_numpy(r64))


def scaled_candidates(acc, r32, bias):
    """The f32 values `acc * r + bias` may legitimately store: the two-rounding form fl(fl(acc r) + bias) and the contracted
    fma(acc, r, bias) (the source leaves the choice to the compiler).  The fma is bracketed: acc r is exact in float64
    (24 + 24 bits), the float64 sum s is within one float64 ulp of the true sum, and rounding is monotonic, so the true
    rounding lies between fl32(nextafter(s, -inf)) and fl32(nextafter(s, +inf)) - which are one value except next to a tie.
    acc [B, N] float64 exact in f32, r32 [B] f32, bias [N] float64 or None -> list of f32 [B, N] tensors."""
    r = r32.double()[:, None]
    prod = acc * r
    if bias is None:
        return [prod.float()]
    s = prod + bias[None, :]
    two = (prod.float() + bias.float()[None, :])
    inf = torch.full_like(s, float("inf"))
    return [two, s.float(), torch.nextafter(s, -inf).float(), torch.nextafter(s, inf).float()]


# ----------------------------------------------------------------------------- SwiGLU
@functools.lru_cache(maxsize=8)
def swiglu_case(kind, N, K):
    """64 rows on one 16-interleaved weight [N, K]; gate / up / ref [64, N / 2] float64.  Row 0: gemv_exact.swiglu_case's
    construction (see the module docstring); fp8: row 0 has unit block scales, rows 1.. the varied ones."""
    fp8 = kind == "fp8"
    I = N // 2
    rng = G._rng(23, N, K, int(fp8))
    unit = 0.25 if fp8 else 1.0
    grid = FP8_GRID if fp8 else BF16_GRID
    # rows 1..: -1, 0, 1 on the eight gate columns and block scales of at most 2, so that |gate| <= (8 + 10) * 2 = 36 and
    # silu(gate) * up stays a normal f32 (e^-88 is where silu_fast's result would be flushed: not what one bf16 ulp is for)
    ucols = np.sort(rng.permutation(K)[:8])
    xv, xq, xs = _x_rows(K, fp8, rng, small_cols=ucols, smax=1 if fp8 else None)
    xmax = 4 if fp8 else 8
    x0 = rng.integers(-xmax, xmax + 1, K).astype(np.float64)
    x0[ucols] = rng.integers(0, 2, 8) * 2.0 - 1
    xu = x0[ucols]
    xv[0] = torch.from_numpy(x0)
    if fp8:
        xq[0], xs[0] = _e4m3_bytes(xv[0]), 127
    rows = np.arange(I)
    if fp8:
        sg, su = 2.0 ** (rows % 5 - 2), 2.0 ** ((rows // 32 + 2) % 5 - 2)
    else:
        sg = su = np.ones(I)
    ok = np.zeros(129, dtype=bool)
    ok[np.asarray(grid) + 64] = True
    t = ((rows * 7 + rng.integers(0, 5)) % 5 - 2).astype(np.float64)
    q = t / sg / unit
    c1 = rng.integers(0, 8, I)
    c2 = (c1 + rng.integers(1, 8, I)) % 8
    a = rng.integers(-8, 9, I).astype(np.float64)
    r = (q - a * xu[c1]) * xu[c2]
    bad = (np.abs(r) > 64) | ~ok[(np.clip(r, -64, 64) + 64).astype(np.int64)]
    a[bad] = 0.0
    r = (q - a * xu[c1]) * xu[c2]
    assert ok[(r + 64).astype(np.int64)].all() and ok[(a + 64).astype(np.int64)].all()
    gate_w = np.zeros((I, K), dtype=np.float32)                       # in grid units
    gate_w[rows, ucols[c1]] = a
    gate_w[rows, ucols[c2]] = r
    up_w = _draw_ints(grid, (I, K), rng).astype(np.float32)
    up_w[:, ucols] = 0.0
    s = up_w.astype(np.float64) @ x0
    d = (rows - s) % 32
    d = np.where(d >= 16, d - 32, d)
    d = np.where(s + d == 0, d + 32, d)
    for j in range(8):
        take = np.clip(d, -8, 8)
        up_w[:, ucols[j]] = take * xu[j]
        d = d - take
    assert (d == 0).all(), "up adjustment out of range"
    gw, uw = torch.from_numpy(gate_w) * unit, torch.from_numpy(up_w) * unit       # values, exact in f32
    w = G.interleave16(gw, uw)
    _abs_bound(w.abs(), xv.abs(), unit)
    sgt, sut = torch.from_numpy(sg), torch.from_numpy(su)
    gate = G._exact_f32(G._matvec(gw, xv) * sgt[None, :], "gate")
    up = G._exact_f32(G._matvec(uw, xv) * sut[None, :], "up")
    assert torch.equal(gate[0], torch.from_numpy(t)) and len(torch.unique(gate[0])) == min(5, I)
    raw_up = up[0] / sut / unit
    assert bool((raw_up != 0).all()) and torch.equal(raw_up % 32, torch.from_numpy(rows).double() % 32)
    win = up[0, :I // 32 * 32].reshape(-1, 32)
    assert bool((win.sort(1).values.diff(dim=1) != 0).all()), "up values repeat inside a group of 32 outputs"
    ref = gate * torch.sigmoid(gate) * up
    assert float(gate.abs().max()) <= 36 and float(ref[ref != 0].abs().min()) > 2.0 ** -60, "an output near the f32 underflow"
    out = dict(kind=kind, N=N, K=K, gate=gate, up=up, ref=ref)
    if fp8:
        out.update(xq=xq, xs=xs, Wq=_e4m3_bytes(w), sw=G.interleave16(sgt[:, None], sut[:, None]).reshape(N).float())
    else:
        assert torch.equal(w.to(torch.bfloat16).float(), w)
        out.update(x=xv.to(torch.bfloat16), W=w.to(torch.bfloat16), sw=torch.ones(N))
    return out


# ----------------------------------------------------------------------------- buffers with something around them
def padded_scales(xs, pad=4, byte=140):
    """[B, K / 32] -> the [:, :K / 32] view of a wider buffer whose padding holds a scale (2^13) that would change the sum."""
    wide = torch.full((xs.shape[0], xs.shape[1] + pad), byte, dtype=torch.uint8)
    wide[:, :xs.shape[1]] = xs
    return wide


def residual_buffer(R, B):
    """[B + 1, N + 24] bf16, NaN around R[:B]."""
    N = R.shape[1]
    rb = torch.full((B + 1, N + 24), G.NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    rb[:B, :N] = R[:B]
    return rb
