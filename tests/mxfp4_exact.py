"""Exact operands, float64 references and the restated launch geometry for the three MXFP4 decode kernels: vis_gemv_mxfp4w /
vis_gemv_mxfp4w_rows (csrc/decode_fp4.hip) and vis_gemm_decode_mxfp4 (csrc/decode_fp4_batched.hip).  The pattern of
tests/gemv_exact.py and tests/decode_proj_exact.py: inputs for which an f32 sum is exact in ANY order, so the kernels must
give the float64 result bit for bit, and a block summed twice, a stale accumulator set, a slot of another tile or a scale byte
of the neighbouring block is a wrong number whatever the tolerance of the older tests hides.

Decode.  `decode` takes E2M1 codes (sign << 3 | exp << 1 | man) and E8M0 bytes (2^(b - 127)) to float64 from the bit fields;
it never calls hip.dequantize_mxfp4 (tests/test_mxfp4_exact.py compares the two on all 16 x 248 pairs).

Operand families (weights [N, K] as codes + one scale byte per 32 elements, x [B, K] bf16):
* "narrow": random code bytes (all 16 codes), scale bytes 125 .. 129, integer x in [-8, 8].  Products are multiples of 2^-3.
* "wide": the scale byte of block j of row n is base(j) + d(n, j); base(j) walks 5 .. 248 evenly over the blocks of a row,
  d(n, j) = (n + 2 j + j // 5) % 5 - 2 differs between neighbouring rows AND neighbouring blocks, so a scale byte read from
  either neighbour is off by a power of two.  x in block j is m 2^(127 - base(j)), m an integer in [-8, 8].  Every weight
  (2^-125 .. 6 x 2^123) and every x is a normal bf16; every product is code x m x 2^d: a multiple of 2^-3, at most 192.
  One vector x serves all rows, so base cannot depend on the row: a matrix of nblk blocks holds the bytes
  base(j) + {-2 .. 2} - all 248 bytes 3 .. 250 from 50 blocks (K >= 1600) on, which the builder asserts; below that it
  asserts that exactly the bytes base(j) + {-2 .. 2} occur, 3 and 250 among them when K >= 64 (K = 32: one block at a
  base drawn per shape).  `every_code_case` covers all of 3 .. 250 on one matrix for both kernels.
* both: the builder asserts on the actual operands that max_n sum_k |w[n, k]| max_b |x[b, k]| < 2^21 (a bound on every
  partial sum of every row in any order; in units of 2^-3 that is < 2^24: exact in f32), that all 16 codes occur, and - as
  gemv_exact does - that every stage of the epilogue (sum + bias) + R, bias and R multiples of 1/4 in [-3, 3], is exact.
* SwiGLU (`swiglu_case`, narrow scale bytes): the gate / up construction of gemv_exact.swiglu_case on the E2M1 grid.  Gate
  rows have one or two non-zero codes on columns where x = +-1 and sum to -2 .. 2; up rows are dense, with the eight unit
  columns (in blocks of scale 1/4) adjusted so that the up sum of output i, in units of 2^-3, is non-zero and congruent to
  i modulo 32.  Tolerance: gemv_exact.swiglu_tolerance (one bf16 ulp for silu_fast), nothing else.
* fused RMSNorm (`norm_case`): gemv_exact.norm_operands - the staged row is sign * norm_w exactly - on narrow weights.
* `every_code_case`: K = 32 x 248, block j of every row has scale byte 3 + j; row 16 j + c holds code c once, in block j at
  element (c + j) % 32, and code 0 elsewhere; x[b] = 2^(b % 3) 2^(127 - byte) throughout block j: y[b, 16 j + c] is
  2^(b % 3) x the E2M1 value of c, for every (code, byte) pair.  Bytes 0 .. 2 and 251 .. 255 are not quantiser output
  (quantize_mxfp4_rows clamps to 3 .. 250) and are left out: with them a weight or its product with x leaves the normal
  bf16 range.

Restated geometry: `walk_gemv` = gemv_mxfp4w_launch (the task shape), gemv_mxfp4w_launch_shape (blocks, the 2048 cap) and the
kernel's g_begin / g_end / nseg / n_tasks; `walk_gemm` = f4g_geometry and the kernel's range walk over its accumulator sets.
tests/test_mxfp4_exact.py asserts from them that every shape below reaches the edge it is listed for.

CPU only: float64 torch / numpy, never the library under test.
"""
import functools

import numpy as np
import torch

import gemv_exact as G

SENTINEL = G.SENTINEL
FAMILIES = ("narrow", "wide")
BYTES = list(range(3, 251))                 # the quantiser's scale bytes: 248 of them
WIDE_ALL_BYTES_FROM = 50                    # blocks per row from which base(j) + {-2 .. 2} covers all of 3 .. 250

# ---- vis_gemv_mxfp4w: (N, K) -> the edge (checked in tests/test_mxfp4_exact.py)
GEMV_SHAPES = [(40968, 32), (152064, 64), (300032, 32), (8200, 10272), (8200, 20512), (1002, 704)]
GEMV_SWIGLU_SHAPES = [(64, 256), (16448, 64), (75776, 64)]
GEMV_NORM_SHAPES = [(6, 4128), (1002, 704)]
GEMV_ROWS_NORM_SHAPES = [(6, 4128), (40968, 32)]
WIDE_MAX_K = 10272                          # both families up to this K, narrow alone above
PADDED_MAX_N = 1002
# ---- vis_gemm_decode_mxfp4: (N, K, batch sizes)
GEMM_SHAPES = [(131200, 64, (33, 64)), (131200, 512, (64,)), (131200, 768, (33,)), (262272, 64, (5, 17)),
               (262272, 512, (17,)), (65664, 384, (5, 17, 33))]
GEMM_WIDE_SHAPES = [(1000, 704, (5, 33)), (131200, 512, (64,))]
GEMM_DIRECT = (131200, 64, 40)
MAX_SLOTS = 16


# ----------------------------------------------------------------------------- number formats
def _e2m1(code):
    s, e, m = code >> 3, (code >> 1) & 3, code & 1
    mag = 0.5 * m if e == 0 else (1 + 0.5 * m) * 2.0 ** (e - 1)
    return -mag if s else mag


E2M1 = torch.tensor([_e2m1(c) for c in range(16)], dtype=torch.float64)
_CODE_OF = {float(E2M1[c]): c for c in range(15, -1, -1) if c != 8}          # value -> code (+0 for zero)


def e8m0(b):
    """2^(byte - 127), float64."""
    return torch.ldexp(torch.ones(b.shape, dtype=torch.float64), b.to(torch.int32) - 127)


def unpack(wq):
    """[n, K / 2] bytes -> [n, K] codes: byte j = element 2 j (low nibble), 2 j + 1 (high nibble)."""
    return torch.stack((wq & 15, wq >> 4), dim=-1).reshape(wq.shape[0], -1)


def pack(codes):
    c = codes.to(torch.uint8).reshape(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous()


def decode(wq, ws):
    """(codes [n, K / 2], scale bytes [n, K / 32]) -> float64 [n, K]."""
    v = E2M1[unpack(wq).long()]
    return (v.reshape(wq.shape[0], -1, 32) * e8m0(ws)[..., None]).reshape(wq.shape[0], -1)


def matmul_ref(wq, ws, x):
    """x [B, K] float64 -> (x @ decode(wq, ws)^T [B, N] float64, max_n sum_k |w| max_b |x|), in row chunks of the weights so
    that the float64 matrix never exceeds 128 MB."""
    N, K = wq.shape[0], wq.shape[1] * 2
    step = max(64, (1 << 24) // K)
    xt = x.t().contiguous()
    xmax = x.abs().amax(0)
    out, bound = [], 0.0
    for i in range(0, N, step):
        w = decode(wq[i:i + step], ws[i:i + step])
        out.append(w @ xt)
        bound = max(bound, float((w.abs() @ xmax).max()))
    return torch.cat(out).t().contiguous(), bound


# ----------------------------------------------------------------------------- geometry, restated
def gemv_task_shape(N, K, swiglu=False):
    """<ROWS, SEG> of gemv_mxfp4w_launch."""
    n_out = N // 2 if swiglu else N
    return (2, 5) if K > 4096 else (2, 2) if n_out <= 8192 else (8, 2)


def walk_gemv(N, K, swiglu=False):
    """The task walk of one vis_gemv_mxfp4w launch: a group is ROWS weight rows (SwiGLU: ROWS / 2 outputs), a task one group
    x one segment of SEG x 64 MX blocks.  Returns rows, seg, n_grps, raw_blocks (before the formula), blocks, capped, nch
    (blocks per row), nch8 (16-byte chunks of x), nseg, groups / tasks [n_waves] per wave, idle_waves, tail_blocks (live
    blocks of the last segment), clamped_blocks (lane slots of the last segment past the row's end), crossings (ring
    buffers from the last segment of one group to the first of the next)."""
    rows, seg = gemv_task_shape(N, K, swiglu)
    n_out = N // 2 if swiglu else N
    n_grps = n_out // (rows // 2) if swiglu else (n_out + rows - 1) // rows
    raw = (n_grps + 3) // 4
    blocks = raw if raw <= 1024 else 1024 + (raw - 1024) // 8
    capped = blocks > 2048
    blocks = min(blocks, 2048)
    n_waves = blocks * 4
    nch = K // 32
    nseg = ((nch + 63) // 64 + seg - 1) // seg
    begin = np.arange(n_waves + 1, dtype=np.int64) * n_grps // n_waves
    groups = np.diff(begin)
    crossings = {"AB"[(j * nseg - 1) % 2] + "AB"[(j * nseg) % 2] for j in range(1, int(groups.max()))}
    return dict(rows=rows, seg=seg, n_grps=n_grps, raw_blocks=raw, blocks=blocks, capped=capped, nch=nch, nch8=K // 8,
                nseg=nseg, groups=groups, tasks=groups * nseg, idle_waves=int((groups == 0).sum()),
                tail_blocks=nch - (nseg - 1) * seg * 64, clamped_blocks=nseg * seg * 64 - nch, crossings=crossings)


def gemm_mb(B):
    return 1 if B <= 16 else 2 if B <= 32 else 4


def walk_gemm(N, K, B, direct=False):
    """f4g_geometry and the range walk of gemm_decode_mxfp4_kernel<MB>.  Returns MB, NSEG, nk, tiles, per (K-steps per
    workgroup), nslots, nwg, last_step_blocks (valid MX blocks of a tile row's last K-step), and per workgroup:
    tiles_per_range, starts_inside / ends_inside (the range begins / ends inside a tile), and `ranges`: for every workgroup
    the list of (tile, set, first_kt, last_kt, done, on_spot, slot) in the order the kernel runs them - `set` the
    accumulator set, `done` what the kernel passes as tile_done, `on_spot` a flush while the ring still runs, `slot` the
    partial slot blockIdx.x - (tile * nk) / per."""
    MB = gemm_mb(B)
    NSEG = 4 if MB == 4 else 8
    tiles, nk = (N + 127) // 128, (K + 255) // 256
    total = tiles * nk
    wg = 256
    while True:
        if direct:
            per = (tiles + wg - 1) // wg * nk
        else:
            per = (total + wg - 1) // wg
            if per < 4:
                per = total if total < 4 else 4
        slots = 1
        if not direct:
            t = np.arange(tiles, dtype=np.int64)
            slots = int((((t + 1) * nk - 1) // per - (t * nk) // per + 1).max())
        if slots <= MAX_SLOTS or wg == 1:
            break
        wg //= 2
    nwg = (total + per - 1) // per
    ranges = []
    for w in range(nwg):
        s0 = w * per
        nsteps = min(s0 + per, total) - s0
        c_tile, c_kt, st, r = s0 // nk, s0 % nk, 0, []
        for sg in range(NSEG):
            if st >= nsteps:
                break
            while True:
                n_here = min(nsteps - st, nk - c_kt)
                first = c_kt
                st += n_here
                c_kt += n_here
                done = c_kt == nk
                more = not (sg + 1 < NSEG or st >= nsteps)
                r.append((c_tile, sg, first, c_kt - 1, done, more, w - (c_tile * nk) // per))
                if done:
                    c_kt, c_tile = 0, c_tile + 1
                if not more:
                    break
        assert st == nsteps, "the kernel would leave K-steps of its range undone"
        ranges.append(r)
    return dict(MB=MB, NSEG=NSEG, nk=nk, tiles=tiles, per=int(per), nslots=slots, nwg=int(nwg),
                last_step_blocks=K // 32 - (nk - 1) * 8, ranges=ranges,
                tiles_per_range=np.array([len(r) for r in ranges]),
                starts_inside=np.array([r[0][2] != 0 for r in ranges]),
                ends_inside=np.array([not r[-1][4] for r in ranges]))


# ----------------------------------------------------------------------------- operands
_ALL_CODES = torch.tensor([0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE], dtype=torch.uint8)


def _codes(N, K, rng):
    wq = torch.from_numpy(rng.integers(0, 256, (N, K // 2), dtype=np.uint8))
    wq[0, :8] = _ALL_CODES
    assert len(torch.unique(unpack(wq[:64]))) == 16, "not all 16 codes occur"
    return wq


def wide_base(nblk, rng):
    if nblk == 1:
        return np.array([5 + int(rng.integers(0, 244))], dtype=np.int64)
    return 5 + (np.arange(nblk, dtype=np.int64) * 243) // (nblk - 1)


def wide_delta(N, nblk):
    n, j = np.arange(N, dtype=np.int64)[:, None], np.arange(nblk, dtype=np.int64)[None, :]
    d = (n + 2 * j + j // 5) % 5 - 2
    assert (np.diff(d, axis=0) != 0).all() and (nblk == 1 or (np.diff(d, axis=1) != 0).all())
    return d


def _distinct_rows(draw, B):
    while True:
        m = draw()
        if len({r.tobytes() for r in m}) == B:
            return m


def _operands(family, N, K, B, rng):
    """(wq, ws, x float64 [B, K]) of one family, with the family's own assertions."""
    nblk = K // 32
    wq = _codes(N, K, rng)
    m = _distinct_rows(lambda: rng.integers(-8, 9, (B, K)), B).astype(np.float64)
    if family == "narrow":
        ws = rng.integers(125, 130, (N, nblk), dtype=np.uint8)
        assert N * nblk < 64 or set(np.unique(ws).tolist()) == {125, 126, 127, 128, 129}
        x = torch.from_numpy(m)
    else:
        base, d = wide_base(nblk, rng), wide_delta(N, nblk)
        ws = (base[None, :] + d).astype(np.uint8)
        have = set(np.unique(ws).tolist())
        reach = {int(b) + e for b in base for e in range(-2, 3)} if N >= 5 else have
        assert have == reach and have <= set(BYTES), "the scale bytes are not base(j) + {-2 .. 2}"
        if nblk >= 2:
            assert {3, 250} <= have
        if nblk >= WIDE_ALL_BYTES_FROM and N >= 5:
            assert have == set(BYTES), "not all 248 scale bytes occur"
        x = torch.from_numpy(m) * e8m0(torch.from_numpy(2 * 127 - base)).repeat_interleave(32)[None, :]
        nz = x[x != 0].abs()
        assert float(nz.min()) >= 2.0 ** -126 and float(nz.max()) <= 2.0 ** 126 and int(np.abs(d).max()) == 2
    assert torch.equal(x.to(torch.bfloat16).double(), x), "x is not exact in bf16"
    return wq, torch.from_numpy(ws), x


@functools.lru_cache(maxsize=3)
def case(family, N, K, B=1):
    """dict: wq [N, K / 2], ws [N, K / 32] uint8, x [B, K] bf16, ref [B, N] float64 = x @ decode^T; for B <= 4 also bias [N],
    R [B, N] bf16 and ref_br = (ref + bias) + R.  The GEMM tests build B = 64 and take x[:B]."""
    rng = G._rng(41, FAMILIES.index(family), N, K, B)
    wq, ws, x = _operands(family, N, K, B, rng)
    ref, bound = matmul_ref(wq, ws, x)
    assert bound < 2 ** 21, f"a partial sum could reach {bound}"
    assert torch.equal(ref * 8, (ref * 8).round())
    out = dict(wq=wq, ws=ws, x=x.to(torch.bfloat16), ref=G._exact_f32(ref, "sum"), bound=bound)
    if B <= 4:
        bias, R = G._quarters((N,), rng), G._quarters((B, N), rng)
        out.update(bias=bias.to(torch.bfloat16), R=R.to(torch.bfloat16), ref_br=G._epilogue(ref, None, bias, R))
    return out


@functools.lru_cache(maxsize=3)
def norm_case(N, K, B=1):
    """Narrow weights behind the exact RMSNorm prologue: x [B, K] = +-c_b, norm_w [K]; ref = (sign * norm_w) @ decode^T,
    ref_b = ref + bias."""
    rng = G._rng(42, N, K, B)
    wq, ws, _ = _operands("narrow", N, K, 1, rng)
    x, nw, staged = G.norm_operands(K, B, rng)
    ref, bound = matmul_ref(wq, ws, staged)
    assert bound < 2 ** 21
    bias = G._quarters((N,), rng)
    return dict(wq=wq, ws=ws, x=x, norm_w=nw, ref=G._exact_f32(ref, "sum"), bias=bias.to(torch.bfloat16),
                ref_b=G._exact_f32(ref + bias[None, :], "+ bias"))


def padded(wq, ws):
    """The [:, :K / 2] / [:, :K / 32] views of wider buffers (ldq = K / 2 + 16, lds = K / 32 + 3) filled with 0xFF, on the
    operands' device (a copy to another device would drop the padding)."""
    wide = torch.full((wq.shape[0], wq.shape[1] + 16), 0xFF, dtype=torch.uint8, device=wq.device)
    wide[:, :wq.shape[1]] = wq
    swide = torch.full((ws.shape[0], ws.shape[1] + 3), 0xFF, dtype=torch.uint8, device=ws.device)
    swide[:, :ws.shape[1]] = ws
    return wide[:, :wq.shape[1]], swide[:, :ws.shape[1]]


# ----------------------------------------------------------------------------- SwiGLU
_UP_LEVELS = [12, 8, 6, 4, 3, 2, 1]        # E2M1 magnitudes x 1/4, in units of 2^-3


@functools.lru_cache(maxsize=3)
def swiglu_case(N, K):
    """dict: x [K] bf16, wq / ws in the 16-interleaved layout, gate / up [N / 2] float64 (exact), ref = silu(gate) * up."""
    I, nblk = N // 2, K // 32
    rng = G._rng(43, N, K)
    x = torch.from_numpy(rng.integers(-8, 9, K).astype(np.float64))
    ucols = np.sort(rng.permutation(K)[:8])
    xu = rng.integers(0, 2, 8) * 2.0 - 1
    x[ucols] = torch.from_numpy(xu)
    ublk = ucols // 32
    rows = np.arange(I)
    ws_g = rng.integers(125, 130, (I, nblk)).astype(np.int64)
    ws_u = rng.integers(125, 130, (I, nblk)).astype(np.int64)
    for b in np.unique(ublk):
        ws_g[:, b] = rng.integers(126, 129, I)          # 1/2, 1, 2: -2 .. 2 divided by it is an E2M1 value
        ws_u[:, b] = 125                                # 1/4: the E2M1 grid in units of 2^-3
    # gate: target t in -2 .. 2 on two of the unit columns
    t = ((rows * 7 + rng.integers(0, 5)) % 5 - 2).astype(np.float64)
    c1 = rng.integers(0, 8, I)
    c2 = (c1 + rng.integers(1, 8, I)) % 8
    X1, X2 = 2.0 ** (ws_g[rows, ublk[c1]] - 127), 2.0 ** (ws_g[rows, ublk[c2]] - 127)
    e2m1 = E2M1.numpy()
    code_a = rng.integers(0, 16, I)
    code_a[code_a == 8] = 0
    q = (t - e2m1[code_a] * X1 * xu[c1]) * xu[c2] / X2
    bad = ~np.isin(q, e2m1)
    code_a[bad] = 0
    q = (t - e2m1[code_a] * X1 * xu[c1]) * xu[c2] / X2
    assert np.isin(q, e2m1).all()
    code_r = np.array([_CODE_OF[float(v)] for v in q])
    cg = np.zeros((I, K), dtype=np.uint8)
    cg[rows, ucols[c1]] = code_a
    cg[rows, ucols[c2]] = code_r
    # up: dense codes, the unit columns then adjusted so that the sum in units of 2^-3 is i (mod 32), non-zero
    cu = rng.integers(0, 16, (I, K)).astype(np.uint8)
    cu[:, ucols] = 0
    xs = x.numpy()
    s8 = (e2m1[cu].reshape(I, nblk, 32) * 2.0 ** (ws_u - 127)[..., None]).reshape(I, K) @ xs * 8
    assert np.array_equal(s8, np.round(s8))
    d = (rows - s8) % 32
    d = np.where(d >= 16, d - 32, d)
    d = np.where(s8 + d == 0, d + 32, d)                # -16 .. 47
    for j in range(8):
        take = np.zeros(I)
        for lvl in _UP_LEVELS:
            take = np.where((take == 0) & (np.abs(d) >= lvl), lvl * np.sign(d), take)
        v = take / 2 * xu[j]                            # the code's value: v x 1/4 x xu = take x 2^-3
        cu[:, ucols[j]] = np.array([_CODE_OF[float(a)] for a in v])
        d = d - take
    assert (d == 0).all(), "up adjustment out of range"
    wq = pack(G.interleave16(torch.from_numpy(cg), torch.from_numpy(cu)))
    ws = G.interleave16(torch.from_numpy(ws_g), torch.from_numpy(ws_u)).to(torch.uint8)
    have = set(torch.unique(ws).tolist())          # (K = 64: both blocks hold unit columns, so 129 does not occur)
    assert len(torch.unique(unpack(wq))) == 16 and {125, 126, 127, 128} <= have <= {125, 126, 127, 128, 129}
    both, bound = matmul_ref(wq, ws, x[None, :])
    assert bound < 2 ** 21
    both = both[0].reshape(I // 16, 2, 16)
    gate, up = both[:, 0].reshape(I), both[:, 1].reshape(I)
    assert np.array_equal(gate.numpy(), t) and len(torch.unique(gate)) == 5
    up8 = up * 8
    assert bool((up8 != 0).all()) and torch.equal(up8 % 32, torch.from_numpy(rows).double() % 32)
    win = up[:I // 32 * 32].reshape(-1, 32)
    assert bool((win.sort(1).values.diff(dim=1) != 0).all()), "up values repeat inside a group of 32 outputs"
    G._exact_f32(gate, "gate"), G._exact_f32(up, "up")
    return dict(x=x.to(torch.bfloat16), wq=wq, ws=ws, gate=gate, up=up, ref=gate * torch.sigmoid(gate) * up)


# ----------------------------------------------------------------------------- every code with every scale byte
EVERY_N, EVERY_K, EVERY_B = 16 * len(BYTES), 32 * len(BYTES), 5


@functools.lru_cache(maxsize=1)
def every_code_case():
    """dict: wq [3968, 3968], ws [3968, 248], x [5, 7936] bf16, want [5, 3968] float64 (see the module docstring)."""
    nb = len(BYTES)
    j, c = np.repeat(np.arange(nb), 16), np.tile(np.arange(16), nb)
    codes = torch.zeros((EVERY_N, EVERY_K), dtype=torch.uint8)
    codes[torch.arange(EVERY_N), torch.from_numpy(j * 32 + (c + j) % 32)] = torch.from_numpy(c.astype(np.uint8))
    wq = pack(codes)
    ws = torch.tensor(BYTES, dtype=torch.uint8)[None, :].repeat(EVERY_N, 1)
    row = torch.ldexp(torch.ones(EVERY_B, dtype=torch.float64), torch.arange(EVERY_B) % 3)
    x = row[:, None] * e8m0(254 - ws[0].to(torch.int32)).repeat_interleave(32)[None, :]
    assert torch.equal(x.to(torch.bfloat16).double(), x) and float(x.max()) <= 2.0 ** 126 and float(x.min()) >= 2.0 ** -123
    want = row[:, None] * E2M1[torch.from_numpy(c)][None, :]
    ref, bound = matmul_ref(wq, ws, x)
    assert torch.equal(ref, want) and bound <= 24
    assert len({(int(a), int(b)) for a, b in zip(c, ws[0][torch.from_numpy(j)])}) == 16 * nb
    return dict(wq=wq, ws=ws, x=x.to(torch.bfloat16), want=want)
