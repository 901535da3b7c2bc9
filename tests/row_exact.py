"""Inputs and float64 references for the row-pass kernels between the GEMMs: the norms (csrc/norm.hip), the fp8 activation
quantiser (vis_quant_rows_fp8, csrc/gemm_fp8.hip) and the rotary split (csrc/rope.hip).

The library is built with the compiler's default fp contraction and rsqrtf is a 1-ulp instruction, so the norm arithmetic
cannot be emulated bit for bit.  Every norm reference therefore returns, per output element, the LOWEST and the HIGHEST
bf16 value a correct kernel may write; a test asserts lo <= got <= hi on the decoded values, which is an exact comparison
wherever lo == hi.  Everything is float64; the slacks follow from the kernels' structure (u = 2^-24, the f32 unit
roundoff), none of them is measured:

* sums: a lane adds at most 8 CH terms one after the other, six wave-reduction steps follow, and the statistics take two
  more roundings (the 1 / N product): relative slack  g = (8 CH + 8) u  on a sum of non-negative terms (contraction only
  removes roundings).  CH = chunks per lane of the instantiation that runs (`chunks`), at most 10.  The signed sum behind
  the mean gets the absolute slack  dm = g sum|x| / N - except on rows whose signed sum is exact in f32 whatever the order
  (`exact_sum`: all elements multiples of one quantum q, sum|x| <= 2^24 q), where only the 1 / N product rounds:
  dm = 3 u |mean|.  The cancellation row 100 + Gaussian is such a row (steps of 1/2, sum < 2^19); with the general bound
  its dm = 100 g would equal a tenth of its sigma and a quarter of its elements would be ambiguous.
* rstd = rsqrtf(sum * inv_n + eps): relative  RSTD = g / 2 + 2^-22  - half the sum's slack through the square root, and
  2^-22 = 4 u for the rsq instruction (1 ulp = 2 u) and the roundings of inv_n, the product and the sum with eps (3 u,
  halved).  With CH = 10: RSTD = 48 u = 3 * 2^-20 < 2^-17.  The LayerNorm variance is taken around the kernel's own mean,
  which adds at most dm^2 to it.
* output: the expression is evaluated at the corners of the (mean, rstd) box; 2^-22 (|scaled term| + |bias|) covers the
  four f32 roundings of  (x - mean) * rstd * w + b;  the lowest and the highest value are rounded to bf16 (monotone, so
  the corners are enough).  RMSNorm rounds twice, as HF and the kernel do: bf16(x * rstd), then bf16(that * w) - the
  second product of two bf16 values is exact in f32 and gets no slack (a slack there would only turn exact ties, which
  round-to-nearest-even decides, into ambiguity).
* eps reaches the kernels as an f32: the references use float32(eps).

A case is valid only if at most AMBIGUOUS_CAP = 2 % of its elements have lo != hi (tests/test_row_exact.py asserts it for
every table entry, on the CPU, from the reference alone).  Roughly 2 RSTD / 2^-8 per rounding stage.  Observed shares (max over the table, CPU):
    rmsnorm 0.15 %   layernorm 0.55 %   rmsnorm_heads 0.00 %   finalize_norm 1.39 % (one element of the 72 at N = 8)
    fused quantiser bytes 0.02 % (RMSNorm) / 0.09 % (LayerNorm)   general-angle rope 0.06 %

The quantiser without a norm is emulated exactly in float32 (max, one correctly rounded division, one product, e4m3
round-to-nearest-even saturating at 448).  The rotary tests use tables from {0, +-1, +-1/2} and qkv values k / 4, |k| <= 8:
every product and sum is exact in f32 and in bf16 whatever the contraction (`rope_build` asserts it from float64).

CPU only: float64 torch and numpy, never the library under test.
"""
import dataclasses
import functools

import numpy as np
import torch

NAN_BF16 = 0x7FC1          # a quiet NaN with a payload bit, as int16: the fill of every bf16 buffer
FILL_U8 = 0xAA             # the fill of every byte output
U = 2.0 ** -24
CH_MAX = 10
OUT_SLACK = 2.0 ** -22
AMBIGUOUS_CAP = 0.02


def sum_slack(ch=CH_MAX):
    return (8 * ch + 8) * U


def rstd_slack(ch=CH_MAX):
    return sum_slack(ch) / 2 + 2.0 ** -22


assert rstd_slack(CH_MAX) == 3 * 2.0 ** -20 < 2.0 ** -17


def chunks(N, entry="norm"):
    """Chunks per lane (template CH) of the instantiation an entry point runs at row length N."""
    ch = (N // 8 + 63) // 64
    if entry == "norm":                      # norm_rows_kernel<., 3 | 7 | 10, .>
        return 3 if ch <= 3 else 7 if ch <= 7 else 10
    if entry == "quant":                     # quant_rows_fp8_kernel<3 | 8>
        return 3 if ch <= 3 else 8
    if entry == "heads":                     # one chunk per lane, a 16-lane row per head
        return 1
    assert entry == "finalize"               # <., 3, 2> or the wide kernel's ten guarded chunks
    return CH_MAX


def bf16r(t):
    """float64 -> the nearest bf16 (through f32, as the kernels round), back as float64.  Monotone."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


# ----------------------------------------------------------------------------- layouts
class Emb:
    """A [rows, cols] tensor inside a flat sentinel-filled buffer: element (r, c) at offset + r * ld + c, `below` rows after."""

    def __init__(self, t, ld, below=2, offset=8):
        rows, cols = t.shape
        assert ld >= cols
        self.rows, self.cols, self.ld, self.offset = rows, cols, ld, offset
        n = offset + (rows + below) * ld
        if t.dtype == torch.bfloat16:
            self.flat = torch.full((n,), NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
        elif t.dtype == torch.uint8:
            self.flat = torch.full((n,), FILL_U8, dtype=torch.uint8)
        else:
            assert t.dtype == torch.float32
            self.flat = torch.full((n,), float("nan"), dtype=torch.float32)
        self.view(self.flat).copy_(t)

    def view(self, flat):
        return flat.as_strided((self.rows, self.cols), (self.ld, 1), self.offset)

    def outside(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool)
        self.view(m).fill_(False)
        return m


def raw(t):
    """The bits of a tensor, for comparisons that NaN sentinels must survive."""
    return t.view({2: torch.int16, 1: torch.uint8, 4: torch.int32}[t.element_size()])


def sentinels_intact(emb, flat_after):
    out = emb.outside()
    return torch.equal(raw(flat_after.cpu())[out], raw(emb.flat)[out])


def blank(shape, dtype=torch.bfloat16):
    """A sentinel-filled tensor."""
    if dtype == torch.bfloat16:
        return torch.full(shape, NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    assert dtype == torch.uint8
    return torch.full(shape, FILL_U8, dtype=torch.uint8)


# ----------------------------------------------------------------------------- norm inputs
FAMILY = ("gauss3", "eps", "cancel", "zero", "last_chunk", "elem0")
EXTRA = ("gauss3", "eps", "last_chunk", "elem0")     # the rows beyond the family: fresh draws of these
NORM_N = (8, 512, 520, 1280, 1536, 1544, 3584, 3592, 5120)
NORM_ROWS = (9, 13)
NORM_EPS = (1e-6, 1e-5)


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def family_row(kind, N, rng):
    g = rng.standard_normal(N)
    if kind == "gauss3":
        return g * 3.0
    if kind == "eps":                       # mean square ~ 2^-20 ~ 1e-6: the row that feels eps
        return g * 2.0 ** -10
    if kind == "cancel":                    # |mean| = 100 sigma: E[x^2] - mean^2 cancels
        return 100.0 + g
    r = np.zeros(N)
    if kind == "last_chunk":                # only the last 16-byte chunk is non-zero
        r[N - 8:] = g[:8] * 3.0
    elif kind == "elem0":
        r[0] = 3.0 if g[0] >= 0 else -3.0
    else:
        assert kind == "zero"
    return r


def row_kinds(rows):
    return FAMILY + tuple(EXTRA[i % len(EXTRA)] for i in range(rows - len(FAMILY)))


@functools.lru_cache(maxsize=None)
def norm_inputs(N, rows, seed=0):
    """(x [rows, N], w [N], b [N]) bf16: the row families, then fresh draws of EXTRA up to `rows`."""
    rng = _rng(seed, N, rows, 101)
    x = np.stack([family_row(k, N, rng) for k in row_kinds(rows)])
    w, b = rng.standard_normal(N), rng.standard_normal(N)
    return tuple(torch.from_numpy(a).to(torch.bfloat16) for a in (x, w, b))


def heads_inputs(tokens, heads, extra, seed=0):
    """x [tokens, heads * 128 + extra], w [128] bf16: the head slices cycle through the row families."""
    rng = _rng(seed, tokens, heads, extra, 505)
    x = rng.standard_normal((tokens, heads * 128 + extra))
    for t in range(tokens):
        for h in range(heads):
            x[t, h * 128:(h + 1) * 128] = family_row(FAMILY[(t * heads + h) % len(FAMILY)], 128, rng)
    return torch.from_numpy(x).to(torch.bfloat16), torch.from_numpy(rng.standard_normal(128)).to(torch.bfloat16)


# ----------------------------------------------------------------------------- norm references
def norm_interval(x, w, b, eps, ch=CH_MAX, slack=True):
    """(lo, hi) float64 [rows, N], bf16-valued: what RMSNorm (b None) or LayerNorm of the bf16 rows x may write.
    slack=False: the midpoint, lo == hi == the correctly rounded float64 result."""
    x, w = x.double(), w.double()
    g, rs, so = (sum_slack(ch), rstd_slack(ch), OUT_SLACK) if slack else (0.0, 0.0, 0.0)
    eps = float(np.float32(eps))
    if b is None:
        r0 = ((x * x).mean(1, keepdim=True) + eps).rsqrt()
        t1, t2 = x * (r0 * (1 - rs)), x * (r0 * (1 + rs))
        s = so * (x * r0).abs()
        lo1, hi1 = bf16r(torch.minimum(t1, t2) - s), bf16r(torch.maximum(t1, t2) + s)
        y1, y2 = bf16r(lo1 * w), bf16r(hi1 * w)          # bf16 x bf16: exact in f32, one rounding
        return torch.minimum(y1, y2), torch.maximum(y1, y2)
    b = b.double()
    mean = x.mean(1, keepdim=True)
    dm = g * x.abs().mean(1, keepdim=True)
    if slack:
        dm = torch.where(exact_sum(x), 3 * U * mean.abs(), dm)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rhi = (var + eps).rsqrt() * (1 + rs)
    rlo = (var + dm * dm + eps).rsqrt() * (1 - rs)
    c = torch.stack([(x - m) * r * w for m in (mean - dm, mean + dm) for r in (rlo, rhi)])
    tmin, tmax = c.amin(0), c.amax(0)
    s = so * (torch.maximum(tmin.abs(), tmax.abs()) + b.abs())
    return bf16r(tmin + b - s), bf16r(tmax + b + s)


def exact_sum(x):
    """bool [rows, 1]: the row's signed sum is exact in f32 in ANY order - every element is a multiple of the row's smallest
    bf16 quantum q (2^-7 of the smallest non-zero element's binade) and sum|x| <= 2^24 q, so every partial sum is a multiple
    of q below 2^24 q, a float32 number.  True for the all-zero and the single-element rows and for the cancellation row
    (values near 100 in steps of 1/2)."""
    a = x.abs()
    e = torch.frexp(torch.where(a > 0, a, torch.full_like(a, float("inf"))).amin(1, keepdim=True))[1] - 1
    q = torch.ldexp(torch.ones_like(a[:, :1]), e - 7)
    total = a.sum(1, keepdim=True)
    return (total == 0) | (total <= 2.0 ** 24 * q)


def ambiguous_share(lo, hi):
    return float((lo != hi).double().mean())


def outside(got, lo, hi):
    """bool [...]: got not in [lo, hi] (a NaN is outside)."""
    return ~((lo <= got) & (got <= hi))


MUTANTS = ("n_minus_1", "no_eps", "eps_outside", "one_pass_f32", "pad512")


def norm_mutant(kind, x, w, b, eps):
    """A subtly wrong norm in float64 (one_pass_f32: its variance in sequential float32), rounded to bf16 like the right one."""
    x, w = x.double(), w.double()
    N = x.shape[1]
    eps = float(np.float32(eps))
    n_stat = {"n_minus_1": N - 1, "pad512": (N + 511) // 512 * 512}.get(kind, N)
    if b is None:
        mean = torch.zeros(x.shape[0], 1, dtype=torch.float64)
        var = (x * x).sum(1, keepdim=True) / n_stat
    else:
        mean = x.sum(1, keepdim=True) / (N if kind == "n_minus_1" else n_stat)
        if kind == "one_pass_f32":
            x32 = x.numpy().astype(np.float32)
            ss = np.cumsum(x32 * x32, axis=1, dtype=np.float32)[:, -1] / np.float32(N)
            m32 = np.cumsum(x32, axis=1, dtype=np.float32)[:, -1] / np.float32(N)
            var = torch.from_numpy((ss - m32 * m32).astype(np.float64))[:, None]
        elif kind == "pad512":              # the pad zeros take part: sum (x - mean)^2 over n_stat elements
            var = (((x - mean) ** 2).sum(1, keepdim=True) + (n_stat - N) * mean ** 2) / n_stat
        else:
            var = ((x - mean) ** 2).sum(1, keepdim=True) / n_stat
    if kind == "no_eps":
        rstd = var.rsqrt()
    elif kind == "eps_outside":
        rstd = 1.0 / (var.sqrt() + eps)
    else:
        rstd = (var + eps).rsqrt()
    if b is None:
        return bf16r(bf16r(x * rstd) * w)
    return bf16r((x - mean) * rstd * w + b.double())


def mutant_targets(kind, layernorm, N, rows):
    """Row indices on which `kind` must leave the interval, or None where it cannot be told from a correct kernel:
    * n_minus_1 / pad512 change rstd by >= 1 / (2 N) ~ 1e-4 (pad512 only where N % 512 != 0): the Gaussian rows, whose N
      roundings at 2^-8 cannot all hide that.  RMSNorm's first rounding bf16(x * rstd) sees only the 128 significands a
      bf16 row has, whatever N: a shift of rstd below ~1e-4 crosses a rounding boundary of about one of them, so N - 1 (the
      LayerNorm variance's mutant) is asked of RMSNorm only up to N = 520 (shift >= 9.6e-4);
    * no_eps / eps_outside move rstd by a factor on the rows whose mean square is ~ eps, and by ~ 1e-7 elsewhere;
    * one_pass_f32 is LayerNorm's, on the cancellation row, from the N at which its float32 sums stop being exact
      (x^2 ~ 1e4 in steps of 1/4: a sum of more than ~400 of them needs more than 24 bits)."""
    kinds = row_kinds(rows)
    pick = lambda *names: [i for i, k in enumerate(kinds) if k in names]
    if kind == "n_minus_1":
        if layernorm:
            return pick("gauss3", "eps", "cancel")
        return pick("gauss3") if N <= 520 else None
    if kind == "pad512":
        return None if N % 512 == 0 else pick("gauss3", "eps")
    if kind in ("no_eps", "eps_outside"):
        return pick("eps")
    assert kind == "one_pass_f32"
    return pick("cancel") if layernorm and N >= 512 else None


# ----------------------------------------------------------------------------- split-K finalisation
FIN_N = (8, 1280, 1536, 1544, 3584, 5120)
FIN_KS = (1, 2, 3, 8)
FIN_M = 9


@functools.lru_cache(maxsize=None)
def finalize_inputs(N, ks, seed=0):
    """(partials [ks, M, N] f32, bias [N], R [M, N], w [N], b [N] bf16)."""
    rng = _rng(seed, N, ks, 202)
    part = torch.from_numpy(rng.standard_normal((ks, FIN_M, N)).astype(np.float32))
    bf = lambda *s: torch.from_numpy(rng.standard_normal(s)).to(torch.bfloat16)
    return part, bf(N), bf(FIN_M, N), bf(N), bf(N)


def finalize_x(part, bias, R):
    """x = bf16(((p0 + p1) + ...) + bias) + R): f32 additions in the kernels' fixed order (additions do not contract)."""
    a = part[0].clone()
    for k in range(1, part.shape[0]):
        a += part[k]
    if bias is not None:
        a += bias.float()[None, :]
    if R is not None:
        a += R.float()
    return a.to(torch.bfloat16)


# ----------------------------------------------------------------------------- fp8 row quantiser
QUANT_K = (8, 1536, 1544, 2048, 2056, 4096, 4104, 6144, 6152, 12288, 12296, 18944, 20480, 20488)
FUSED_K = (8, 256, 1280, 1536, 1544, 3584, 4096)
PLANT = 3.0


def quant_kernel(K):
    """The kernel vis_quant_rows_fp8 runs for a row of K elements without a norm (default dispatch)."""
    ch = (K // 8 + 63) // 64
    if ch <= 3:
        return "kernel<3>"
    if ch <= 4:
        return "kernel<8>"
    if ch <= 8:
        return "wide<8>"
    if ch <= 12:
        return "wide<12>"
    if ch <= 40:
        return "rowwg<6>" if (K // 8 + 255) // 256 <= 6 else "rowwg<10>"
    return "kernel<8> streaming"


def plant_positions(K):
    nch = K // 8
    pos = {0, 7, 511, 512, K - 8, K - 1}
    pos |= {512 * w for w in range(4)}                       # chunk 64 w: the first of wave w in the row-workgroup kernel
    pos |= {8 * 64 * ((nch - 1) // 64), 8 * 256 * ((nch - 1) // 256)}   # first chunk of the last round: per wave / per workgroup
    return sorted(p for p in pos if 0 <= p < K)


@functools.lru_cache(maxsize=None)
def quant_inputs(K, seed=0):
    """(x [rows, K] bf16, planted column per row or -1): one row per planted position (Gaussian clipped to |x| <= 1 and one
    +-3 at the position), an all-zero row, two plain Gaussian rows times 2."""
    rng = _rng(seed, K, 303)
    pos = plant_positions(K)
    x = np.clip(rng.standard_normal((len(pos) + 3, K)), -1.0, 1.0)
    for r, p in enumerate(pos):
        x[r, p] = PLANT if r % 2 == 0 else -PLANT
    x[len(pos)] = 0.0
    x[len(pos) + 1:] = rng.standard_normal((2, K)) * 2.0
    return torch.from_numpy(x).to(torch.bfloat16), pos + [-1, -1, -1]


def e4m3_bytes(t32):
    """float32 -> e4m3 bytes, round to nearest even, saturating at +-448 (v_cvt_pk_fp8_f32)."""
    return t32.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_value(bytes_):
    return bytes_.view(torch.float8_e4m3fn).to(torch.float64)


def quant_scale(amax32):
    """numpy float32: max(amax / 448, 1e-12), one correctly rounded division."""
    return np.maximum(amax32.astype(np.float32) / np.float32(448.0), np.float32(1e-12))


def quant_bytes(v, scale32):
    """e4m3(v * (1.0f / scale)) for bf16-valued rows v (any float dtype) and numpy float32 scales [rows]."""
    inv = (np.float32(1.0) / scale32.astype(np.float32)).astype(np.float32)
    return e4m3_bytes(v.to(torch.float32) * torch.from_numpy(inv)[:, None])


def quant_expect(x):
    """(bytes [rows, K] uint8, scale [rows] numpy f32) of the quantiser without a norm: exact."""
    sc = quant_scale(x.float().abs().amax(1).numpy())
    return quant_bytes(x, sc), sc


def fused_scale_interval(lo, hi):
    """[s_lo, s_hi] numpy float32 for the row scale of a normed row known as [lo, hi]: the max of the smallest and of the
    largest |value| each element may have, / 448, widened by one f32 ulp."""
    small = torch.where((lo <= 0) & (hi >= 0), torch.zeros_like(lo), torch.minimum(lo.abs(), hi.abs())).amax(1)
    large = torch.maximum(lo.abs(), hi.abs()).amax(1)
    s_lo, s_hi = quant_scale(small.numpy()), quant_scale(large.numpy())
    floor = s_hi == np.float32(1e-12)                        # both bounds on the floor (an all-zero normed row): exact
    return (np.where(floor, s_lo, np.nextafter(s_lo, np.float32(0))).astype(np.float32),
            np.where(floor, s_hi, np.nextafter(s_hi, np.float32(np.inf))).astype(np.float32))


def fused_byte_interval(lo, hi, scale32):
    """Decoded e4m3 bounds of every byte, given the scale the kernel returned (or, on the CPU, the midpoint's)."""
    return e4m3_value(quant_bytes(lo, scale32)), e4m3_value(quant_bytes(hi, scale32))


# ----------------------------------------------------------------------------- rotary split
@dataclasses.dataclass(frozen=True)
class Rope:
    HD: int
    S: int
    Hq: int
    Hkv: int
    rot: bool = True       # False: cos = sin = None, a pure head split
    ld_pad: int = 0        # ld_qkv - packed width
    k_pos0: int = 0
    vt_col0: int = 0
    v: bool = True
    vt: bool = True
    general: bool = False  # random angles (interval check) instead of the exact tables

    @property
    def id(self):
        f = [n for n, on in (("norot", not self.rot), (f"ld+{self.ld_pad}", self.ld_pad), (f"pos{self.k_pos0}", self.k_pos0),
                             (f"col{self.vt_col0}", self.vt_col0), ("nov", not self.v), ("novt", not self.vt),
                             ("general", self.general)) if on]
        return f"d{self.HD}-s{self.S}-h{self.Hq}+{self.Hkv}" + "".join("-" + n for n in f)

    @property
    def width(self):
        return (self.Hq + 2 * self.Hkv) * self.HD


ROPE_S = (1, 15, 16, 17, 63, 64, 65, 129)
ROPE_HEADS = ((1, 0), (0, 1), (2, 1), (6, 1), (7, 1), (8, 1), (11, 1), (12, 1), (28, 4), (32, 8))


def _rope_cases():
    c = []
    for HD in (128, 80):
        # every S and every head pair with this HD; the layout switches rotate over them
        pairs = [(S, ROPE_HEADS[(i * 3 + (HD == 80)) % 10]) for i, S in enumerate(ROPE_S)]
        pairs += [(ROPE_S[(j * 5 + 2 + (HD == 80)) % 8], h) for j, h in enumerate(ROPE_HEADS)]
        for n, (S, (Hq, Hkv)) in enumerate(pairs):
            c.append(Rope(HD, S, Hq, Hkv, ld_pad=64 * (n % 2), k_pos0=3 * (n % 3 == 1), vt_col0=64 * (n % 4 == 2)))
        c.append(Rope(HD, 65, 2, 1, rot=False, ld_pad=64))
        c.append(Rope(HD, 17, 0, 1, rot=False, k_pos0=3))
        c.append(Rope(HD, 65, 6, 1, v=False, vt_col0=64))
        c.append(Rope(HD, 17, 2, 1, vt=False, k_pos0=3))
    return c


ROPE_CASES = _rope_cases()
ROPE_GENERAL = (Rope(128, 65, 7, 1, general=True, ld_pad=64, k_pos0=3), Rope(80, 65, 11, 1, general=True, ld_pad=64))
MANY_CASES = [(HD, S, nreq, 6 if HD == 128 else 11, 2 if HD == 128 else 1)
              for HD in (128, 80) for S in (17, 65) for nreq in (1, 3, 8)]     # (HD, S, nreq, Hq, Hkv)


def vt_key_order(n_cols):
    """key_of_col [n_cols]: inside each aligned group of 32 keys, key 16 a + 4 h + r sits at column 8 h + 4 a + r
    (csrc/rope.hip, the layout comment) - written from that sentence, not from the library."""
    key = torch.empty(n_cols, dtype=torch.long)
    for base in range(0, n_cols, 32):
        for a in range(2):
            for h in range(4):
                for r in range(4):
                    key[base + 8 * h + 4 * a + r] = base + 16 * a + 4 * h + r
    return key


def rope_inputs(case, seed=0, rows=None):
    """(qkv [rows or S, width] bf16, cos, sin [S, HD] f32 or None)."""
    rng = _rng(seed, case.HD, case.S, case.Hq, case.Hkv, 404)
    n = case.S if rows is None else rows
    if case.general:
        qkv = rng.standard_normal((n, case.width))
        ang = rng.random((case.S, case.HD)) * 6.28          # its own angle for every channel: first half != second half
        cos, sin = np.cos(ang), np.sin(ang)
    else:
        qkv = rng.integers(-8, 9, (n, case.width)) / 4.0
        table = np.array([0.0, 1.0, -1.0, 0.5, -0.5])
        cos, sin = table[rng.integers(0, 5, (case.S, case.HD))], table[rng.integers(0, 5, (case.S, case.HD))]
    qkv = torch.from_numpy(qkv).to(torch.bfloat16)
    if not case.rot:
        return qkv, None, None
    return qkv, torch.from_numpy(cos).float(), torch.from_numpy(sin).float()


ROPE_MUTANTS = ("half_table", "sign", "head_off", "vt_plain")


def rope_expect(case, qkv, cos, sin, mutant=None, slack=0.0):
    """float64 expectation of one request: dict q [Hq, S, HD], k, v [Hkv, S, HD], vt [Hkv, HD, round_up(S, 64)] in the
    kernel's column order (pad columns zero); with slack > 0, q and k are (lo, hi) pairs of bf16-valued bounds."""
    S, HD, Hq, Hkv = case.S, case.HD, case.Hq, case.Hkv
    half = HD // 2
    x = qkv.double().reshape(S, Hq + 2 * Hkv, HD)
    if mutant == "head_off":
        x = torch.roll(x, -1, 1)
    rot = x[:, :Hq + Hkv]
    if cos is None:
        c = torch.ones(S, 1, HD, dtype=torch.float64)
        s = torch.zeros(S, 1, HD, dtype=torch.float64)
    else:
        c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    if mutant == "half_table":
        c, s = torch.cat((c[..., :half], c[..., :half]), -1), torch.cat((s[..., :half], s[..., :half]), -1)
    sign = -1.0 if mutant == "sign" else 1.0
    rh = torch.cat((-rot[..., half:], rot[..., :half]), -1) * sign          # rotate_half
    out = rot * c + rh * s
    v = x[:, Hq + Hkv:].permute(1, 0, 2)
    ld = (S + 63) // 64 * 64
    plain = torch.zeros(Hkv, HD, ld, dtype=torch.float64)
    plain[:, :, :S] = v.permute(0, 2, 1)
    vt = plain if mutant == "vt_plain" else plain[:, :, vt_key_order(ld)]
    if slack:
        e = slack * ((rot * c).abs() + (rh * s).abs())
        lo, hi = bf16r(out - e).permute(1, 0, 2), bf16r(out + e).permute(1, 0, 2)
        return dict(q=(lo[:Hq], hi[:Hq]), k=(lo[Hq:], hi[Hq:]), v=v, vt=vt)
    out = out.permute(1, 0, 2)
    return dict(q=out[:Hq], k=out[Hq:], v=v, vt=vt)


@functools.lru_cache(maxsize=4)
def rope_build(case, seed=0):
    """Inputs and the exact expectation of an exact case; asserts that every expected value is a bf16 number."""
    assert not case.general
    qkv, cos, sin = rope_inputs(case, seed)
    exp = rope_expect(case, qkv, cos, sin)
    for name in ("q", "k", "v", "vt"):
        assert torch.equal(exp[name], bf16r(exp[name])), f"{case.id}: expected {name} not exact in bf16"
    return qkv, cos, sin, exp
