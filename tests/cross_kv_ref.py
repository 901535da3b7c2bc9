"""Restatements, from the stated definition, of the fp8 cross-attention keys / values (csrc/cross_attn.hip, MllamaEngine
cross_kv="fp8"): the row quantiser, the attention over codes and scales in float64, a float32 emulation of the kernel's
order of operations, and the slack the comparison allows.

* Row quantiser (vis_quant_rows_fp8 without a norm, over rows of 128): scale = max(amax / 448, 1e-12) with one correctly rounded
  f32 division, code = e4m3(x * (1 / scale)), both products in f32, round to nearest even, saturating at +-448.  An all-zero row
  has scale 1e-12 and codes 0.
* Attention of one new token, per query head g over keys j < nkeys of its kv head:
      q^ = bf16(bf16(q * rstd) * w)   rstd = 1 / sqrt(mean(q^2) + eps)             (HF q_norm rounding)
      s_j = kscale_j * sum_d q^_d kcode_jd * (scale * log2 e)    p_j = 2^(s_j - max s)
      o_d = sum_j (p_j vscale_j) vcode_jd / sum_j p_j
  P is never rounded below f32 (the split decode attention's softmax scheme); the output is one bf16 rounding of o.
* Slack, derived and never measured (u = 2^-24, the f32 unit roundoff; first order, every count rounded up).  The bound
  inputs make sum_d q^_d kcode_jd exact in f32 in any order (integers below 2^24) and scale * log2 e exactly 2^-3.  A key's
  weight p_j then carries, relative: the rounding of acc * kscale (|s_j| u in the exponent = ln 2 |s_j| u), the subtraction
  s_j - m in the split (<= 2 Smax u in the exponent), the split's exp2 (2 u), the combine's m - M (2 Smax u in the exponent)
  and its exp2 (2 u): eta = (5 ln 2 Smax + 4) u <= (3.5 Smax + 4) u.  The numerator adds one rounding for p * vscale, one
  for the product with the code, 8 + 7 accumulations inside the split, one product and up to NS accumulations in the
  combine and one for its two halves: eta + 19 + NS.  The denominator adds 6 (the split's sum tree), 1, 6 + 3 (the combine's
  trees): eta + 16; the division one more.  Together rel(Smax, NS) = (7 Smax + NS + 48) u, relative to
  a_d = sum_j p_j vscale_j |vcode_jd| / sum_j p_j.  The kernel may write any bf16 in [rne(o - rel a), rne(o + rel a)];
  no element is excluded.
* Arbitrary K codes (general_inputs): the dot product is no longer exact.  Its 128 exact products meet 127 f32 accumulations
  in an order the MFMA does not publish; allowing two units per accumulation (a truncating adder), the score is off by at
  most 256 u Sabs_j with Sabs_j = kscale_j 2^-3 sum_d |q^_d kcode_jd|, a weight by ln 2 times that: 180 Sabs u more in eta,
  360 Sabs u more in rel, Sabs the largest Sabs_j of a valid key: rel = (7 Smax + NS + 48 + 360 Sabs) u.

CPU only: numpy, torch for bf16.  Never imports the library under test."""
import numpy as np
import torch

U = 2.0 ** -24
LN2_F32 = np.float32(0.6931471824645996)
SCALE = float(LN2_F32 * np.float32(0.125))        # scale * 1.4426950408889634f is exactly 0.125 in f32 (asserted by the tests)
LOG2E_F32 = np.float32(1.4426950408889634)
KEYS_PER_SPLIT = 64


def _e4m3_table():
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
        if (c & 0x7F) == 0x7F:
            v = np.nan
        t[c] = -v if c & 0x80 else v
    return t


E4M3 = _e4m3_table()          # code -> value (0x7F, 0xFF: NaN); every finite value is exact in bf16


def e4m3_encode(x32):
    """numpy float32 -> e4m3 codes (uint8): round to nearest even, saturating at +-448; NaN -> 0x7F."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    a = np.minimum(np.abs(x), 448.0)
    _, ex = np.frexp(np.where(a > 0, a, 1.0))                 # a = f * 2^ex, f in [0.5, 1)
    e = np.maximum(ex - 1, -6)                                # exponent of the binade; denormals share 2^-6's quantum
    q = np.rint(a / np.exp2(e - 3.0))                         # RNE (numpy rint), exact division by a power of two
    code = ((e + 7) * 8 + q - 8).astype(np.int64)             # q = 16 carries into the next binade by itself
    code = np.where(a < 2.0 ** -6, np.rint(a * 512.0).astype(np.int64), code)
    code = np.minimum(code, 0x7E)
    code = np.where(np.isnan(x), 0x7F, code | np.where(np.signbit(x), 0x80, 0))
    return code.astype(np.uint8)


def quantize_rows(x):
    """x: rows of bf16 values (numpy float32 [..., K]) -> (codes uint8 [..., K], scales float32 [...])."""
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=-1)
    sc = np.maximum((amax / np.float32(448.0)).astype(np.float32), np.float32(1e-12))
    inv = (np.float32(1.0) / sc).astype(np.float32)
    return e4m3_encode((x * inv[..., None]).astype(np.float32)), sc


def bf16r(x):
    """float64 / float32 numpy -> the nearest bf16 (through f32), as float64."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def q_norm(q, w, eps):
    """HF rounding of the per-head RMSNorm: q [Hq, 128] and w [128] bf16 values -> bf16 values (float64)."""
    q = np.asarray(q, dtype=np.float64)
    rstd = 1.0 / np.sqrt((q * q).mean(axis=-1, keepdims=True) + eps)
    return bf16r(bf16r(q * rstd) * np.asarray(w, dtype=np.float64))


def rel_slack(smax, nsplit):
    return (7.0 * smax + nsplit + 48.0) * U


def dot_abs(qn, kq, ksc, nkeys, scale_log2=0.125):
    """Sabs: the largest kscale_j * scale_log2 * sum_d |q^_d kcode_jd| over heads and valid keys."""
    Hq, Hkv = qn.shape[0], kq.shape[0]
    G = Hq // Hkv
    return max(float(((np.abs(E4M3[kq[h // G, :nkeys]]) @ np.abs(qn[h])) * ksc[h // G, :nkeys].astype(np.float64)).max())
               for h in range(Hq)) * scale_log2


def attention(qn, kq, ksc, vq, vsc, nkeys, scale_log2=0.125):
    """float64 from the definition.  qn [Hq, 128] normed q; codes [Hkv, T, 128] uint8, scales [Hkv, T] f32.
    Returns (o [Hq, 128], a [Hq, 128], smax): the output, its absolute companion and the largest |score| of a valid key."""
    Hq, Hkv = qn.shape[0], kq.shape[0]
    G = Hq // Hkv
    o, a, smax = np.zeros((Hq, 128)), np.zeros((Hq, 128)), 0.0
    for h in range(Hq):
        kv = h // G
        k = E4M3[kq[kv, :nkeys]]
        v = E4M3[vq[kv, :nkeys]]
        s = (k @ qn[h]) * ksc[kv, :nkeys].astype(np.float64) * scale_log2
        p = np.exp2(s - s.max())
        wv = p * vsc[kv, :nkeys].astype(np.float64)
        o[h] = (wv @ v) / p.sum()
        a[h] = (wv @ np.abs(v)) / p.sum()
        smax = max(smax, float(np.abs(s).max()))
    return o, a, smax


def interval(o, a, smax, nkeys, sabs=0.0):
    """The bf16 values the kernel may write: [lo, hi] as float64 arrays.  ``sabs``: dot_abs where the dot product is inexact."""
    nsplit = -(-nkeys // KEYS_PER_SPLIT)
    e = (rel_slack(smax, nsplit) + 360.0 * sabs * U) * a
    return bf16r(o - e), bf16r(o + e)


def attention_f32(qn, kq, ksc, vq, vsc, nkeys, scale_log2=0.125):
    """float32 emulation of the fault-free kernel's order: per split of 64 keys the statistics and the P * V sums (thread
    = key group kg, keys kg + 8 i ascending, then the 8 groups in order), then the combine over the splits that ran (two
    interleaved halves).  The MFMA dot product is taken as exact (the bound inputs make it so).  Returns bf16 values [Hq, 128]."""
    f = np.float32
    Hq, Hkv = qn.shape[0], kq.shape[0]
    G = Hq // Hkv
    out = np.zeros((Hq, 128))
    ns = -(-nkeys // KEYS_PER_SPLIT)
    for h in range(Hq):
        kv = h // G
        ms, ls, os_ = [], [], []
        for sp in range(ns):
            k0, k1 = sp * 64, min(nkeys, sp * 64 + 64)
            acc = (E4M3[kq[kv, k0:k1]] @ qn[h]).astype(f)
            s = ((acc * ksc[kv, k0:k1].astype(f)).astype(f) * f(scale_log2)).astype(f)
            m = s.max()
            e = np.exp2((s - m).astype(f)).astype(f)
            w = (e * vsc[kv, k0:k1].astype(f)).astype(f)
            v = E4M3[vq[kv, k0:k1]].astype(f)
            grp = np.zeros((8, 128), dtype=f)
            for j in range(k1 - k0):
                grp[j % 8] = (grp[j % 8] + (w[j] * v[j]).astype(f)).astype(f)
            o = grp[0]
            for g in range(1, 8):
                o = (o + grp[g]).astype(f)
            ms.append(m); ls.append(e.sum(dtype=f)); os_.append(o)
        M = max(ms)
        wt = [np.exp2(f(m - M)).astype(f) for m in ms]
        half = [np.zeros(128, dtype=f), np.zeros(128, dtype=f)]
        lt = f(0)
        for sp in range(ns):
            half[sp % 2] = (half[sp % 2] + (wt[sp] * os_[sp]).astype(f)).astype(f)
            lt = f(lt + f(wt[sp] * ls[sp]))
        out[h] = bf16r(((half[0] + half[1]).astype(f) / lt).astype(f))
    return out


# ----------------------------------------------------------------------------- inputs of the bound comparison
INT_CODES = np.array([c for c in range(256) if np.isfinite(E4M3[c]) and E4M3[c] == np.rint(E4M3[c]) and abs(E4M3[c]) <= 16
                      and not (c == 0x80)], dtype=np.uint8)      # integer-valued codes up to +-16 (no negative zero)
FINITE_CODES = np.array([c for c in range(256) if np.isfinite(E4M3[c])], dtype=np.uint8)


def bound_inputs(Hq, Hkv, T, seed):
    """Inputs whose q_norm and dot products are exact: q = +-1 in every dim (rstd rounds to 1 in bf16 with a wide margin:
    1 / sqrt(1 + eps) is 1 - eps / 2, bf16's half-ulp below 1 is 2^-9), so q^_d = +-w_d with w small integers; K codes
    integer-valued up to 16: |sum| <= 128 * 4 * 16 < 2^24.  K scales are arbitrary f32 around 2^-3, V codes any finite code, V
    scales arbitrary f32.  Returns q, w (float32 arrays of bf16 values), kq, ksc, vq, vsc."""
    rng = np.random.default_rng([seed, Hq, Hkv, T])
    q = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(Hq, 128))
    w = rng.integers(1, 5, size=128).astype(np.float32)
    kq = rng.choice(INT_CODES, size=(Hkv, T, 128))
    vq = rng.choice(FINITE_CODES, size=(Hkv, T, 128))
    ksc = (rng.uniform(0.5, 1.5, size=(Hkv, T)) * 2.0 ** -3).astype(np.float32)
    vsc = (rng.uniform(0.5, 1.5, size=(Hkv, T)) * 2.0 ** -6).astype(np.float32)
    return q, w, kq, ksc, vq, vsc


def general_inputs(Hq, Hkv, T, seed):
    """bound_inputs with ANY finite K code - fractional, denormal, up to +-448 - and K scales around 2^-8."""
    q, w, _, _, vq, vsc = bound_inputs(Hq, Hkv, T, seed)
    rng = np.random.default_rng([seed, Hq, Hkv, T, 1])
    kq = rng.choice(FINITE_CODES, size=(Hkv, T, 128))
    ksc = (rng.uniform(0.5, 1.5, size=(Hkv, T)) * 2.0 ** -8).astype(np.float32)
    return q, w, kq, ksc, vq, vsc
