"""Inputs and float64 references for the token pick: vis_argmax_f32, vis_argmax_masked_f32, vis_gemv_bf16_argmax(_masked)
(csrc/decode.hip) and vis_sample_f32 (csrc/sampling.hip).

Every sampled pick is  argmax_i  fl(fl(v_i * inv_temp) + gumbel_noise(seed, step, i))  with ties to the lower id, and
gumbel_noise (csrc/decode_common.hip.h) is a counter hash, so the token a given (seed, step, row) must produce is a
function of the inputs.  `noise_u` is that hash in exact uint64 arithmetic; u = (k + 0.5) / 2^23 with k < 2^23 is exact in
f32 and in float64.  The two logarithms are not emulated bit for bit: `perturbed` returns, per id, the interval [lo, hi] a
correct kernel's value lies in, `candidates` the ids whose hi reaches the largest lo.  A draw with ONE candidate is
decisive and the kernel must produce it; an ambiguous draw passes when the pick is among its candidates.

The slack S.  half-width = S * max(1, |v * inv_temp|, |g|),  g = -log(-log u).  S is a bound, not a measurement:

* The library is built without fast-math, and <llvm>/lib/clang/<ver>/include/__clang_hip_math.h then maps BOTH logf and
  __logf to __builtin_logf (line "float __logf(float __x) { return __builtin_logf(__x); }"; logf goes through
  __FAST_OR_SLOW, which picks the same builtin unless the approximate-functions macro is set), i.e. to OCML's log_f32.  That
  header and the HIP headers beside it carry no ulp table; the figures below are the OpenCL full-profile limits the OCML
  functions are written to meet (log <= 3 ulp, exp <= 3 ulp) with one ulp of headroom: E_LOG = E_EXP = 4 ulp, 1 ulp <= 2^-23
  relative.  The outer log is bounded as if it WERE the fast instruction form (v_log_f32, 1 ulp on log2, times ln 2), so the
  bound holds under either mapping.
* inner:  e = -logf(u), relative error <= 4 * 2^-23 = 2^-21;  e lies in [-log(1 - 2^-24), -log(2^-24)] = [2^-24, 16.64].
* outer:  g = -log e.  The inner error moves log e by <= 2^-21 (1 + 2^-20).  A full-precision outer log adds <= 4 ulp of g,
  i.e. <= 2^-21 |g|; the fast form adds 1 ulp of |log2 e| <= 24, ulp(24) = 2^-19, times ln 2 and one product rounding:
  < 2^-19.  With M = max(1, |v t|, |g|):  |g - g_exact| <= 2^-21 (1 + 2^-20) + max(2^-21 M, 2^-19) <= (2^-21 + 2^-19) M + 2^-41.
* the product v * inv_temp and the sum each round once (relative 2^-24; one rounding in all when they contract to an fma):
  <= 2^-24 |v t| + 2^-24 (|v t| + |g| + 2^-18) <= 2^-22 M.
* total <= (2^-21 + 2^-19 + 2^-22) M + 2^-41 = 11 * 2^-22 M + 2^-41 < 2^-18 M.  S_DERIVED = 2^-17 doubles that and S = 2^-14
  leaves another factor 8; every honest bug (a wrong id, step or seed, 24 bits instead of 23, a missing 0.5) moves a value
  by O(1).

The nucleus cut.  `nucleus_interval` keeps the order of sampling.nucleus_ref (logit desc, id asc over the allowed ids; NaN
logits weigh nothing, are never kept and are left out of the order - nucleus_ref itself is undefined on rows with NaN) and
bounds the kernel's fixed-point weight q_i = rintf(expf(-d_i) * 2^40), d_i = fl(fl(m - l_i) * t):  two f32 roundings move d
by <= d 2^-23, expf adds E_EXP ulp, the product with 2^40 is exact and rintf adds <= 1/2:
    q_i in [w_i 2^40 (1 - R_i) - 1/2, w_i 2^40 (1 + R_i) + 1/2],   R_i = 1.01 (1.01 d_i + E_EXP) 2^-23,
with two exact cases: d_i = 0 gives expf(-0) = 1, q_i = 2^40; an upper bound below 1/2 gives q_i = 0.  The kernel keeps the
shortest prefix with  c_n >= ceil(double(p) * double(Z));  c_n is an integer, so that is  c_n (1 - p') >= p' (Z - c_n)  with
p' = p (1 + delta), |delta| <= 2^-53 (2^-50 used) - a form whose two sides are bounded separately by the prefix and the
tail sums.  n_lo is the first n at which the inequality CAN hold, n_hi the first at which it MUST.  Rows whose weights are
all exact (constant rows; rows holding only m and m - 40 / t) are cut in integers exactly as the kernel does (Z,
target = ceil(double(float32(p)) * Z), the first prefix reaching it), so n_lo == n_hi there.

Case tables are built with seeded numpy generators.  A table entry is valid only if at most AMBIGUOUS_CAP = 1 % of its
draws are ambiguous, and at most 1 % of a nucleus table's rows may have n_lo != n_hi; these are conditions on the INPUTS,
met from the reference alone: an entry whose first inputs miss the cap is rebuilt from the next generator seed (`_resolve`;
tests/test_pick_exact.py asserts the caps on what the tables finally hold).  Observed (CPU, shares of the worst entry /
of all draws):
    argmax 0.39 % / 0.07 %   argmax masked 0.20 % / 0.03 %   gemv 0.00 % / 0.00 %   gemv masked 0.00 % / 0.00 %
    sample draws 0.00 % / 0.00 %   sample rows with n_lo != n_hi 0.00 %

CPU only: numpy and float64, never the library under test.
"""
import dataclasses
import functools
import math

import numpy as np

GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
SEQ_SEED_STRIDE = 0x9E3779B9       # vis_argmax_f32: row b draws with seed + SEQ_SEED_STRIDE * b (mod 2^32)
NO_ID = 0x7FFFFFFF                 # the kernels' "nothing found" index, and i* of an open cut record
E_LOG = 4
E_EXP = 4
S_DERIVED = 2.0 ** -17
S = 2.0 ** -14
AMBIGUOUS_CAP = 0.01
T_TOK = 8                          # token slots per row: steps >= T_TOK store no token
STEPS = 8
STARTS = (0, 5, 2 ** 31 - 9)
SEEDS = (0, 0xFFFFFFFF, 0xC0000000)   # the last two wrap when SEQ_SEED_STRIDE * row is added

assert S_DERIVED <= S <= 2.0 ** -10


# ----------------------------------------------------------------------------- the hash
def noise_k(seed, step, ids):
    """The 23 random bits of gumbel_noise(seed, step, i) for every i of ids (uint64 arithmetic, wrapping as the kernel's)."""
    i = np.atleast_1d(np.asarray(ids)).astype(np.uint64)
    c = ((int(seed) & 0xFFFFFFFF) << 32) ^ (((int(step) & 0xFFFFFFFF) * GOLD) & M64)
    z = (i ^ np.uint64(c)) + np.uint64(GOLD)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(41)


def noise_u(seed, step, ids):
    return (noise_k(seed, step, ids).astype(np.float64) + 0.5) / 8388608.0


def noise(seed, step, ids):
    return -np.log(-np.log(noise_u(seed, step, ids)))


def perturbed(logits, inv_temp, seed, step, ids):
    """(lo, hi) float64 per id: the interval of fl(fl(v * inv_temp) + gumbel_noise(seed, step, id)).  Infinite logits give
    lo = hi = +-inf, NaN logits NaN."""
    ids = np.atleast_1d(np.asarray(ids, dtype=np.int64))
    x = np.asarray(logits, dtype=np.float32)[ids].astype(np.float64) * float(np.float32(inv_temp))
    g = noise(seed, step, ids)
    c = x + g
    with np.errstate(invalid="ignore"):
        h = S * np.maximum(1.0, np.maximum(np.abs(x), np.abs(g)))
    h = np.where(np.isfinite(x), h, 0.0)
    return c - h, c + h


def candidates(logits, inv_temp, seed, step, ids):
    """The ids (ascending) a correct kernel may pick among `ids` (ascending).  Nothing to pick from (no id, or NaN only):
    id 0.  inv_temp = 0: the lowest id among the exact maxima.  Equal infinite values tie exactly: the lowest id."""
    ids = np.atleast_1d(np.asarray(ids, dtype=np.int64))
    zero = np.zeros(1, dtype=np.int64)
    if ids.size == 0:
        return zero
    if float(np.float32(inv_temp)) == 0.0:
        lo = hi = np.asarray(logits, dtype=np.float32)[ids].astype(np.float64)
        exact = True
    else:
        lo, hi = perturbed(logits, inv_temp, seed, step, ids)
        exact = False
    ok = ~np.isnan(lo)
    if not ok.any():
        return zero
    top = lo[ok].max()
    if exact or np.isinf(top):
        return ids[ok & (hi == top)][:1]
    return ids[ok & (hi >= top)]


# ----------------------------------------------------------------------------- the nucleus cut
@dataclasses.dataclass
class Nucleus:
    n_lo: int              # admissible nkeep, lowest
    n_hi: int              # ... and highest
    order: np.ndarray      # the allowed, non-NaN ids by (logit desc, id asc)
    open: bool             # K = A: the cut record is (-inf, NO_ID) and the pick runs over the whole order
    exact: bool            # every weight exact: n_lo == n_hi from the integer emulation


def nucleus_interval(logits, inv_temp, top_p, allow=None):
    l = np.asarray(logits, dtype=np.float32).reshape(-1)
    V = l.size
    ids = np.arange(V) if allow is None else np.flatnonzero(np.asarray(allow, dtype=bool).reshape(-1)[:V])
    v = l[ids].astype(np.float64)
    ids, v = ids[~np.isnan(v)], v[~np.isnan(v)]
    order = ids[np.lexsort((ids, -v))]
    n = int(order.size)
    t, p = float(np.float32(inv_temp)), float(np.float32(top_p))
    if n == 0:
        return Nucleus(0, 0, order, True, True)
    if t == 0.0:
        return Nucleus(1, 1, order, True, True)
    vo = l[order].astype(np.float64)
    m = vo[0]
    assert m < np.inf, "a +inf logit has no weight (m - l = NaN): outside the tables"
    if p >= 1.0 or m == -np.inf:
        return Nucleus(n, n, order, True, True)
    d = (m - vo) * t
    w = np.exp(-d)
    R = 1.01 * (1.01 * np.where(np.isfinite(d), d, 0.0) + E_EXP) * 2.0 ** -23
    vhi = w * 2.0 ** 40 * (1 + R)
    vlo = w * 2.0 ** 40 * (1 - R)
    one, none = d == 0, vhi < 0.5
    if (one | none).all():
        q = np.where(one, 1 << 40, 0).astype(np.int64)
        c = np.cumsum(q)
        Z = int(c[-1])
        target = max(1, min(Z, math.ceil(p * float(Z))))
        nk = int(np.searchsorted(c, target, side="left")) + 1
        return Nucleus(nk, nk, order, False, True)
    qlo = np.where(one, 2.0 ** 40, np.where(none, 0.0, np.maximum(0.0, vlo - 0.5)))
    qhi = np.where(one, 2.0 ** 40, np.where(none, 0.0, vhi + 0.5))
    clo, chi = np.cumsum(qlo), np.cumsum(qhi)
    tlo, thi = np.maximum(0.0, clo[-1] - clo), np.maximum(0.0, chi[-1] - chi)
    thi[-1] = 0.0
    p_lo, p_hi, eps = p * (1 - 2.0 ** -50), p * (1 + 2.0 ** -50), 1e-12
    sure = clo * (1 - p_hi) >= p_hi * thi * (1 + eps)
    poss = chi * (1 - p_lo) * (1 + eps) >= p_lo * tlo
    return Nucleus(int(np.argmax(poss)) + 1, int(np.argmax(sure)) + 1, order, False, False)


# ----------------------------------------------------------------------------- masks
MASK_KINDS = ("rand10", "only_last", "lastword", "alt_words", "empty")


def mask_words(kind, V, rng):
    """One allow row, uint64 [ceil(V / 64)].  "lastword" and "alt_words" leave LIVE bits past V in the last word."""
    nw = (V + 63) // 64
    bits = np.zeros(nw * 64, dtype=bool)
    if kind == "rand10":
        bits[:V] = rng.random(V) < 0.1
    elif kind == "only_last":
        bits[V - 1] = True
    elif kind == "lastword":
        bits[:V] = rng.random(V) < 0.5
        bits[V:] = True
    elif kind == "alt_words":
        bits.reshape(nw, 64)[(nw - 1) % 2::2] = True       # the last word is an allowed one, bits past V included
    elif kind == "ones":
        bits[:V] = True
    else:
        assert kind == "empty"
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8").astype(np.uint64)


def allowed_ids(words, V):
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:V]
    return np.flatnonzero(bits)


# ----------------------------------------------------------------------------- logit rows
def _two_ids(V, how):
    """Two ids for a planted tie.  Stage 1 gives id i to workgroup (i / 256) mod min(256, ceil(V / 256)), wave (i mod 256) / 64.
    "wg": different workgroups (the last id; at V > 65536 that is workgroup 0's SECOND grid-stride trip against its first);
    "wave": two waves of workgroup 0.  Short rows take what there is."""
    a = min(3, V - 1)
    b = V - 1 if how == "wg" else min(130, V - 1)
    return a, b


ARGMAX_KINDS = ("gauss1", "gauss8", "tie_wg", "tie_wave", "const", "shaped", "neginf", "nan")


def logit_row(kind, V, rng):
    if kind == "gauss1":
        return rng.normal(0, 1, V).astype(np.float32)
    if kind == "gauss8":
        return (rng.normal(0, 1, V) * 8).astype(np.float32)
    if kind in ("tie_wg", "tie_wave"):
        r = rng.normal(0, 1, V).astype(np.float32)
        top = np.float32(r.max() + 1)
        for i in _two_ids(V, kind[4:]):
            r[i] = top
        return r
    if kind == "const":
        return np.full(V, 1.5, dtype=np.float32)
    if kind == "shaped":       # what vis_shape_f32's copy looks like under top_k = 50: -inf below the 50th value
        r = (rng.normal(0, 1, V) * 3).astype(np.float32)
        if V > 50:
            r[r < np.sort(r)[-50]] = -np.inf
        return r
    if kind == "neginf":
        return np.full(V, -np.inf, dtype=np.float32)
    assert kind == "nan"
    return np.full(V, np.nan, dtype=np.float32)


def _resolve(build, what):
    """The first of build(0), build(1), ... that meets the caps (see the module docstring)."""
    for attempt in range(32):
        case = build(attempt)
        if case.ambiguous_share() <= AMBIGUOUS_CAP and case.valid():
            return case
    raise AssertionError(f"{what}: no inputs within the ambiguity cap")


def _share(cands):
    flat = [c for step in cands for c in step]
    return sum(len(c) > 1 for c in flat) / max(1, len(flat))


# ----------------------------------------------------------------------------- (a), (b): vis_argmax_f32 and its masked form
@dataclasses.dataclass(eq=False)
class ArgmaxCase:
    name: str
    V: int
    B: int
    T: float
    start: int
    seed: int
    pad: bool                  # ld_logits = V + 5 with +inf in the padding
    logits: np.ndarray         # [B, V] f32
    kinds: tuple
    words: np.ndarray = None   # [B, ceil(V / 64)] uint64, masked table only
    mask_kinds: tuple = ()

    @property
    def inv_temp(self):        # as hip.py forms it: a double quotient, narrowed to f32 on the way into the library
        return float(np.float32(1.0 / self.T)) if self.T > 0 else 0.0

    @functools.cached_property
    def expected(self):
        """[STEPS][B] candidate arrays."""
        out = []
        ids = [np.arange(self.V) if self.words is None else allowed_ids(self.words[b], self.V) for b in range(self.B)]
        for s in range(STEPS):
            out.append([candidates(self.logits[b], self.inv_temp, (self.seed + SEQ_SEED_STRIDE * b) & 0xFFFFFFFF,
                                   self.start + s, ids[b]) for b in range(self.B)])
        return out

    def ambiguous_share(self):
        return _share(self.expected)

    def valid(self):
        return True


BATCHES = (64, 1, 3)
VS_ARGMAX = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 65536, 65537)
TS_ARGMAX = (0.0, 0.1, 0.7, 1.0, 2.0)


def _argmax_case(V, B, T, start, seed, pad, off, masked, tag):
    def build(attempt):
        rng = np.random.default_rng([7, V, B, int(T * 10), int(masked), attempt])
        kinds = tuple(ARGMAX_KINDS[(off + attempt + r) % len(ARGMAX_KINDS)] for r in range(B))
        logits = np.stack([logit_row(k, V, rng) for k in kinds])
        words, mk = None, ()
        if masked:
            mk = tuple(MASK_KINDS[(off + r // 2) % len(MASK_KINDS)] for r in range(B))
            words = np.stack([mask_words(k, V, rng) for k in mk])
        return ArgmaxCase(f"{tag}-V{V}-B{B}-T{T}-s{start}", V, B, T, start, SEEDS[(seed + attempt) % 3], pad, logits, kinds,
                          words, mk)
    return _resolve(build, f"{tag} V={V} T={T}")


@functools.lru_cache(maxsize=None)
def argmax_cases(V, masked=False):
    """The entries of one vocabulary size: every temperature, B / start / seed / padding / row kinds rotating."""
    tag = "masked" if masked else "argmax"
    if V == 152064:
        return (_argmax_case(V, 3, 0.7, 0, 2, True, 0, masked, tag),)
    vi = VS_ARGMAX.index(V)
    out = []
    for ti, T in enumerate(TS_ARGMAX):
        B = BATCHES[(vi + ti) % 3]
        if V >= 65536 and B == 64 and not (V == 65537 and T == 0.7):
            B = 3                                     # one 64-row entry at the large sizes: the reference costs B * V * STEPS
        out.append(_argmax_case(V, B, T, STARTS[(vi + 2 * ti) % 3], 2 * vi + ti, (vi + ti) % 2 == 1, 3 * vi + ti, masked, tag))
    return tuple(out)


# ----------------------------------------------------------------------------- (c): vis_gemv_bf16_argmax and its masked form
GEMV_K = 64
GEMV_STEPS = 4
NS_GEMV = (1, 2, 7, 513, 8191, 8193, 73729, 152064)


def gemv_grid(N):
    """Workgroups of vis_gemv_bf16_argmax at N rows (the grid rule of gemv_bf16_launch)."""
    blocks = ((N + 1) // 2 + 3) // 4
    if blocks > 1024:
        blocks = 1024 + (blocks - 1024) // 8
    return min(blocks, 2048)


def gemv_owner(N, row):
    """(workgroup, wave) that computes `row`: wave w of the 4 * blocks waves owns pairs [n_pairs w / n_waves, n_pairs (w + 1) / n_waves)."""
    n_pairs, n_waves = (N + 1) // 2, 4 * gemv_grid(N)
    begins = (n_pairs * np.arange(n_waves + 1, dtype=np.int64)) // n_waves
    w = int(np.searchsorted(begins, row // 2, side="right")) - 1
    return w // 4, w % 4


def _gemv_tie_rows(N, how):
    """Two rows for a planted exact tie: in one row pair, in two waves of one workgroup, in two workgroups (a launch of one
    workgroup has only the first two)."""
    if N < 2:
        return None
    if how == "pair" or N < 4:
        a = 2 * ((N // 2 - 1) // 2)
        return a, a + 1
    a = 10 if N > 64 else 0
    oa = gemv_owner(N, a)
    if how == "wave":
        for r in range(a + 2, min(N, a + 64), 2):
            o = gemv_owner(N, r)
            if o[0] == oa[0] and o[1] != oa[1]:
                return a, min(r + 1, N - 1)
    return a, N - 1


@dataclasses.dataclass(eq=False)
class GemvCase:
    name: str
    N: int
    T: float
    start: int
    seed: int
    x: np.ndarray              # [K] f32 holding +-1 (exact in bf16)
    W: np.ndarray              # [N, K] f32 holding bf16 values
    norm_w: np.ndarray         # [K] f32 holding bf16 values, or None
    logits: np.ndarray         # [N] f32: W x' EXACTLY (every term a multiple of 2^-10, every partial sum < 2^14)
    tie: tuple
    words: np.ndarray = None
    mask_kind: str = ""

    inv_temp = ArgmaxCase.inv_temp

    @functools.cached_property
    def expected(self):
        return self.expected_for(self.logits)

    def expected_for(self, logits):
        """[GEMV_STEPS][1] candidates from the f32 logits the launch wrote (the test reads them back)."""
        ids = np.arange(self.N) if self.words is None else allowed_ids(self.words, self.N)
        return [[candidates(logits, self.inv_temp, self.seed, self.start + s, ids)] for s in range(GEMV_STEPS)]

    def ambiguous_share(self):
        return _share(self.expected)

    def valid(self):
        return True


def _gemv_case(N, norm, T, start, seed, tie_how, mask_kind, ci):
    def build(attempt):
        rng = np.random.default_rng([11, N, int(norm), int(T * 10), ci, attempt])
        K = GEMV_K
        x = rng.choice([-1.0, 1.0], K).astype(np.float32)
        x[:3] = 1.0
        # rmsnorm of a +-1 row: rstd = rsqrt(1 + eps) rounds x * rstd back to +-1 in bf16, so x' = x * norm_w exactly
        nw = rng.choice([0.5, 1.0, 2.0], K).astype(np.float32) if norm else None
        if norm:
            nw[:3] = 1.0
        xe = x * nw if norm else x
        W = np.empty((N, K), dtype=np.float32)
        W[:, 3:] = rng.integers(-4, 5, K - 3).astype(np.float32) / 4          # the same for every row: a common offset
        val = rng.permutation(N)                                              # distinct logits: val * 2^-10 + offset
        W[:, 0] = (val & 255) * 2.0 ** -10
        W[:, 1] = ((val >> 8) & 255) * 2.0 ** -2
        W[:, 2] = (val >> 16) * 2.0 ** 6
        tie = _gemv_tie_rows(N, tie_how) if tie_how else None
        if tie:
            top = int(np.argmax(val))
            W[[tie[0], top]] = W[[top, tie[0]]]
            W[tie[1]] = W[tie[0]]                                             # identical weight rows: an exact tie at the top
        logits = (W.astype(np.float64) @ xe.astype(np.float64)).astype(np.float32)
        assert (logits.astype(np.float64) == W.astype(np.float64) @ xe.astype(np.float64)).all()
        assert np.unique(logits).size == N - (1 if tie else 0)
        words = mask_words(mask_kind, N, rng) if mask_kind else None
        return GemvCase(f"gemv-N{N}-norm{int(norm)}-T{T}-{tie_how}-{mask_kind}", N, T, start, SEEDS[(seed + attempt) % 3], x,
                        W, nw, logits, tie, words, mask_kind)
    return _resolve(build, f"gemv N={N}")


GEMV_MASKS = MASK_KINDS + ("ones",)       # "only_last" at the odd sizes allows the odd last row N - 1 alone


@functools.lru_cache(maxsize=None)
def gemv_cases(N, masked=False):
    ni = NS_GEMV.index(N)
    out = []
    for ci, (norm, T) in enumerate(((False, 0.0), (True, 0.7), (False, 0.7), (True, 0.0))):
        tie = ("pair", "wave", "wg", "")[(ni + ci) % 4] if T > 0 else ("pair", "wave", "wg")[(ni + ci) % 3]
        mk = GEMV_MASKS[(ni + ci) % len(GEMV_MASKS)] if masked else ""
        if masked and T == 0.0 and ci == 0:
            mk = "ones"                                # the planted tie decides this one: both of its rows allowed
        out.append(_gemv_case(N, norm, T, STARTS[(ni + ci) % 3], ni + ci, tie, mk, ci))
    return tuple(out)


# ----------------------------------------------------------------------------- (d): vis_sample_f32
SAMPLE_KINDS = ("const", "two_exact", "two_level", "straddle", "gauss1", "gauss8", "shaped", "nan_some")
VS_SAMPLE = (1, 2, 64, 65, 1023, 1024, 1025, 2049, 4097, 65537)
PS_SAMPLE = (0.0, 2.0 ** -24, 0.1, 0.5, 0.9, 1 - 2.0 ** -24, 1.0)
TS_SAMPLE = (0.1, 0.7, 2.0)


def sample_row(kind, V, T, rng):
    if kind == "const":                    # tie group = the whole allowed set: < 1024 LDS cut, > 1024 bisection
        return np.full(V, 1.5, dtype=np.float32)
    if kind == "two_exact":                # weights exactly 2^40 (at m) or exactly 0 (40 / t below it)
        r = np.full(V, np.float32(2.0) - np.float32(40.0) * np.float32(T), dtype=np.float32)
        r[rng.choice(V, V // 2 + 1, replace=False)] = 2.0
        return r
    if kind == "two_level":                # five ids at m, everything else T / 2 below: the cut falls inside the lower group
        r = np.full(V, np.float32(1.0) - np.float32(0.5) * np.float32(T), dtype=np.float32)
        r[rng.choice(V, min(5, V), replace=False)] = 1.0
        return r
    if kind == "straddle":                 # a tie group holding 40 % of the ids near the top of a Gaussian row
        r = rng.normal(0, 1, V).astype(np.float32)
        r[rng.choice(V, max(1, (2 * V) // 5), replace=False)] = 3.0
        r[rng.integers(V)] = 4.0
        return r
    if kind == "nan_some":                 # NaN and -inf entries weigh nothing
        r = (rng.normal(0, 1, V) * 2).astype(np.float32)
        if V > 2:
            r[rng.random(V) < 0.1] = np.nan
            r[rng.random(V) < 0.1] = -np.inf
            r[rng.integers(V)] = 5.0
        return r
    return logit_row(kind, V, rng)


@dataclasses.dataclass(eq=False)
class SampleCase:
    name: str
    V: int
    B: int
    T: float
    p: float
    pad: bool
    logits: np.ndarray         # [B, V]
    kinds: tuple
    seeds: np.ndarray          # [B] uint32
    steps: np.ndarray          # [B] int32
    words: np.ndarray = None
    mask_kinds: tuple = ()

    inv_temp = ArgmaxCase.inv_temp

    def allow(self, b):
        if self.words is None:
            return None
        a = np.zeros(self.V, dtype=bool)
        a[allowed_ids(self.words[b], self.V)] = True
        return a

    @functools.cached_property
    def nucleus(self):
        return [nucleus_interval(self.logits[b], self.inv_temp, self.p, self.allow(b)) for b in range(self.B)]

    def pick_candidates(self, b, nkeep):
        """Candidates of row b's Gumbel-max over the first nkeep ids of the order (the whole order under an open cut)."""
        nu = self.nucleus[b]
        ids = np.sort(nu.order if nu.open else nu.order[:nkeep])
        return candidates(self.logits[b], self.inv_temp, int(self.seeds[b]), int(self.steps[b]), ids)

    @functools.cached_property
    def expected(self):
        return [[self.pick_candidates(b, self.nucleus[b].n_lo) for b in range(self.B)]]

    def ambiguous_share(self):
        return _share(self.expected)

    def wide_rows(self):
        return sum(nu.n_lo != nu.n_hi for nu in self.nucleus)

    def valid(self):
        return self.wide_rows() == 0


def _sample_case(V, B, T, p, start, pad, off, masked):
    def build(attempt):
        rng = np.random.default_rng([13, V, B, int(T * 10), int(p * 2 ** 24), int(masked), attempt])
        words, mk = None, ()
        if masked:
            mk = tuple(MASK_KINDS[(off + r // len(SAMPLE_KINDS)) % len(MASK_KINDS)] for r in range(B))
            words = np.stack([mask_words(k, V, rng) for k in mk])
        inv_temp = float(np.float32(1.0 / T))
        kinds, rows, nus = [], [], []
        for r in range(B):
            # a row whose cut the interval cannot decide (a cut deep in the tail, where the weights are a few units of 2^-40)
            # is drawn again, then replaced by a two-level row: the cap on n_lo != n_hi is a condition on the inputs
            kind = SAMPLE_KINDS[(off + attempt + r) % len(SAMPLE_KINDS)]
            allow = None if words is None else np.isin(np.arange(V), allowed_ids(words[r], V))
            for sub in range(5):
                row = sample_row(kind if sub < 4 else "two_level", V, T, rng)
                nu = nucleus_interval(row, inv_temp, p, allow)
                if nu.n_lo == nu.n_hi:
                    break
            kinds.append(kind if sub < 4 else "two_level")
            rows.append(row)
            nus.append(nu)
        logits = np.stack(rows)
        seeds = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
        seeds[0] = SEEDS[(off + attempt) % 3]
        if B > 1:
            seeds[1] = SEEDS[(off + attempt + 1) % 3]
        steps = (start + np.arange(B) % 5).astype(np.int64).astype(np.int32)
        case = SampleCase(f"sample-V{V}-B{B}-T{T}-p{p!r}-m{int(masked)}", V, B, T, p, pad, logits, tuple(kinds), seeds, steps,
                          words, mk)
        case.__dict__["nucleus"] = nus
        return case
    return _resolve(build, f"sample V={V} p={p}")


@functools.lru_cache(maxsize=None)
def sample_cases(V):
    """Every top_p at one vocabulary size; T, B, masked / unmasked, start and padding rotate."""
    if V == 152064:
        return (_sample_case(V, 8, 0.7, 0.9, 0, True, 0, False),)
    vi = VS_SAMPLE.index(V)
    out = []
    for pi, p in enumerate(PS_SAMPLE):
        B = 64 if (pi + vi) % 2 == 0 else 1
        out.append(_sample_case(V, B, TS_SAMPLE[(pi + vi) % 3], p, STARTS[(pi + 2 * vi) % 3], (pi + vi) % 4 == 0, 3 * pi + vi,
                                (pi + vi // 2) % 2 == 1))
    # one more 64-row launch at the next temperature, so that every row kind meets p = 1/2 at every size
    out.append(_sample_case(V, 64, TS_SAMPLE[(vi + 1) % 3], 0.5, 5, False, vi, vi % 2 == 0))
    return tuple(out)
