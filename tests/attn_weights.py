"""Power-of-two softmax weights for the attention kernels: inputs whose exact output says HOW each query weighted its keys.

tests/attn_needles.py makes every weight 0 or 1; here every key of a query gets a weight 2^k, different for the queries that
share a wave, a 16-row q-block or a GQA group, so the online-softmax bookkeeping (csrc/attn_prefill.hip: the lazy reference
m, alpha and its shuffle, the two denominator paths, the key-split merge; csrc/decode.hip and decode_common.hip.h: the
strict running maximum per wave, pal, the eight-wave merge, the split combine) is pinned to far below one bf16 ulp.

* Scale.  SCALE = float32(ln 2) * 2^-3: every entry point computes scale * 1.4426950408889634f in f32, which is exactly
  0.125 (tests/test_attn_weights.py asserts it in numpy float32).  A query is 8 e_d (or 8 (e_a + e_b)): the prefill kernels
  round q * 0.125 = 1 to bf16, the decode kernels multiply the f32 dot product by 0.125 - both exact.  Column d of K is then
  the score profile, in log2 units, of every query that looks in direction d: small integers, exact in bf16.
* Profiles.  A column holds at most A_MAX = 8 active keys with scores inside a window of 12, every other key of it is
  background at BG = -200 (weight 2^-188 relative: 0 in f32, the needle file's margin argument).  A causal row sees a
  prefix of its column; a prefix without an active key weights all its keys equally (a plain mean - still exact).  Keys
  no query of a column may see (past the context, the causal future of the column's last row, a segment without a row of
  the column, stale cache rows) score POISON_S = +200 in that column; rows no query at all may see carry V = POISON_V.
* V is attn_needles.v_rows: multiples of 1/8 in [-4, 4].  `reference` asserts, in integers, that
  sum_j 2^(s_j - s_min) |8 v_jd| < 2^24 over a query's keys of non-zero weight: every partial sum of numerator and
  denominator is then exact in f32 in any order and under any reference m, provided the exp2 of an integer is exact.
* Reference, float64 from the integer scores: w_j = ldexp(1, s_j - max), o = sum w v / sum w, a = sum w |v| / sum w.
* Slack, derived and never measured: rel(A) = (6 A + 16) * 2^-23 for a query with A keys of non-zero weight; the kernel may
  write any bf16 in [rne(o - rel a), rne(o + rel a)].  Numerator and denominator each get one f32 unit (2^-24) of exp2
  error per term, one per rescale that matters (at most A), one rounding per accumulation, and eight for the wave / split
  merges and the final 1 / l product: (3 A + 8) * 2^-24 each, relative to a.  Nobody has measured whether v_exp_f32 is
  exact on integer arguments; the slack does not assume it.  With A = 8 it is 2^-17 against a bf16 half-ulp of 2^-9.
* A case is valid only if at most AMBIGUOUS_CAP = 2 % of its outputs have lo != hi (tests/test_attn_weights.py, on the
  CPU, from the reference alone).  Observed shares (max over the cases of a family, CPU):
      prefill head_dim 128  1.42 %   prefill head_dim 80  0.76 %   decode self-attention  1.11 %
      decode cross-attention  0.46 %   draft rows  1.03 %

The float32 emulations at the end (lazy-reference tile loop; strict-max step loop with the eight-wave merge; split +
combine) exist for the discrimination checks: without a planted fault they must pass `check` on every case, with one they
must not.

CPU only: torch for bf16, numpy float64 / float32.  Never imports the library under test.
"""
import dataclasses
import functools

import numpy as np
import torch

import attn_needles as N

LN2_F32 = np.float32(0.6931471824645996)
SCALE = float(LN2_F32 * np.float32(0.125))
LOG2E_F32 = np.float32(1.4426950408889634)
QV = 8.0
BG = -200
POISON_S = 200
A_MAX = 8
WINDOW = 12
AMBIGUOUS_CAP = 0.02
MASKED = -(1 << 40)


def bf16r(x):
    """float64 numpy -> the nearest bf16 (through f32, as the kernels round), as float64."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def rel_slack(A):
    return (6.0 * A + 16.0) * 2.0 ** -23


# ----------------------------------------------------------------------------- profiles
def tiles(lo, hi, unit=64):
    """The absolute `unit`-key tiles that meet [lo, hi), clipped to it."""
    return [(max(lo, t), min(hi, t + unit)) for t in range(lo - lo % unit, hi, unit)]


def wave_slots(lo, hi, wave):
    """The 16-key steps of one wave of the streaming decode kernel (steps wave, wave + 8, ..), clipped to [lo, hi)."""
    s = [(max(lo, t), min(hi, t + 16)) for t in range(16 * wave, hi, 128)]
    return [x for x in s if x[0] < x[1]] or [(lo, hi)]


def _end(slot, i):
    return slot[0] if i % 2 == 0 else slot[1] - 1


def _steps(deltas, sign):
    def prof(slots):
        k = min(len(deltas) + 1, len(slots))
        used = deltas[len(deltas) - (k - 1):] if k > 1 else ()
        level = [0]
        for d in used:
            level.append(level[-1] + d)
        level = [x - level[-1] for x in level]             # rising: .., 0
        if sign < 0:
            level = level[::-1]                            # falling: 0, ..
        out = {}
        for i in range(k):
            out[_end(slots[i], i)] = level[i]
        for i in range(k):                                 # a lower companion at the other end of the tile
            key = _end(slots[i], i + 1)
            if key not in out and len(out) < A_MAX and level[i] - 2 >= -WINDOW:
                out[key] = level[i] - 2
        return out
    return prof


def _bg_first(slots):
    s = slots[-1]
    return {s[0]: 0, s[1] - 1: -1, (s[0] + s[1]) // 2: -5}


def _bg_first_early(slots):
    s = slots[min(1, len(slots) - 1)]
    return {s[0]: 0, s[1] - 1: -1, (s[0] + s[1]) // 2: -5}


def _max_first(slots, first=False):
    out = {slots[0][0] if first else slots[0][1] - 1: 0}
    for i, s in enumerate(slots[1:A_MAX]):
        out.setdefault(_end(s, i), -(1 + (i * 5) % WINDOW))
    return out


def _one_tile(slots, first=False):
    s = slots[0 if first else len(slots) // 2]
    n = min(A_MAX, s[1] - s[0])
    keys = sorted({s[0] + (i * (s[1] - s[0] - 1)) // max(n - 1, 1) for i in range(n)})
    return {k: -sc for k, sc in zip(keys, (0, 1, 2, 3, 4, 6, 9, 12))}


def _two_max(slots):
    out = {slots[0][0]: 0, slots[-1][1] - 1: 0}
    m = slots[len(slots) // 2]
    out.setdefault((m[0] + m[1]) // 2, -4)
    return out


def _edges(slots):
    inner = [s[0] for s in slots[1:]]
    pick = inner if len(inner) <= 4 else [inner[0], inner[1], inner[len(inner) // 2], inner[-1]]
    if 4096 in inner and 4096 not in pick:
        pick[2] = 4096
    out = {}
    for i, e in enumerate(pick):
        out[e - 1] = -(i % 2)
        out[e] = -((i + 1) % 2)
    return out or {slots[0][0]: 0}


def _app_max(slots):
    last = slots[-1][1] - 1
    out = {last: 0}
    out.setdefault(slots[0][0], -3)
    out.setdefault((slots[0][0] + last) // 2, -7)
    return out


def _app_min(slots):
    last = slots[-1][1] - 1
    out = {last: -WINDOW}
    out.setdefault(slots[0][0], 0)
    out.setdefault((slots[0][0] + last) // 2, -6)
    return out


PROFILES = {
    "rise1": _steps((1,), 1), "rise7": _steps((7,), 1), "rise8": _steps((8,), 1), "rise9": _steps((9,), 1),
    "rise12": _steps((12,), 1), "rise1_7": _steps((1, 7), 1), "rise8_1": _steps((8, 1), 1),
    "rise1x5": _steps((1, 1, 1, 1, 1), 1), "fall": _steps((3, 4, 5), -1), "fall8": _steps((8,), -1),
    "bg_first": _bg_first, "max_first": _max_first, "one_tile": _one_tile, "two_max": _two_max, "edges": _edges,
    "app_max": _app_max, "app_min": _app_min,
}
PREFILL_PROFILES = ("rise8", "rise9", "bg_first", "rise1", "edges", "rise7", "fall", "rise12", "two_max", "rise1_7",
                    "max_first", "one_tile", "rise8_1", "fall8", "rise1x5")
DECODE_PROFILES = PREFILL_PROFILES + ("app_max", "app_min")


def place(name, slots, causal=False):
    """{key: score} of profile `name` over the tile list `slots`.  A causal row below its column's first active key weights
    all its keys equally, and there should be few such rows: a causal column's bg_first peaks in its second tile, its one_tile
    is the first tile and its max_first starts at the first key."""
    if causal and name == "bg_first":
        out = _bg_first_early(slots)
    elif causal and name in ("one_tile", "max_first"):
        out = PROFILES[name](slots, first=True)
    else:
        out = PROFILES[name](slots)
    assert 1 <= len(out) <= A_MAX and max(out.values()) - min(out.values()) <= WINDOW, (name, out)
    assert all(slots[0][0] <= k < slots[-1][1] for k in out), (name, out, slots)
    return out


# ----------------------------------------------------------------------------- reference and check
@dataclasses.dataclass
class Unit:
    """The queries that share one K / V: s int64 [n, T] integer scores (MASKED where a query may not look), V float64 [T, D],
    labels [n] (case-specific: row, head, direction, profile, active keys with their 64-key tile)."""
    s: np.ndarray
    V: np.ndarray
    labels: list
    meta: dict = dataclasses.field(default_factory=dict)


def unit_from_tensors(q, k, v, valid, labels, **meta):
    """Unit from the tensors a kernel gets (q [n, D], k / v [T, D] bf16-valued, valid bool [n, T]): the scores must come out
    as integers after the exact 0.125."""
    s = (q.double() @ k.double().t()).numpy() * 0.125
    si = np.rint(s).astype(np.int64)
    assert np.array_equal(si.astype(np.float64), s), "scores are not integers"
    si = np.where(valid.numpy(), si, MASKED)
    return Unit(si, v.double().numpy(), list(labels), dict(meta))


def reference(u: Unit):
    """(o, a [n, D] float64, A [n]) of a unit; asserts the window / background structure and the f32 exactness bound."""
    s, V = u.s, u.V
    valid = s != MASKED
    assert valid.any(1).all(), "a query without a valid key"
    smax = np.where(valid, s, MASKED).max(1)
    rel = np.where(valid, s - smax[:, None], MASKED)
    act = rel >= -WINDOW
    assert (act | (rel <= -188)).all(), "a valid key is neither active nor background"
    w = np.where(act, np.ldexp(1.0, np.clip(rel, -WINDOW, 0).astype(np.int64)), 0.0)
    A = act.sum(1)
    # integers: sum_j 2^(s_j - s_min) |8 v_jd| < 2^24 over the keys of non-zero weight
    smin = np.where(act, rel, 0).min(1)
    wi = np.where(act, np.left_shift(1, np.clip(rel - smin[:, None], 0, WINDOW)), 0).astype(np.int64)
    seen = np.abs(V) * valid.any(0)[:, None]               # (rows no query may see are poison)
    v8 = np.rint(seen * 8).astype(np.int64)
    assert np.array_equal(v8 / 8.0, seen) and int(v8.max()) <= 32
    bound = wi @ v8
    assert int(bound.max()) < 1 << 24 and int(wi.sum(1).max()) < 1 << 24, "partial sums not exact in f32"
    den = w.sum(1, keepdims=True)
    return (w @ V) / den, (w @ np.abs(V)) / den, A


def interval(u: Unit):
    o, a, A = reference(u)
    e = rel_slack(A)[:, None] * a
    return bf16r(o - e), bf16r(o + e)


def ambiguous(units):
    """(elements with lo != hi, elements) over the units of a case."""
    amb = tot = 0
    for u in units:
        lo, hi = interval(u)
        amb += int((lo != hi).sum())
        tot += lo.size
    return amb, tot


def outside(u: Unit, got):
    lo, hi = interval(u)
    g = np.asarray(got, dtype=np.float64)
    return ~((lo <= g) & (g <= hi))


def check(u: Unit, got, what):
    """got [n, D]: every element inside [lo, hi], and |got| < 64 (no poison key, no NaN workspace)."""
    g = np.asarray(got, dtype=np.float64)
    lo, hi = interval(u)
    bad = ~((lo <= g) & (g <= hi))
    if bad.any():
        i, d = [int(x) for x in np.argwhere(bad)[0]]
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} outputs outside [lo, hi]; first: {u.labels[i]}, dim {d}: "
                             f"got {g[i, d]!r}, allowed [{lo[i, d]!r}, {hi[i, d]!r}]")
    m = np.abs(g).max()
    if not m < 64.0:
        raise AssertionError(f"{what}: |out| reaches {m} (a poison key or a NaN workspace reached a query)")


def _label(row, head, d, prof, col, lo, hi, unit=64):
    seen = {k: v for k, v in sorted(col.items()) if lo <= k < hi}
    return (f"query row {row} head {head} dir {d} profile {prof}, keys [{lo}, {hi}), actives key:score@tile "
            + " ".join(f"{k}:{v}@{k // unit}" for k, v in seen.items()))


# ----------------------------------------------------------------------------- prefill layout
@dataclasses.dataclass
class Prefill:
    name: str
    Q: torch.Tensor          # [Hq, S, D] bf16
    K: torch.Tensor          # [Hkv, T, D] bf16
    V: torch.Tensor          # [Hkv, T, D] bf16 (plain rows; the test transposes and reorders)
    units: list              # one per kv head: queries ordered (g, row)
    pos: list
    segments: list
    causal: bool
    mid: int = 0             # key-split cut (0: none)


def build_prefill(name, Hq, Hkv, D, segments, causal, P=0, T=None, pairs_every=0, seed=0, salt=0, mid=0):
    """Queries at positions P .. S - 1 of the segments [(lo, hi)] (S = the last hi), keys 0 .. S - 1 in a K of T >= S rows.
    Row i of Q, head h (g = h % G): direction dirs[(i % nd) * G + g]; nd >= 32 consecutive rows - more than a wave's - use
    different directions, so do the G heads that share a kv head.  pairs_every = n: every n-th row asks 8 (e_a + e_b) with a
    modifier column b (values in [-6, 0] on every key, no background of its own) and a column a whose window is 6."""
    G = Hq // Hkv
    S = segments[-1][1]
    T = T or S
    pos = list(range(P, S))
    alld = N.probe_dirs(D, D)
    nmod = 32 if pairs_every else 0
    nd = (D - nmod) // G
    nd = 96 if (G == 1 and nd >= 96) else nd
    assert nd >= 32
    seg_of = {}
    for si, (lo, hi) in enumerate(segments):
        for p in range(lo, hi):
            seg_of[p] = si
    K = torch.zeros((Hkv, T, D))
    V = torch.stack([N.v_rows(torch.arange(T), D, salt=salt * 16 + kv) for kv in range(Hkv)])
    if T > S:
        V[:, S:] = N.POISON_V
    Q = torch.zeros((Hq, len(pos), D))
    cols = {}                                               # (kv, c) -> (profile name, {key: score})
    rng = np.random.default_rng(seed)
    for kv in range(Hkv):
        for c in range(nd * G):
            rows = [p for i, p in enumerate(pos) if (i % nd) == c // G]
            d = alld[c]
            K[kv, :, d] = float(POISON_S)
            if not rows:
                continue
            prof = PREFILL_PROFILES[(c * 7 + kv * 3 + seed) % len(PREFILL_PROFILES)]
            col = {}
            for si, (lo, hi) in enumerate(segments):
                mine = [p for p in rows if seg_of[p] == si]
                if not mine:
                    continue                                # a segment without a row of this column stays poison
                end = max(mine) + 1 if causal else hi
                K[kv, lo:end, d] = float(BG)
                pname = PREFILL_PROFILES[(PREFILL_PROFILES.index(prof) + si) % len(PREFILL_PROFILES)]
                part = place(pname, tiles(lo, end), causal)
                if pairs_every:
                    part = {k: v // 2 for k, v in part.items()}
                col.update(part)
            for k, v in col.items():
                K[kv, k, d] = float(v)
            cols[(kv, c)] = (prof, col)
        for m in range(nmod):                               # modifier columns
            K[kv, :, alld[nd * G + m]] = torch.from_numpy(-rng.integers(0, 7, T).astype(np.float32))
    labels = [[] for _ in range(Hkv)]
    valid = torch.zeros((len(pos), T), dtype=torch.bool)
    for i, p in enumerate(pos):
        lo, hi = segments[seg_of[p]]
        hi = p + 1 if causal else hi
        valid[i, lo:hi] = True
    for h in range(Hq):
        kv, g = h // G, h % G
        for i, p in enumerate(pos):
            c = (i % nd) * G + g
            Q[h, i, alld[c]] = QV
            two = pairs_every and i % pairs_every == 0
            if two:
                Q[h, i, alld[nd * G + (i // pairs_every) % nmod]] = QV
            lo, hi = segments[seg_of[p]]
            labels[kv].append(_label(p, h, alld[c], cols[(kv, c)][0] + ("+modifier" if two else ""), cols[(kv, c)][1],
                                     lo, p + 1 if causal else hi))
    Qb, Kb, Vb = Q.to(torch.bfloat16), K.to(torch.bfloat16), V.to(torch.bfloat16)
    assert torch.equal(Kb.float(), K) and torch.equal(Vb.float(), V)
    units = []
    for kv in range(Hkv):
        q = Q[kv * G:(kv + 1) * G].reshape(G * len(pos), D)
        units.append(unit_from_tensors(q, K[kv], V[kv], valid.repeat(G, 1), labels[kv], k0=[segments[seg_of[p]][0] for p in pos] * G,
                                       rows=len(pos), mid=mid))
    return Prefill(name, Qb, Kb, Vb, units, pos, list(segments), causal, mid)


def prefill_got(case: Prefill, out, kv):
    """out [S, Hq * D] (a kernel's output, any float tensor on the CPU) -> [G * S, D] in the unit's order (g, row)."""
    Hq, S, D = case.Q.shape
    G = Hq // case.K.shape[0]
    o = out.double().reshape(S, Hq, D).permute(1, 0, 2)
    return o[kv * G:(kv + 1) * G].reshape(G * S, D).numpy()


# ----------------------------------------------------------------------------- decode / cross layout
@dataclasses.dataclass
class Decode:
    name: str
    K: torch.Tensor          # [B, Hkv, T, D] bf16 cache (rows >= ctx - 1 poison when a key is appended)
    V: torch.Tensor
    q: torch.Tensor          # [B, Hq, D] f32: 8 e_d
    knew: torch.Tensor       # [B, Hkv, D] (zeros for cross-attention)
    vnew: torch.Tensor
    ctxs: list
    units: list              # [b * Hkv + kv]: G queries over ctx keys
    Hq: int
    Hkv: int

    @property
    def qkv(self):
        B = self.q.shape[0]
        return torch.cat((self.q, self.knew, self.vnew), 1).reshape(B, -1).to(torch.bfloat16)


def decode_slots(n, h):
    """Tile list of head h over keys [0, n): one wave's 16-key steps of the streaming form (heads 0, 2, ..: a rising column
    moves that wave's running maximum, and the steps sit in different 64-key splits), or the 64-key splits (odd heads)."""
    return wave_slots(0, n, (h // 2) % 8) if h % 2 == 0 else tiles(0, n, 64)


def build_decode(name, Hq, Hkv, T, ctxs, append=True, own_from=0, seed=0, D=128):
    """Caches of B = len(ctxs) sequences.  append: key ctx - 1 comes from the projection row (knew / vnew) and the cache rows
    from ctx - 1 on are poison (the stale rows of a longer request); else (cross-attention) rows from ctx on are.
    own_from = P: sequences b > 0 place their actives at keys >= P (share_prefix then gives them sequence 0's first P rows)."""
    B, G = len(ctxs), Hq // Hkv
    dirs = N.probe_dirs(G, D)
    K = torch.zeros((B, Hkv, T, D))
    V = torch.zeros((B, Hkv, T, D))
    knew, vnew = torch.zeros((B, Hkv, D)), torch.zeros((B, Hkv, D))
    q = torch.zeros((B, Hq, D))
    units = []
    for b, n in enumerate(ctxs):
        for kv in range(Hkv):
            Kf = torch.zeros((n, D))
            Vf = N.v_rows(torch.arange(n), D, salt=seed * 64 + b * Hkv + kv)
            labels = []
            for g in range(G):
                h = kv * G + g
                prof = DECODE_PROFILES[(h * 5 + b * 3 + seed) % len(DECODE_PROFILES)]
                slots = tiles(own_from, n, 64) if (own_from and b > 0) else decode_slots(n, h)
                col = place(prof, slots)
                Kf[:, dirs[g]] = float(BG)
                for k, v in col.items():
                    Kf[k, dirs[g]] = float(v)
                labels.append(_label(f"seq {b}", h, dirs[g], prof, col, 0, n))
                q[b, h, dirs[g]] = QV
            units.append(unit_from_tensors(q[b, kv * G:(kv + 1) * G], Kf, Vf, torch.ones((G, n), dtype=torch.bool), labels, ctx=n))
            last = n - 1 if append else n
            K[b, kv, :last], V[b, kv, :last] = Kf[:last], Vf[:last]
            K[b, kv, last:, dirs] = float(POISON_S)
            V[b, kv, last:] = N.POISON_V
            if append:
                knew[b, kv], vnew[b, kv] = Kf[n - 1], Vf[n - 1]
    return Decode(name, K.to(torch.bfloat16), V.to(torch.bfloat16), q, knew, vnew, list(ctxs), units, Hq, Hkv)


def share_prefix(case: Decode, P, poison_copies=False):
    """Keys [0, P) of every sequence b > 0 become sequence 0's rows (copied into b's cache, or - poison_copies, the forked
    form, which must read the parent's - left as poison there); the units are rebuilt from the tensors."""
    G = case.Hq // case.Hkv
    dirs = N.probe_dirs(G, case.K.shape[-1])
    K, V = case.K.clone(), case.V.clone()
    units = []
    for b, n in enumerate(case.ctxs):
        assert b == 0 or n > P
        for kv in range(case.Hkv):
            Kf, Vf = case.K[b, kv, :n].float().clone(), case.V[b, kv, :n].float().clone()
            Kf[n - 1], Vf[n - 1] = case.knew[b, kv], case.vnew[b, kv]
            if b > 0:
                Kf[:P], Vf[:P] = case.K[0, kv, :P].float(), case.V[0, kv, :P].float()
                if poison_copies:
                    K[b, kv, :P] = 0.0
                    K[b, kv, :P, dirs] = float(POISON_S)
                    V[b, kv, :P] = N.POISON_V
                else:
                    K[b, kv, :P], V[b, kv, :P] = case.K[0, kv, :P], case.V[0, kv, :P]
            old = case.units[b * case.Hkv + kv]
            units.append(unit_from_tensors(case.q[b, kv * G:(kv + 1) * G], Kf, Vf, torch.ones((G, n), dtype=torch.bool),
                                           old.labels, ctx=n))
    return dataclasses.replace(case, K=K, V=V, units=units)


def decode_got(case: Decode, out, b, kv):
    G = case.Hq // case.Hkv
    return out.double().reshape(len(case.ctxs), case.Hq, -1)[b, kv * G:(kv + 1) * G].numpy()


@dataclasses.dataclass
class Draft:
    K: torch.Tensor          # [Hkv, T, D] bf16: rows >= step poison
    V: torch.Tensor
    qkv: torch.Tensor        # [R, (Hq + 2 Hkv) * D] bf16
    knew: torch.Tensor       # [R, Hkv, D]
    vnew: torch.Tensor
    units: list              # [r * Hkv + kv]
    step: int


def build_draft(Hq, Hkv, T, step, R, D=128, seed=0):
    """R rows of one sequence at positions step .. step + R - 1.  Row r, head g looks in its own direction dirs[r G + g]; its
    column holds actives in the cache, at every row 0 .. r - 1 the same launch appends and at its own row; the rows after it
    are its causal future: poison in its direction."""
    G = Hq // Hkv
    dirs = N.probe_dirs(R * G, D)
    n_all = step + R
    K = torch.zeros((Hkv, T, D))
    V = torch.zeros((Hkv, T, D))
    q = torch.zeros((R, Hq, D))
    Kf = torch.zeros((Hkv, n_all, D))
    Vf = torch.stack([N.v_rows(torch.arange(n_all), D, salt=seed * 64 + 40 + kv) for kv in range(Hkv)])
    labels = {}
    for kv in range(Hkv):
        for r in range(R):
            for g in range(G):
                d = dirs[r * G + g]
                h = kv * G + g
                col = {(h * 7) % step: -2 - (h % 3), step - 1: -5 + (g % 4)}
                for rr in range(r + 1):
                    col[step + rr] = -((rr + r + g) % 4) if rr < r else (0 if (g + r) % 2 == 0 else -WINDOW + 2)
                Kf[kv, :, d] = float(BG)
                Kf[kv, step + r + 1:, d] = float(POISON_S)
                for k, v in col.items():
                    Kf[kv, k, d] = float(v)
                q[r, h, d] = QV
                labels[(r, kv, g)] = _label(f"draft row {r}", h, d, "draft", col, 0, step + r + 1)
    units = []
    for r in range(R):
        for kv in range(Hkv):
            n = step + r + 1
            units.append(unit_from_tensors(q[r, kv * G:(kv + 1) * G], Kf[kv, :n], Vf[kv, :n], torch.ones((G, n), dtype=torch.bool),
                                           [labels[(r, kv, g)] for g in range(G)], ctx=n))
    K[:, :step], V[:, :step] = Kf[:, :step], Vf[:, :step]
    K[:, step:, :] = 0.0
    K[:, step:, dirs] = float(POISON_S)
    V[:, step:] = N.POISON_V
    knew, vnew = Kf[:, step:].permute(1, 0, 2).contiguous(), Vf[:, step:].permute(1, 0, 2).contiguous()
    qkv = torch.cat((q, knew, vnew), 1).reshape(R, -1).to(torch.bfloat16)
    return Draft(K.to(torch.bfloat16), V.to(torch.bfloat16), qkv, knew, vnew, units, step)


# ----------------------------------------------------------------------------- the GPU cases (built once, on the CPU)
PREFILL_S = (65, 130, 321)
PREFILL_HEADS = ((4, 1), (2, 2))
DECODE_HEADS = ((28, 4), (8, 2), (2, 1))
DECODE_CTXS = (1, 17, 64, 65, 200, 512)
D80_SEGMENTS = ((0, 64), (64, 256), (256, 320))
SPLIT_S, SPLIT_MID = 2945, 1472     # the smallest S whose 3-head ViT plan splits keys, and its cut (the GPU test reads the plan)


@functools.lru_cache(maxsize=None)
def prefill128(S, causal, Hq, Hkv, P=0, T=None, salt=0):
    pairs = 4 if (not causal and (Hq, Hkv) == (2, 2) and S == 130) else 0
    return build_prefill(f"prefill128 S {S} causal {causal} heads {Hq}/{Hkv} P {P} salt {salt}", Hq, Hkv, 128, [(0, S)], causal,
                         P=P, T=T, pairs_every=pairs, seed=S + 2 * causal + Hq + salt, salt=salt)


@functools.lru_cache(maxsize=None)
def prefill80(causal=False):
    segs = [(0, 320)] if causal else list(D80_SEGMENTS)
    return build_prefill(f"prefill80 S 320 causal {causal}", 3, 3, 80, segs, causal, seed=5 + causal)


@functools.lru_cache(maxsize=None)
def prefill80_split(S, mid):
    return build_prefill(f"prefill80 key-split S {S}", 3, 3, 80, [(0, S)], False, seed=9, mid=mid)


@functools.lru_cache(maxsize=None)
def decode_case(Hq, Hkv, T, ctxs, append=True, own_from=0, seed=0):
    return build_decode(f"decode heads {Hq}/{Hkv} T {T} ctxs {ctxs} append {append} own_from {own_from}", Hq, Hkv, T, list(ctxs),
                        append=append, own_from=own_from, seed=seed)


SHARED_P = 64
SHARED_CTXS = (65,) + tuple((66, 81, 129, 200, 512)[i % 5] for i in range(31))


@functools.lru_cache(maxsize=None)
def shared_case(poison_copies=False):
    return share_prefix(decode_case(28, 4, 512, SHARED_CTXS, own_from=SHARED_P, seed=1), SHARED_P, poison_copies)


@functools.lru_cache(maxsize=None)
def draft_case():
    return build_draft(8, 2, 512, 62, 4)


def cpu_cases():
    """(family, name, units, emulation kind) of every case the GPU file runs that can be built without the library."""
    out = []
    for S in PREFILL_S:
        for causal in (True, False):
            for Hq, Hkv in PREFILL_HEADS:
                c = prefill128(S, causal, Hq, Hkv)
                out.append(("prefill128", c.name, c.units, "lazy"))
    c = prefill128(130, True, 4, 1, P=65)
    out.append(("prefill128", c.name, c.units, "lazy"))
    c = prefill128(130, True, 2, 2, P=65)
    out.append(("prefill128", c.name, c.units, "lazy"))
    for j in range(3):
        for causal in (True, False):
            c = prefill128(130, causal, 4, 1, T=192, salt=j + 1)
            out.append(("prefill128", c.name, c.units, "lazy"))
    for causal in (False, True):
        c = prefill80(causal)
        out.append(("prefill80", c.name, c.units, "lazy_f32sum" if causal else "lazy"))
    c = prefill80_split(SPLIT_S, SPLIT_MID)
    out.append(("prefill80", c.name, c.units, "lazy"))
    for Hq, Hkv in DECODE_HEADS:
        c = decode_case(Hq, Hkv, 512, DECODE_CTXS)
        out.append(("decode", c.name, c.units, "decode"))
    c = decode_case(8, 2, 4608, (4161,))
    out.append(("decode", c.name, c.units, "decode"))
    c = decode_case(32, 8, 448, (1, 63, 64, 65, 200, 448), append=False, seed=3)
    out.append(("cross", c.name, c.units, "decode"))
    c = shared_case()
    out.append(("decode", c.name + " shared", c.units, "decode"))
    out.append(("draft", "draft R 4 step 62", draft_case().units, "decode"))
    return out


# ----------------------------------------------------------------------------- float32 emulations (discrimination checks)
F32 = np.float32
NEG = F32(-1.0e30)
LAZY = F32(8.0)


def _exp2(x):
    """float32 exp2 of (near-)integers: exact powers of two, 0 below the f32 range."""
    x = np.asarray(x, dtype=F32)
    xi = np.rint(np.clip(x, -200.0, 200.0))
    frac = (np.clip(x, -200.0, 200.0) - xi).astype(np.float64)
    r = np.ldexp(np.exp2(frac), xi.astype(np.int64))
    r = np.where(x < -149.0, 0.0, r)
    with np.errstate(over="ignore"):
        return r.astype(F32)


def _bf16_f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16).to(torch.float32).numpy()


LAZY_FAULTS = ("alpha_neighbour", "o_not_l", "l_not_o", "ge8_clamp", "never_move", "p_ulp", "bg_weight")
DECODE_FAULTS = ("combine_xor1", "pal_next_head", "bg_weight")


def _scores_f32(u, fault):
    s = np.where(u.s == MASKED, NEG, u.s.astype(F32)).astype(F32)
    if fault == "bg_weight":                                # background keys weigh 2^-12 relative to the row's maximum
        smax = s.max(1, keepdims=True)
        s = np.where((s > NEG) & (s < smax - 100), smax - 12, s).astype(F32)
    return s


def _lazy_range(s, V, k_lo, k_hi, kt0, fault, f32sum):
    """The tile loop of csrc/attn_prefill.hip over keys [k_lo, k_hi) on the absolute 64-key grid from kt0: (O, l, m)."""
    n, D = s.shape[0], V.shape[1]
    O, l, negm = np.zeros((n, D), F32), np.zeros(n, F32), np.zeros(n, F32)
    for t, kt in enumerate(range(kt0, k_hi, 64)):
        a, b = max(kt, k_lo), min(kt + 64, k_hi)
        sc = (s[:, a:b] + negm[:, None]).astype(F32)
        sc = np.where(s[:, a:b] <= NEG, NEG, sc)
        mx = sc.max(1)
        if fault == "never_move":
            move = np.full(n, t == 0)
        else:
            move = (mx > LAZY) | (t == 0)
        delta = np.where(move, mx, F32(0)).astype(F32)
        negm = (negm - delta).astype(F32)
        sc = (sc - delta[:, None]).astype(F32)
        alpha = _exp2(np.minimum(-delta, F32(0)))           # (tile 0 may move m down: the factor is clamped to 1)
        ao = alpha[np.minimum(np.arange(n) ^ 1, n - 1)] if fault == "alpha_neighbour" else alpha
        with np.errstate(over="ignore", invalid="ignore"):
            if fault != "l_not_o":
                O = (O * ao[:, None]).astype(F32)
            if fault != "o_not_l":
                l = (l * alpha).astype(F32)
            p = _exp2(sc)
            if fault == "ge8_clamp":                        # the tile counts as moved at mx >= 8, delta is still the > 8 one, and a
                hit = (mx >= LAZY) & ~move                  # moved tile's p is taken to be <= 1
                p = np.where(hit[:, None], np.minimum(p, F32(1)), p)
            pb = _bf16_f32(p)
            pn = pb
            if fault == "p_ulp":                            # numerator: every second key's p one bf16 ulp up; denominator: raw p
                pn = pb.copy()
                pn[:, ::2] = pb[:, ::2] * F32(1 + 2.0 ** -7)
            O = (O + pn.astype(np.float64) @ V[a:b]).astype(F32)
            l = (l + (p if (f32sum or fault == "p_ulp") else pb).astype(np.float64).sum(1)).astype(F32)
    return O, l, -negm


def emulate_lazy(u: Unit, fault=None, f32sum=False):
    """Prefill kernels: rows grouped by their work item's first key (the absolute tile grid starts at k0 & ~63); `mid` cuts the
    keys in two halves merged as attn_vit32_kernel does."""
    s = _scores_f32(u, fault)
    n, T = s.shape
    out = np.zeros((n, u.V.shape[1]), np.float64)
    k0s = np.asarray(u.meta["k0"])
    mid = u.meta.get("mid", 0)
    for k0 in np.unique(k0s):
        idx = np.nonzero(k0s == k0)[0]
        valid = u.s[idx] != MASKED
        k_hi = int(np.nonzero(valid.any(0))[0].max()) + 1
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if mid:
                O1, l1, m1 = _lazy_range(s[idx], u.V, int(k0), mid, int(k0) & ~63, fault, f32sum)
                O2, l2, m2 = _lazy_range(s[idx], u.V, mid, k_hi, mid, fault, f32sum)
                m = np.maximum(m1, m2)
                a1, a2 = _exp2(m1 - m), _exp2(m2 - m)
                O = ((a1[:, None] * O1).astype(F32) + (a2[:, None] * O2).astype(F32)).astype(F32)
                l = ((a1 * l1).astype(F32) + (a2 * l2).astype(F32)).astype(F32)
            else:
                O, l, _ = _lazy_range(s[idx], u.V, int(k0), k_hi, int(k0) & ~63, fault, f32sum)
            inv = np.where(l > 0, F32(1) / l, F32(0)).astype(F32)
            out[idx] = _bf16_f32((O * inv[:, None]).astype(F32))
    return out


def emulate_stream(u: Unit, fault=None):
    """decode_attn_stream_kernel: eight waves, wave w walks the 16-key steps w, w + 8, .. with a strict running maximum per head,
    bf16-rounded p in numerator and denominator, pal[wave][g] rescales; merged with exp2f(m_w - M)."""
    s = _scores_f32(u, fault)
    G, n = s.shape
    D = u.V.shape[1]
    Ow, lw, mw = np.zeros((8, G, D), F32), np.zeros((8, G), F32), np.full((8, G), NEG, F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for w in range(8):
            for k0 in range(16 * w, n, 128):
                sc = s[:, k0:min(k0 + 16, n)]
                m_new = np.maximum(mw[w], sc.max(1))
                al = _exp2(mw[w] - m_new)
                mw[w] = m_new
                pb = _bf16_f32(_exp2(sc - m_new[:, None]))
                lw[w] = (lw[w] * al + pb.sum(1)).astype(F32)
                if (al != 1).any():
                    ag = np.roll(al, -1) if fault == "pal_next_head" else al
                    Ow[w] = (Ow[w] * ag[:, None]).astype(F32)
                Ow[w] = (Ow[w] + pb.astype(np.float64) @ u.V[k0:k0 + sc.shape[1]]).astype(F32)
        M = mw.max(0)
        wt = _exp2(mw - M[None])
        o = (wt[:, :, None] * Ow).sum(0).astype(F32)
        l = (wt * lw).sum(0).astype(F32)
        return _bf16_f32(np.where(l[:, None] > 0, o / l[:, None], F32(0)))


def emulate_split(u: Unit, fault=None):
    """decode_attn_split_body + decode_attn_combine_body: 64-key splits with their own maximum and unrounded f32 p, merged with
    exp2f(m_s - M)."""
    s = _scores_f32(u, fault)
    G, n = s.shape
    ns = (n + 63) // 64
    D = u.V.shape[1]
    Os, ls, ms = np.zeros((ns, G, D), F32), np.zeros((ns, G), F32), np.zeros((ns, G), F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(ns):
            sc = s[:, 64 * j:min(64 * j + 64, n)]
            ms[j] = sc.max(1)
            e = _exp2(sc - ms[j][:, None])
            ls[j] = e.sum(1)
            Os[j] = (e.astype(np.float64) @ u.V[64 * j:64 * j + sc.shape[1]]).astype(F32)
        M = ms.max(0)
        wt = _exp2(ms - M[None])
        if fault == "combine_xor1":
            wt = wt[[min(j ^ 1, ns - 1) for j in range(ns)]]
        o = (wt[:, :, None] * Os).sum(0).astype(F32)
        l = (wt * ls).sum(0).astype(F32)
        return _bf16_f32(np.where(l[:, None] > 0, o / l[:, None], F32(0)))
