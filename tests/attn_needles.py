"""Needle inputs for the attention coverage tests: inputs whose exact output says which keys each probe query attended.

A probe query is a basis direction e_d.  A needle is a key C * e_d: its score is more than 150 log2 units above every other
key's, so in f32 every other weight underflows to 0 and every needle weight is exactly 1.  Background keys and non-probe
queries are zero in every probe direction (their scores against needles and probes are exactly 0).  V rows are multiples of
1/8 in [-4, 4], distinct per (key, salt): one needle returns its V row, two or four equal needles their exact mean (a multiple
of 1/32 in [-4, 4], exact in bf16).  Every key a probe must not see - past the context, past nkeys, the future of a causal
row, another segment - is a poison key: C in the probe's direction and V = POISON_V, so reading it moves the output by
thousands.
"""
import math

import torch

C_NEEDLE = 1536.0           # bf16-exact; score C * 128**-0.5 * log2(e) = 195.9 log2 units (head_dim 80: 247.7)
POISON_V = 4096.0
LOG2E = 1.4426950408889634


def log2_margin(c: float, q: float, scale: float) -> float:
    """Score of a needle c * e_d against a probe q * e_d in log2 units (the kernels' softmax domain), background at 0."""
    return c * q * scale * LOG2E


def probe_dirs(n: int, D: int):
    """n distinct directions < D, spread over the head (not only the first dims)."""
    if n > D:
        raise ValueError("more probes than dimensions")
    step = next(s for s in (37, 29, 23, 19, 17, 13, 11, 7, 3, 1) if math.gcd(s, D) == 1)
    return [(5 + step * i) % D for i in range(n)]


def v_rows(keys: torch.Tensor, D: int, salt: int = 0) -> torch.Tensor:
    """V rows [len(keys), D] for key indices `keys`: multiples of 1/8 in [-4, 4], a hash of (key, dim, salt)."""
    k = keys.to(torch.int64)[:, None]
    d = torch.arange(D, dtype=torch.int64, device=keys.device)[None, :]
    h = (k * 1000003 + d * 7919 + (salt + 1) * 104729) & 0x7FFFFFFF
    h = ((h ^ (h >> 13)) * 1274126177) & 0x7FFFFFFF
    h = h ^ (h >> 16)
    return ((h % 65) - 32).to(torch.float32) / 8.0


def background(shape, gen: torch.Generator, dirs, scale: float = 0.25) -> torch.Tensor:
    """Small random values (bf16-exact) that are zero in every probe direction."""
    x = (torch.randn(shape, generator=gen, device=gen.device) * scale).to(torch.bfloat16).float()
    x[..., list(dirs)] = 0.0
    return x


def build_keys(T: int, D: int, dirs, needles, poison, gen: torch.Generator, salt: int = 0):
    """K, V [T, D] f32 (bf16-exact) for one kv head.

    needles: {dir: iterable of key rows}; poison: {dir: iterable of key rows} (keys that dir's probes must not see).
    A poison row that is nobody's needle gets V = POISON_V; a row that is one probe's needle and another's poison keeps
    its needle V (reading it still moves that other probe's output far off its exact value)."""
    K = background((T, D), gen, dirs)
    V = v_rows(torch.arange(T, device=gen.device), D, salt)
    is_needle = torch.zeros(T, dtype=torch.bool, device=gen.device)
    for d, rows in needles.items():
        rows = torch.as_tensor(sorted(set(rows)), dtype=torch.int64, device=gen.device)
        K[rows, d] = C_NEEDLE
        is_needle[rows] = True
    for d, rows in poison.items():
        rows = torch.as_tensor(sorted(set(rows)), dtype=torch.int64, device=gen.device)
        if rows.numel():
            K[rows, d] = C_NEEDLE
            pv = rows[~is_needle[rows]]
            V[pv] = POISON_V
    return K, V


def probe_query(D: int, d: int, value: float = 1.0) -> torch.Tensor:
    q = torch.zeros(D)
    q[d] = value
    return q


def attn_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, valid: torch.Tensor, scale: float) -> torch.Tensor:
    """float64 softmax(q k^T scale) v over exactly the valid keys: q [n, D], k / v [T, D], valid [n, T] bool -> [n, D]."""
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.t()) * scale
    s = s.masked_fill(~valid, float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at |x| (8 significant bits); the smallest normal's ulp at 0."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def assert_within_ulp(got: torch.Tensor, ref: torch.Tensor, what: str, ulps: float = 1.0) -> None:
    g, r = got.double().cpu(), ref.double().cpu()
    bad = ~((g - r).abs() <= ulps * bf16_ulp(r))
    if bad.any():
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside {ulps} bf16 ulp; first at {idx}: "
                             f"got {g[tuple(idx)].item()} ref {r[tuple(idx)].item()}")


def assert_no_poison(got: torch.Tensor, what: str) -> None:
    m = float(got.float().abs().max())
    if not m < 64.0:
        raise AssertionError(f"{what}: |out| reaches {m} (a poison key, or a NaN workspace, reached a probe)")


def rope_bf16(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Rotate-half rope of bf16 x [.., D] with f32 tables, rounded to bf16 once (the decode kernels' q / k staging)."""
    h = x.shape[-1] // 2
    a, b = x[..., :h].double(), x[..., h:].double()
    c0, c1, s0, s1 = cos[..., :h].double(), cos[..., h:].double(), sin[..., :h].double(), sin[..., h:].double()
    return torch.cat((a * c0 - b * s0, b * c1 + a * s1), -1).to(torch.bfloat16).float()


def qnorm_bf16(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """Cross-attention q-norm as the decode kernels stage it: bf16(bf16(x * rstd) * w) per 128-dim head (x [.., D])."""
    xd = x.double()
    rstd = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    return ((xd * rstd).to(torch.bfloat16).double() * w.double()).to(torch.bfloat16).float()


def needle_groups(n: int, edges):
    """Needle sets for one probe over keys [0, n): single needles at the first key, the last key and either side of every
    edge in `edges` that lies inside, then pairs / fours of equal needles spread over the range."""
    singles = {0, n - 1}
    for b in edges:
        for p in (b - 1, b):
            if 0 <= p < n:
                singles.add(p)
    groups = [(p,) for p in sorted(singles)]
    if n >= 2:
        groups.append((0, n - 1))
    four = tuple(sorted({0, n // 3, (2 * n) // 3, n - 1}))
    if len(four) == 4:
        groups.append(four)
    return groups
