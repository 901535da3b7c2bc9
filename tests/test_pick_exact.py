"""CPU checks of the pick reference alone (tests/pick_exact.py): the hash against values worked out by hand, the range and
the mean of u, the ambiguity caps on every entry of every GPU case table, the integer emulation on the exact-weight rows
and the agreement with sampling.nucleus_ref."""
import math

import numpy as np
import pytest

import pick_exact as P
from vision_inspection_system_amd.sampling import nucleus_ref


def test_slack_is_within_the_issue_bounds():
    # the derivation of the module docstring, term by term
    inner = P.E_LOG * 2.0 ** -23 * (1 + 2.0 ** -20)        # the inner log's relative error, as it moves log e
    outer = max(P.E_LOG * 2.0 ** -23, 2.0 ** -19)           # per unit of M: 4 ulp of g, or the fast form's 1 ulp of 24
    rounding = 2.0 ** -22                                   # product and sum
    assert inner + outer + rounding + 2.0 ** -41 < 2.0 ** -18 <= P.S_DERIVED / 2
    assert P.S_DERIVED <= P.S <= 2.0 ** -10
    assert -math.log(1 - 2.0 ** -24) >= 2.0 ** -24 and -math.log(2.0 ** -24) < 17


# (seed, step, i): z after the three xors, after the increment, after each multiply round, after the last shift-xor; k = z >> 41.
# Worked out with plain integers mod 2^64:  z0 = (seed << 32) ^ (step * 0x9E3779B97F4A7C15) ^ i;  z1 = z0 + 0x9E3779B97F4A7C15;
# z2 = (z1 ^ (z1 >> 30)) * 0xBF58476D1CE4E5B9;  z3 = (z2 ^ (z2 >> 27)) * 0x94D049BB133111EB;  z4 = z3 ^ (z3 >> 31).
HAND = [
    ((0, 0, 0), (0x0, 0x9E3779B97F4A7C15, 0x6F68261B57E7A770, 0xE220A838BF5C9DDE, 0xE220A8397B1DCDAF), 0x711054),
    ((1, 0, 0), (0x100000000, 0x9E3779BA7F4A7C15, 0x10DCCE0DB2A26C1C, 0xC42C5A1B2BDAB50E, 0xC42C5A1AA3820138), 0x62162D),
    ((0, 1, 0), (0x9E3779B97F4A7C15, 0x3C6EF372FE94F82A, 0x2A94FCBFCCB43499, 0x6E789E6A7D485920, 0x6E789E6AA1B965F4), 0x373C4F),
    ((0xFFFFFFFF, 0x7FFFFFFF, 152063), (0xDE923BAE00B7D214, 0x7CC9B56780024E29, 0x9E8D5796A7BB3A3F, 0x0316E65476A60AB9,
                                        0x0316E654708BC611), 0x18B73),
]


@pytest.mark.parametrize("args,zs,k", HAND)
def test_hash_by_hand(args, zs, k):
    seed, step, i = args
    M = (1 << 64) - 1
    z0, z1, z2, z3, z4 = zs
    assert z0 == ((seed << 32) ^ ((step * 0x9E3779B97F4A7C15) & M) ^ i)
    assert z1 == (z0 + 0x9E3779B97F4A7C15) & M
    assert z2 == ((z1 ^ (z1 >> 30)) * 0xBF58476D1CE4E5B9) & M
    assert z3 == ((z2 ^ (z2 >> 27)) * 0x94D049BB133111EB) & M
    assert z4 == z3 ^ (z3 >> 31)
    assert k == z4 >> 41
    assert int(P.noise_k(seed, step, i)[0]) == k
    assert float(P.noise_u(seed, step, i)[0]) == (k + 0.5) / 2 ** 23
    assert float(P.noise(seed, step, i)[0]) == -math.log(-math.log((k + 0.5) / 2 ** 23))


def test_u_stays_inside_the_unit_interval_and_is_centred():
    u = P.noise_u(12345, 7, np.arange(1 << 20))
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24
    assert float(np.float32(u.max())) == u.max() and float(np.float32(u.min())) == u.min()      # exact in f32
    assert abs(u.mean() - 0.5) <= 4 * math.sqrt(1 / 12 / u.size)
    # the extremes of k, whatever the hash: u never reaches 0 or 1, and -log(-log u) stays finite
    for k in (0, 2 ** 23 - 1):
        uk = (k + 0.5) / 2 ** 23
        assert 0 < uk < 1 and float(np.float32(uk)) == uk and math.isfinite(-math.log(-math.log(uk)))


def test_candidates_rules():
    x = np.array([1.0, 3.0, np.nan, 3.0, -np.inf], dtype=np.float32)
    assert P.candidates(x, 0.0, 0, 0, np.arange(5)).tolist() == [1]
    assert P.candidates(x, 0.0, 0, 0, np.array([0, 2, 4])).tolist() == [0]
    assert P.candidates(x, 0.0, 0, 0, np.array([2])).tolist() == [0]                 # NaN only: id 0
    assert P.candidates(x, 1.0, 0, 0, np.array([], dtype=np.int64)).tolist() == [0]  # nothing allowed: id 0
    ninf = np.full(9, -np.inf, dtype=np.float32)
    assert P.candidates(ninf, 1.0, 3, 4, np.arange(2, 9)).tolist() == [2]            # equal infinities: the lowest id
    far = np.array([0.0, 50.0, 0.0], dtype=np.float32)
    assert P.candidates(far, 1.0, 3, 4, np.arange(3)).tolist() == [1]
    same = np.zeros(1 << 16, dtype=np.float32)                                       # a constant row: the largest noise wins
    g = P.noise(9, 2, np.arange(same.size))
    assert P.candidates(same, 1.0, 9, 2, np.arange(same.size)).tolist()[0] == int(np.argmax(g)) or \
        int(np.argmax(g)) in P.candidates(same, 1.0, 9, 2, np.arange(same.size)).tolist()


def _shares(cases):
    worst, amb, tot = 0.0, 0, 0
    for c in cases:
        flat = [x for step in c.expected for x in step]
        a = sum(len(x) > 1 for x in flat)
        assert a / len(flat) <= P.AMBIGUOUS_CAP, (c.name, a, len(flat))
        assert c.ambiguous_share() == a / len(flat)
        worst, amb, tot = max(worst, a / len(flat)), amb + a, tot + len(flat)
    return worst, amb / tot, tot


@pytest.mark.parametrize("table", ["argmax", "argmax masked", "gemv", "gemv masked", "sample"])
def test_ambiguity_cap(table, capsys):
    if table.startswith("argmax"):
        cases = [c for V in P.VS_ARGMAX + (152064,) for c in P.argmax_cases(V, table.endswith("masked"))]
    elif table.startswith("gemv"):
        cases = [c for N in P.NS_GEMV for c in P.gemv_cases(N, table.endswith("masked"))]
    else:
        cases = [c for V in P.VS_SAMPLE + (152064,) for c in P.sample_cases(V)]
    worst, overall, tot = _shares(cases)
    with capsys.disabled():
        print(f"\n  {table}: {len(cases)} entries, {tot} draws, ambiguous: worst entry {100 * worst:.2f} %, overall {100 * overall:.2f} %")
    if table == "sample":
        rows = sum(c.B for c in cases)
        wide = sum(c.wide_rows() for c in cases)
        with capsys.disabled():
            print(f"  sample: {rows} rows, n_lo != n_hi on {100 * wide / rows:.2f} %")
        assert wide <= 0.01 * rows


def test_tables_cover_what_they_claim():
    a = [c for V in P.VS_ARGMAX + (152064,) for c in P.argmax_cases(V)]
    assert {c.B for c in a} == {1, 3, 64} and {c.T for c in a} == set(P.TS_ARGMAX) and {c.start for c in a} == set(P.STARTS)
    assert {c.seed for c in a} == set(P.SEEDS) and {c.pad for c in a} == {False, True}
    assert {k for c in a for k in c.kinds} == set(P.ARGMAX_KINDS)
    for B in (1, 3, 64):
        assert {c.T for c in a if c.B == B} == set(P.TS_ARGMAX)
    m = [c for V in P.VS_ARGMAX + (152064,) for c in P.argmax_cases(V, True)]
    assert {k for c in m for k in c.mask_kinds} == set(P.MASK_KINDS)
    assert any(c.V % 64 and int(c.words[b][-1]) >> (c.V % 64) for c in m for b in range(c.B))     # live bits past V
    g = [c for N in P.NS_GEMV for c in P.gemv_cases(N)]
    assert P.gemv_grid(8192) == 1024 and P.gemv_grid(8193) == 1024 and P.gemv_grid(8256) == 1025   # the blocks > 1024 rule
    assert P.gemv_grid(73728) == 2048 and P.gemv_grid(73729) == 2048 and P.gemv_grid(152064) == 2048
    hows = set()
    for c in g:
        if c.tie:
            assert c.logits[c.tie[0]] == c.logits[c.tie[1]] == c.logits.max()
            oa, ob = P.gemv_owner(c.N, c.tie[0]), P.gemv_owner(c.N, c.tie[1])
            hows.add("pair" if c.tie[0] // 2 == c.tie[1] // 2 else "wave" if oa[0] == ob[0] else "wg")
    assert hows == {"pair", "wave", "wg"}
    gm = [c for N in P.NS_GEMV for c in P.gemv_cases(N, True)]
    assert any(c.mask_kind == "only_last" and c.N % 2 == 1 and c.N > 1 for c in gm)              # the odd last row alone
    s = [c for V in P.VS_SAMPLE + (152064,) for c in P.sample_cases(V)]
    assert {c.p for c in s} == set(P.PS_SAMPLE) and {c.T for c in s} == set(P.TS_SAMPLE) and {c.B for c in s} >= {1, 64}
    assert {k for c in s for k in c.kinds} == set(P.SAMPLE_KINDS)
    groups = {int(nu.order.size) for c in s for b, nu in enumerate(c.nucleus) if c.kinds[b] == "const" and not nu.open}
    assert any(n < 1024 for n in groups) and 1024 in groups and any(n > 1024 for n in groups)   # LDS cut, its limit, bisection


def _integer_cut(row, inv_temp, p, allow):
    """The kernel's cut on a row whose weights are 2^40 (at the maximum) or 0: Z, target, the first prefix reaching it."""
    ids = np.arange(row.size) if allow is None else np.flatnonzero(allow)
    ids = ids[~np.isnan(row[ids])]
    if ids.size == 0:
        return 0
    m = row[ids].max()
    if p >= 1.0 or m == -np.inf:
        return int(ids.size)
    n_top = int((row[ids] == m).sum())
    Z = n_top << 40
    target = max(1, min(Z, math.ceil(float(np.float32(p)) * float(Z))))
    return -(-target // (1 << 40))


def test_exact_rows_cut_in_integers():
    seen = 0
    for V in P.VS_SAMPLE:
        for c in P.sample_cases(V):
            for b, nu in enumerate(c.nucleus):
                if c.kinds[b] not in ("const", "two_exact"):
                    continue
                assert nu.exact and nu.n_lo == nu.n_hi, (c.name, b)
                assert nu.n_lo == _integer_cut(c.logits[b], c.inv_temp, c.p, c.allow(b)), (c.name, b)
                seen += 1
    assert seen > 300


def test_nkeep_of_nucleus_ref_is_admissible():
    """nucleus_ref(...).nkeep lies in [n_lo, n_hi] on every table row of nucleus_ref's domain (it has no rule for NaN logits
    and none for a row with nothing allowed but NaN)."""
    seen = 0
    for V in P.VS_SAMPLE + (152064,):
        for c in P.sample_cases(V):
            for b, nu in enumerate(c.nucleus):
                if np.isnan(c.logits[b]).any():
                    continue
                ref = nucleus_ref(c.logits[b], c.T, float(np.float32(c.p)), c.allow(b))
                want = ref.nkeep if ref.order.size else 0
                if c.p >= 1.0 and c.words is not None:
                    want = int(ref.order.size)           # nucleus_ref counts V at top_p = 1, masked or not; the kernel counts |A|
                assert nu.n_lo <= want <= nu.n_hi, (c.name, b, c.kinds[b], want, nu.n_lo, nu.n_hi)
                assert (nu.order == ref.order).all()
                seen += 1
    assert seen > 2000
