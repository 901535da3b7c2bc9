"""CPU checks of the needle construction behind tests/test_attn_coverage_gpu.py: margins, the float64 reference, exactness."""
import itertools

import torch

import attn_needles as N


def test_needle_margin_exceeds_150_log2_units():
    """Every probe the GPU file builds: q = e_d (self-attention, head_dim 128 and 80) or the q-norm of e_d with weights in
    [0.5, 1.5] (cross-attention); the needle's score sits > 150 log2 units above a background score of exactly 0, so every
    other f32 weight exp2(-margin) underflows to 0."""
    assert N.log2_margin(N.C_NEEDLE, 1.0, 128 ** -0.5) > 150
    assert N.log2_margin(N.C_NEEDLE, 1.0, 80 ** -0.5) > 150
    qn = N.qnorm_bf16(N.probe_query(128, 7)[None], torch.full((128,), 0.5), 1e-5)
    assert N.log2_margin(N.C_NEEDLE, float(qn[0, 7]), 128 ** -0.5) > 150
    assert torch.exp2(torch.tensor(-N.log2_margin(N.C_NEEDLE, 1.0, 128 ** -0.5), dtype=torch.float32)) == 0.0
    # background keys / non-probe queries are exactly 0 in the probe directions
    dirs = N.probe_dirs(8, 128)
    assert len(set(dirs)) == 8 and all(0 <= d < 128 for d in dirs)
    assert len(set(N.probe_dirs(80, 80))) == 80
    bg = N.background((64, 128), torch.Generator().manual_seed(0), dirs)
    assert float(bg[:, dirs].abs().max()) == 0.0 and float(bg.abs().max()) < 2.0


def test_build_keys_needles_and_poison():
    gen = torch.Generator().manual_seed(1)
    dirs = N.probe_dirs(2, 128)
    K, V = N.build_keys(100, 128, dirs, {dirs[0]: [3, 50], dirs[1]: [7]}, {dirs[0]: range(60, 100), dirs[1]: [50, 8]}, gen, salt=4)
    assert K[3, dirs[0]] == N.C_NEEDLE and K[7, dirs[1]] == N.C_NEEDLE and K[60, dirs[0]] == N.C_NEEDLE
    assert torch.equal(V[50], N.v_rows(torch.tensor([50]), 128, 4)[0]), "a needle keeps its V when it is another probe's poison"
    assert (V[60:] == N.POISON_V).all() and (V[8] == N.POISON_V).all()
    # V rows: multiples of 1/8 in [-4, 4], distinct per key and per salt
    r = N.v_rows(torch.arange(6464), 128, 0)
    assert float(r.abs().max()) <= 4.0 and torch.equal(r * 8, (r * 8).round())
    assert torch.unique(r, dim=0).shape[0] == 6464
    assert not torch.equal(N.v_rows(torch.arange(64), 128, 1), N.v_rows(torch.arange(64), 128, 2))


def _brute_softmax(q, k, v, valid, scale):
    out = []
    for i in range(q.shape[0]):
        s = [float(q[i].double() @ k[j].double()) * scale for j in range(k.shape[0]) if valid[i, j]]
        vs = [v[j].double() for j in range(k.shape[0]) if valid[i, j]]
        m = max(s)
        w = [pow(2.718281828459045, x - m) for x in s]
        tot = sum(w)
        out.append(sum(wi * vi for wi, vi in zip(w, vs)) / tot)
    return torch.stack(out)


def test_float64_reference_matches_brute_force():
    g = torch.Generator().manual_seed(2)
    q, k, v = torch.randn((5, 16), generator=g), torch.randn((23, 16), generator=g), torch.randn((23, 16), generator=g)
    valid = torch.rand((5, 23), generator=g) > 0.4
    valid[:, 0] = True
    valid[4] = torch.arange(23) <= 4          # a causal row
    got = N.attn_ref(q, k, v, valid, 0.25)
    ref = _brute_softmax(q, k, v, valid, 0.25)
    assert got.dtype == torch.float64 and float((got - ref).abs().max()) < 1e-12
    # needle construction: the reference returns exactly the needle row / the exact mean of equal needles
    dirs = N.probe_dirs(1, 128)
    K, V = N.build_keys(300, 128, dirs, {dirs[0]: [0, 65, 130, 299]}, {}, g)
    out = N.attn_ref(N.probe_query(128, dirs[0])[None], K, V, torch.ones((1, 300), dtype=torch.bool), 128 ** -0.5)
    exact = V[[0, 65, 130, 299]].double().mean(0)
    assert torch.equal(out[0].to(torch.bfloat16).double(), exact)


def test_equal_needle_means_are_exact_in_bf16():
    """Every 2- and 4-needle mean of V rows is a multiple of 1/32 in [-4, 4]: exactly representable in bf16, so the expected
    output of an equal-needle case carries no rounding."""
    rows = N.v_rows(torch.arange(0, 6464, 97), 128, 3).double()
    for a, b in itertools.combinations(range(rows.shape[0]), 2):
        m = (rows[a] + rows[b]) / 2
        assert torch.equal(m.to(torch.bfloat16).double(), m)
    for idx in itertools.combinations(range(12), 4):
        m = rows[list(idx)].mean(0)
        assert torch.equal(m.to(torch.bfloat16).double(), m)
    for n in (1, 2, 3, 4, 5, 17, 64, 65, 4097, 6144, 6464):
        for grp in N.needle_groups(n, (16, 64, 4096)):
            assert len(grp) in (1, 2, 4) and len(set(grp)) == len(grp) and all(0 <= p < n for p in grp)


def test_ulp_helper():
    assert float(N.bf16_ulp(torch.tensor([1.0]))) == 2.0 ** -7
    assert float(N.bf16_ulp(torch.tensor([-3.9]))) == 2.0 ** -6
    N.assert_within_ulp(torch.tensor([1.0 + 2 ** -7]), torch.tensor([1.0]), "one ulp")
    try:
        N.assert_within_ulp(torch.tensor([1.0 + 2 ** -6]), torch.tensor([1.0]), "two ulps")
    except AssertionError:
        return
    raise AssertionError("two ulps passed")
