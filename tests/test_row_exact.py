"""The interval references of tests/row_exact.py have teeth and their case tables are valid (no GPU, no library): the
zero-slack midpoint is torch's float64 norm, every subtly wrong norm leaves the interval on every row it is aimed at, the
rotary mutants differ from the exact expectation, and no case has more than 2 % of its elements ambiguous."""
import numpy as np
import pytest
import torch

import row_exact as X

NORM_TENSORS = [(N, rows) for N in X.NORM_N for rows in X.NORM_ROWS]


def _norm_cases():
    for N, rows in NORM_TENSORS:
        x, w, b = X.norm_inputs(N, rows)
        for eps in X.NORM_EPS:
            for ln in (False, True):
                yield N, rows, eps, ln, x, w, (b if ln else None)


def test_constants():
    assert X.sum_slack(10) == 88 * 2.0 ** -24
    assert X.rstd_slack(10) == 3 * 2.0 ** -20 < 2.0 ** -17
    assert [X.chunks(N) for N in X.NORM_N] == [3, 3, 3, 3, 3, 7, 7, 10, 10]
    assert [X.quant_kernel(K) for K in X.QUANT_K] == [
        "kernel<3>", "kernel<3>", "kernel<8>", "kernel<8>", "wide<8>", "wide<8>", "wide<12>", "wide<12>", "rowwg<6>", "rowwg<6>",
        "rowwg<10>", "rowwg<10>", "rowwg<10>", "kernel<8> streaming"]


def test_midpoint_is_the_float64_norm():
    for N, rows, eps, ln, x, w, b in _norm_cases():
        lo, hi = X.norm_interval(x, w, b, eps, slack=False)
        assert torch.equal(lo, hi)
        xd, e32 = x.double(), float(np.float32(eps))
        if ln:
            ref = torch.nn.functional.layer_norm(xd, (N,), w.double(), b.double(), e32)
        else:
            ref = w.double() * X.bf16r(xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + e32))
        assert torch.equal(lo, X.bf16r(ref)), (N, rows, eps, ln)
        lo, hi = X.norm_interval(x, w, b, eps, X.chunks(N))
        assert bool(((lo <= X.bf16r(ref)) & (X.bf16r(ref) <= hi)).all())


def test_special_rows_are_exact():
    """The all-zero row: RMSNorm exactly 0, LayerNorm exactly b, no ambiguity."""
    for N, rows, eps, ln, x, w, b in _norm_cases():
        lo, hi = X.norm_interval(x, w, b, eps, X.chunks(N))
        z = X.row_kinds(rows).index("zero")
        want = b.double() if ln else torch.zeros(N, dtype=torch.float64)
        assert torch.equal(lo[z], want) and torch.equal(hi[z], want)


@pytest.mark.parametrize("kind", X.MUTANTS)
def test_norm_mutants_leave_the_interval(kind):
    hit = 0
    for N, rows, eps, ln, x, w, b in _norm_cases():
        rows_t = X.mutant_targets(kind, ln, N, rows)
        if rows_t is None:
            continue
        lo, hi = X.norm_interval(x, w, b, eps, X.chunks(N))
        out = X.outside(X.norm_mutant(kind, x, w, b, eps), lo, hi)
        for r in rows_t:
            assert bool(out[r].any()), f"{kind} passes on row {r} ({X.row_kinds(rows)[r]}) of N={N} rows={rows} eps={eps} ln={ln}"
            hit += 1
    assert hit >= 16


def test_ambiguity_cap_norms():
    worst = {False: 0.0, True: 0.0}
    for N, rows, eps, ln, x, w, b in _norm_cases():
        share = X.ambiguous_share(*X.norm_interval(x, w, b, eps, X.chunks(N)))
        assert share <= X.AMBIGUOUS_CAP, (N, rows, eps, ln, share)
        worst[ln] = max(worst[ln], share)
    print(f"ambiguous share: rmsnorm {worst[False]:.4%}, layernorm {worst[True]:.4%}")


def test_ambiguity_cap_heads_and_finalize():
    worst_h = worst_f = 0.0
    for tokens in (1, 5):
        for heads in (1, 3, 4, 5, 8):
            x, w = X.heads_inputs(tokens, heads, 0)
            share = X.ambiguous_share(*X.norm_interval(x.reshape(tokens * heads, 128), w, None, 1e-6, X.chunks(128, "heads")))
            assert share <= X.AMBIGUOUS_CAP, (tokens, heads, share)
            worst_h = max(worst_h, share)
    for N in X.FIN_N:
        for ks in X.FIN_KS:
            part, bias, R, w, b = X.finalize_inputs(N, ks)
            for use_b, use_r in ((True, True), (False, False)):
                xo = X.finalize_x(part, bias if use_b else None, R if use_r else None)
                for ln in (False, True):
                    share = X.ambiguous_share(*X.norm_interval(xo, w, b if ln else None, 1e-6, X.chunks(N, "finalize")))
                    assert share <= X.AMBIGUOUS_CAP, (N, ks, use_b, ln, share)
                    worst_f = max(worst_f, share)
    print(f"ambiguous share: rmsnorm_heads {worst_h:.4%}, finalize_norm {worst_f:.4%}")


def test_ambiguity_cap_fused_quantiser():
    """Bytes with unequal bounds, at the midpoint's scale; the scale interval holds the midpoint's scale."""
    worst = {False: 0.0, True: 0.0}
    for K in X.FUSED_K:
        for rows in X.NORM_ROWS:
            x, w, b = X.norm_inputs(K, rows)
            for eps in X.NORM_EPS:
                for ln in (False, True):
                    lo, hi = X.norm_interval(x, w, b if ln else None, eps, X.chunks(K, "quant"))
                    mid, _ = X.norm_interval(x, w, b if ln else None, eps, slack=False)
                    sc = X.quant_scale(mid.abs().amax(1).numpy())
                    s_lo, s_hi = X.fused_scale_interval(lo, hi)
                    assert bool(((s_lo <= sc) & (sc <= s_hi)).all())
                    blo, bhi = X.fused_byte_interval(lo, hi, sc)
                    assert bool((blo <= bhi).all())
                    share = X.ambiguous_share(blo, bhi)
                    assert share <= X.AMBIGUOUS_CAP, (K, rows, eps, ln, share)
                    worst[ln] = max(worst[ln], share)
    print(f"ambiguous byte share: fused RMSNorm {worst[False]:.4%}, fused LayerNorm {worst[True]:.4%}")


def test_quantiser_rows():
    for K in X.QUANT_K:
        x, pos = X.quant_inputs(K)
        q, sc = X.quant_expect(x)
        three = np.float32(3.0) / np.float32(448.0)
        want = set(X.plant_positions(K))
        assert {0, 7, K - 8, K - 1} <= want and all(p % 8 == 0 or p in (7, 511, K - 1) for p in want)
        for r, p in enumerate(pos):
            if p >= 0:
                assert sc[r] == three and abs(float(X.e4m3_value(q)[r, p])) == 448.0
                assert float(x[r].float().abs().sort().values[-2]) <= 1.0
        z = pos.index(-1)
        assert sc[z] == np.float32(1e-12) and int(q[z].max()) == 0
    assert X.e4m3_bytes(torch.tensor([1e9, -1e9, 464.0, 0.0])).tolist() == [0x7E, 0xFE, 0x7E, 0]      # saturating, no NaN


def test_rope_tables():
    cases = X.ROPE_CASES
    assert 36 <= len(cases) <= 48 and len({c.id for c in cases}) == len(cases)
    for HD in (128, 80):
        mine = [c for c in cases if c.HD == HD]
        assert {c.S for c in mine} == set(X.ROPE_S) and {(c.Hq, c.Hkv) for c in mine} >= set(X.ROPE_HEADS)
        for flag in ("ld_pad", "k_pos0", "vt_col0"):
            assert any(getattr(c, flag) for c in mine)
        assert any(not c.rot for c in mine) and any(not c.v for c in mine) and any(not c.vt for c in mine)
    assert torch.equal(X.vt_key_order(64)[:12], torch.tensor([0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7]))
    assert sorted(X.vt_key_order(128).tolist()) == list(range(128))


@pytest.mark.parametrize("case", [c for c in X.ROPE_CASES if c.rot and c.v and c.vt], ids=lambda c: c.id)
def test_rope_exact_and_mutants(case):
    qkv, cos, sin, exp = X.rope_build(case)                  # asserts representability
    half = case.HD // 2
    assert not torch.equal(cos[:, :half], cos[:, half:]) or case.S * half < 8
    for m in X.ROPE_MUTANTS:
        if m == "vt_plain" and (case.Hkv == 0 or case.S < 5):
            continue                                          # keys 0..3 sit at columns 0..3 in both orders
        if m == "head_off" and case.Hq + 2 * case.Hkv < 2:
            continue
        bad = X.rope_expect(case, qkv, cos, sin, mutant=m)
        names = ("vt",) if m == "vt_plain" else tuple(n for n in ("q", "k") if exp[n].numel())
        assert any(not torch.equal(bad[n], exp[n]) for n in names), f"{case.id}: mutant {m} is invisible"


def test_rope_general_ambiguity_cap():
    for case in X.ROPE_GENERAL:
        qkv, cos, sin = X.rope_inputs(case)
        half = case.HD // 2
        assert not torch.equal(cos[:, :half], cos[:, half:]) and not torch.equal(sin[:, :half], sin[:, half:])
        exp = X.rope_expect(case, qkv, cos, sin, slack=2.0 ** -22)
        for n in ("q", "k"):
            lo, hi = exp[n]
            assert bool((lo <= hi).all()) and X.ambiguous_share(lo, hi) <= X.AMBIGUOUS_CAP
        for m in ("half_table", "sign", "head_off"):
            bad = X.rope_expect(case, qkv, cos, sin, mutant=m)
            assert bool(X.outside(X.bf16r(bad["q"]), *exp["q"]).any())
