"""CPU checks of tests/attn_weights.py: the scale identity, exactness and ambiguity of every GPU case, and discrimination - a
float32 emulation of the kernels' two softmax schemes passes the check on every case, each planted fault does not.

Ambiguous shares (lo != hi) per family are printed by test_every_case_is_exact_and_under_the_cap (run with -s)."""
import numpy as np
import pytest

import attn_weights as W

CASES = W.cpu_cases()


def test_scale_identity():
    """scale * 1.4426950408889634f is exactly 0.125 in float32, and SCALE is a float32 number (it crosses the ABI as one)."""
    assert np.float32(0.6931471824645996) * np.float32(1.4426950408889634) == np.float32(1.0)
    assert np.float32(W.SCALE) * W.LOG2E_F32 == np.float32(0.125)
    assert float(np.float32(W.SCALE)) == W.SCALE
    assert np.float32(W.QV) * np.float32(0.125) == 1.0
    assert float(np.exp2(np.float32(W.BG + W.WINDOW))) == 0.0        # a background weight is 0 in f32


def test_profile_table_holds_the_required_shapes():
    six = W.tiles(0, 321)
    assert len(six) == 6 and six[-1] == (320, 321)
    for name, step in (("rise1", 1), ("rise7", 7), ("rise8", 8), ("rise9", 9), ("rise12", 12)):
        col = W.place(name, six)
        assert max(v for k, v in col.items() if k < 64) + step == max(v for k, v in col.items() if 64 <= k < 128) == 0
    assert set(W.place("bg_first", six)) <= set(range(320, 321)) and min(W.place("bg_first", W.tiles(0, 130))) >= 128
    assert sorted(W.place("two_max", six).items())[0] == (0, 0) and W.place("two_max", six)[320] == 0
    e = W.place("edges", W.tiles(0, 130))
    assert {63, 64, 127, 128} <= set(e)
    assert len({k // 64 for k in W.place("one_tile", six)}) == 1 and len(W.place("one_tile", six)) == W.A_MAX
    assert len({k // 64 for k in W.place("max_first", six)}) == 6
    f = W.place("fall", six)
    assert [max(v for k, v in f.items() if k // 64 == t) for t in range(4)] == [0, -5, -9, -12]
    assert W.place("app_max", W.tiles(0, 200))[199] == 0 and W.place("app_min", W.tiles(0, 200))[199] == -W.WINDOW
    assert W.place("app_min", W.tiles(0, 1)) == {0: -W.WINDOW}               # a single valid key
    long = W.place("edges", W.tiles(0, 4161))
    assert 4095 in long and 4096 in long                                        # past the combine's 64 preloaded splits
    assert max(W.place("two_max", W.tiles(0, 4161))) == 4160


def test_every_case_is_exact_and_under_the_cap():
    """`reference` asserts integer scores, window / background structure and the 2^24 bound; the ambiguous share of every case
    stays under AMBIGUOUS_CAP."""
    worst = {}
    for fam, name, units, _ in CASES:
        amb, tot = W.ambiguous(units)
        worst[fam] = max(worst.get(fam, 0.0), amb / tot)
        assert amb <= W.AMBIGUOUS_CAP * tot, f"{name}: {amb}/{tot} outputs ambiguous"
    print("ambiguous share, max per family: " + "  ".join(f"{k} {100 * v:.2f} %" for k, v in worst.items()))
    assert W.rel_slack(8) == 2.0 ** -17


def test_single_key_and_lazy_boundary_queries_exist():
    """The prefill cases hold a query with one valid key, queries whose tile maximum exceeds the reference by exactly 8 and by
    exactly 9, and a query whose first tile is all background; the decode cases a context of one key."""
    c = W.prefill128(321, False, 2, 2)
    s = c.units[0].s
    t0 = s[:, :64].max(1)
    t1 = s[:, 64:128].max(1)
    assert ((t1 - t0) == 8).any() and ((t1 - t0) == 9).any() and (t0 == W.BG).any()
    c = W.prefill128(65, True, 4, 1)
    assert ((c.units[0].s != W.MASKED).sum(1) == 1).any()
    assert any(u.s.shape[1] == 1 for u in W.decode_case(28, 4, 512, W.DECODE_CTXS).units)


def _emulations(kind):
    if kind == "lazy":
        return [lambda u, f: W.emulate_lazy(u, f)]
    if kind == "lazy_f32sum":
        return [lambda u, f: W.emulate_lazy(u, f, f32sum=True)]
    return [W.emulate_stream, W.emulate_split]


def test_fault_free_emulation_passes_every_case():
    for fam, name, units, kind in CASES:
        for emu in _emulations(kind):
            for i, u in enumerate(units):
                W.check(u, emu(u, None), f"{name} unit {i}")


def _worst_share(fault, kinds, emus=None):
    worst = 0.0
    for fam, name, units, kind in CASES:
        if kind not in kinds or "4608" in name or "key-split" in name:
            continue
        for emu in (emus or _emulations(kind)):
            bad = tot = 0
            for u in units:
                o = W.outside(u, emu(u, fault))
                bad += int(o.sum())
                tot += o.size
            worst = max(worst, bad / tot)
    return worst


@pytest.mark.parametrize("fault", W.LAZY_FAULTS)
def test_lazy_scheme_faults_are_rejected(fault):
    """alpha of the neighbouring query; O rescaled but not the sum, and the reverse; the >= 8 boundary with p clamped to 1; a
    reference that never moves after tile 0; a numerator p one bf16 ulp off the denominator's; background at 2^-12."""
    assert _worst_share(fault, ("lazy", "lazy_f32sum")) > W.AMBIGUOUS_CAP


@pytest.mark.parametrize("fault,emu", [("combine_xor1", W.emulate_split), ("pal_next_head", W.emulate_stream),
                                       ("bg_weight", W.emulate_split), ("bg_weight", W.emulate_stream)])
def test_decode_scheme_faults_are_rejected(fault, emu):
    assert _worst_share(fault, ("decode",), [emu]) > W.AMBIGUOUS_CAP


def test_check_names_the_query():
    u = W.prefill128(65, False, 2, 2).units[0]
    got = W.emulate_lazy(u)
    got[3, 5] += 1.0
    with pytest.raises(AssertionError, match=r"query row 3 head 0 dir \d+ profile \w+.*dim 5"):
        W.check(u, got, "case")
    got = W.emulate_lazy(u)
    got[0, 0] = 4096.0
    with pytest.raises(AssertionError):
        W.check(u, got, "case")
