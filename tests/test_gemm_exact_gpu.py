"""Exact-arithmetic tests of every prefill GEMM tile kernel and epilogue (vis_gemm_bf16, vis_gemm_fp8, the split-K forms).

Operands and the float64 reference come from tests/gemm_exact.py (integers whose every rounded value is representable);
tests/test_gemm_exact.py shows, without a GPU, that the case table reaches every kernel x epilogue form x epilogue kind.
Here: bit-exact results (activations: the derived one-ulp rule), layouts with NaN canaries, in-place residuals, split-K
slabs, and the dispatcher's claim that the tile choice - a function of M - never changes a result bit.
"""
import math

import pytest
import torch

import gemm_exact as G

pytestmark = pytest.mark.gpu

REPEATS = 3          # a staging race comes and goes


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _dev(ops, device):
    """Operand buffers on the device, logical views into them."""
    d = {}
    for k in ("A", "W", "R"):
        d[k] = None if ops[k] is None else ops[k].view(ops[k].flat.to(device))
    for k in ("bias", "sa", "sw"):
        d[k] = None if ops[k] is None else ops[k].to(device)
    return d


def _run(hip, case, d, out, **kw):
    if case.entry == "bf16":
        return hip.gemm(d["A"], d["W"], bias=d["bias"], residual=d["R"], act=case.act, out=out)
    return hip.gemm_fp8(d["A"], d["sa"], d["W"], d["sw"], bias=d["bias"], residual=d["R"], act=case.act, out=out, **kw)


def _prepare(case, device):
    """Build the case once (float64 on the host) and put on the device what the comparisons need: the operands, and the
    whole expected C buffer - reference inside, NaN canaries outside - so that one bit comparison checks values, canaries
    and stray NaN together.  Activation kinds carry the reference and the derived tolerance instead."""
    ops = G.build(case)
    pr = dict(d=_dev(ops, device), C=ops["C"], R=ops["R"], c_init=ops["C"].flat.to(device))
    if ops["tol"] is None:
        pr["c_want"] = G.expected_flat(ops["C"], ops["ref"]).to(device)
        if ops["R"] is not None:
            pr["x_init"] = ops["R"].flat.to(device)
            pr["x_want"] = G.expected_flat(ops["R"], ops["ref"]).to(device)
    else:
        pr["ref"], pr["tol"] = ops["ref"].to(device), ops["tol"].to(device)
        pr["c_blank"] = G.expected_flat(ops["C"], torch.zeros_like(ops["ref"])).to(device)
    return pr


def _bits(t):
    return t.view(torch.int16)


def _verify(case, pr, c_flat, what):
    """Fast path on the device; whatever it does not accept goes to the host checker (gemm_exact.check: torch.equal on the
    values / the tolerance, canaries, NaN), which decides and names the first wrong element."""
    if "c_want" in pr:
        ok = torch.equal(_bits(c_flat), _bits(pr["c_want"]))
    else:
        got = pr["C"].view(c_flat).double()
        ok = bool(((got - pr["ref"]).abs() <= pr["tol"]).all())            # a NaN compares False
        if ok:
            rest = c_flat.clone()
            pr["C"].view(rest).zero_()
            ok = torch.equal(_bits(rest), _bits(pr["c_blank"]))
    if not ok:
        G.check(case, G.build(case), c_flat, what)


# ----------------------------------------------------------------------------- 1 + 2: exact results in every layout
INPLACE = [c for c in G.CASES if c.kind in ("residual", "bias_residual") and (c.M >= 300 or c.K == 18944 or c.M == 100)]
_STASH = {}          # test_exact keeps the device operands of the INPLACE cases for test_in_place_residual (no second build)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_exact(hip, device, case):
    """torch.equal against the float64 reference (activations: within one bf16 ulp + the activation's documented error),
    NaN canaries around C bit-for-bit intact, NaN padding of A / W / R without effect; three runs."""
    pr = _prepare(case, device)
    d = pr["d"]
    c_flat = pr["c_init"].clone()
    # the epilogue form the case table claims (test_gemm_exact.py) is the one these pointers get
    lda, ldw, ldc, ldr, off = case.ld()
    ptrs = pr["C"].view(c_flat).data_ptr() | (d["R"].data_ptr() if d["R"] is not None else 0)
    assert (ptrs % 16 == 0) == (off == 0) and ptrs % 8 == 0
    for rep in range(REPEATS):
        c_flat.copy_(pr["c_init"])                          # NaN everywhere, the logical output included
        _run(hip, case, d, pr["C"].view(c_flat))
        _verify(case, pr, c_flat, f"run {rep}")
    if case in INPLACE:
        _STASH[case] = pr


def test_argument_errors_write_nothing(hip, device):
    """ldc % 4 != 0, a misaligned A, a misaligned C: VIS_ERR_ARG (status 1) from the host checks before any launch, C untouched."""
    case = G.Case("bf16", 130, 132, 128, "plain", "padded")
    ops = G.build(case)
    d = _dev(ops, device)
    c_flat = ops["C"].flat.to(device)
    before = c_flat.clone()
    bad_ldc = c_flat.as_strided((case.M, case.N), (case.N + 2, 1), 0)
    a_off = ops["A"].flat.to(device).as_strided((case.M, case.K), (ops["A"].ld, 1), 4)       # 8-byte, not 16-byte aligned
    c_odd = c_flat.as_strided((case.M, case.N), (ops["C"].ld, 1), 2)                           # 4-byte aligned
    for a, out in ((d["A"], bad_ldc), (a_off, ops["C"].view(c_flat)), (d["A"], c_odd)):
        with pytest.raises(hip.HipLibraryError, match="vis_gemm_bf16 failed with status 1 "):
            hip.gemm(a, d["W"], out=out)
    f8 = G.Case("fp8", 130, 132, 128, "plain", "padded")
    o8 = G.build(f8)
    d8 = _dev(o8, device)
    a8_off = o8["A"].flat.to(device).as_strided((f8.M, f8.K), (o8["A"].ld, 1), 8)
    for a, out in ((d8["A"], bad_ldc), (a8_off, ops["C"].view(c_flat)), (d8["A"], c_odd)):
        with pytest.raises(hip.HipLibraryError, match="vis_gemm_fp8 failed with status 1 "):
            hip.gemm_fp8(a, d8["sa"], d8["W"], d8["sw"], out=out)
    torch.cuda.synchronize()
    assert torch.equal(c_flat.view(torch.int16), before.view(torch.int16))


# ----------------------------------------------------------------------------- 3: in place (residual is out)
@pytest.mark.parametrize("case", INPLACE, ids=lambda c: c.id)
def test_in_place_residual(hip, device, case):
    """The engines call every o / proj / fc2 / down projection with residual=x, out=x: bit-identical to out of place and
    to the exact reference, in every kernel and in the mixed plans."""
    pr = _STASH.pop(case, None) or _prepare(case, device)
    d = pr["d"]
    ref_flat = pr["c_init"].clone()
    _run(hip, case, d, pr["C"].view(ref_flat))
    _verify(case, pr, ref_flat, "out of place")
    for rep in range(REPEATS):
        x_flat = pr["x_init"].clone()
        x = pr["R"].view(x_flat)
        _run(hip, case, dict(d, R=x), x)
        assert torch.equal(x, pr["C"].view(ref_flat)), f"{case.id} run {rep}: in place differs from out of place"
        if not torch.equal(_bits(x_flat), _bits(pr["x_want"])):                 # values, canaries around x, stray NaN
            ops = G.build(case)
            got = x.double().cpu()
            assert torch.equal(got, ops["ref"]), f"{case.id} in place, run {rep}: {int((got != ops['ref']).sum())} wrong elements"
            assert G.canary_intact(ops["R"], x_flat), f"{case.id} in place, run {rep}: the kernel wrote outside x"


# ----------------------------------------------------------------------------- 4: split-K
@pytest.mark.parametrize("M,N,K,ks", [(300, 520, 1088, 2), (300, 520, 1088, 3), (300, 520, 1088, 8), (257, 264, 18944, 2),
                                      (1030, 768, 576, 3)])
def test_splitk_bf16_exact(hip, device, M, N, K, ks):
    case = G.Case("bf16", M, N, K, "bias_residual", "padded")
    ops = G.build(case)
    d = _dev(ops, device)
    for rep in range(REPEATS):
        work = torch.full((ks * M * N,), float("nan"), dtype=torch.float32, device=device)
        c_flat = ops["C"].flat.to(device)
        hip.gemm_splitk(d["A"], d["W"], work, ks, bias=d["bias"], residual=d["R"], out=ops["C"].view(c_flat))
        G.check(case, ops, c_flat, f"split-K ks={ks} run {rep}")
        # the K-sliced tiles alone: every slab finite, their sum the exact integer product
        work.fill_(float("nan"))
        hip.gemm_splitk_part(d["A"], d["W"], work, ks)
        slabs = work.view(ks, M, N).double().cpu()
        assert bool(torch.isfinite(slabs).all()), "a partial slab holds an unwritten / NaN element"
        assert torch.equal(slabs.sum(0), ops["acc"])
        assert all(bool((slabs[i] != 0).any()) for i in range(ks))
        # ... and finalised by vis_splitk_finalize_norm: the rounded x exactly (y: test_splitk_finalize_norm's bit identity)
        x_flat = ops["C"].flat.to(device)
        hip.splitk_finalize_norm(work, ks, ops["C"].view(x_flat), bias=d["bias"], residual=d["R"])
        G.check(case, ops, x_flat, f"finalize_norm ks={ks} run {rep}")


@pytest.mark.parametrize("M,N,K,ks", [(300, 520, 1152, 2), (300, 520, 1152, 4), (257, 264, 18944, 2), (1270, 768, 1024, 4)])
def test_splitk_fp8_exact(hip, device, M, N, K, ks):
    case = G.Case("fp8", M, N, K, "bias_residual", "padded")
    ops = G.build(case)
    d = _dev(ops, device)
    for rep in range(REPEATS):
        work = torch.full((ks * M * N,), float("nan"), dtype=torch.float32, device=device)
        c_flat = ops["C"].flat.to(device)
        _run(hip, case, d, ops["C"].view(c_flat), work=work, ksplit=ks)
        G.check(case, ops, c_flat, f"fp8 split-K ks={ks} run {rep}")
        slabs = work.view(ks, M, N).double().cpu()
        assert bool(torch.isfinite(slabs).all())
        assert torch.equal(slabs.sum(0), ops["acc"])


# ----------------------------------------------------------------------------- 5: the tile choice never changes a bit
def _randn(shape, device, seed, scale=1.0):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=device) * scale).to(torch.bfloat16)


LADDER = [1, 100, 129, 1100, 2249, 4 * 2249]
LADDER_SHAPES = [(4608, 3584, "bias"), (3584, 3584, "bias_residual"), (37888, 3584, "swiglu")]   # LLM qkv, o, gate/up


def _ladder_plans(query, N, K, act, residual):
    plans = {}
    for m in LADDER:
        p = query(m, N, K, act=act, residual=residual)
        plans[m] = tuple((l["kernel"], l["n0"]) for l in p["launches"])
    return plans


@pytest.mark.parametrize("N,K,kind", LADDER_SHAPES)
def test_row_count_invariance_bf16(hip, device, N, K, kind):
    """gemm_dispatch: "Every kernel accumulates K in the same order, so the choice (which depends on M) never changes a
    result bit."  Real-valued data (no integer trick): rows [0, m) are bit-identical whether they run alone or stacked
    under more rows, across a ladder of M that the plan query shows crossing the kernel boundaries."""
    act = G.ACT_OF[kind]
    res = kind.endswith("residual")
    plans = _ladder_plans(hip.gemm_plan, N, K, act, res)
    assert len(set(plans.values())) >= 3, plans
    mx = LADDER[-1]
    a = _randn((mx, K), device, 41)
    w = _randn((N, K), device, 42, 1.0 / math.sqrt(K))
    b = _randn((N,), device, 43)
    r = _randn((mx, N), device, 44) if res else None
    full = hip.gemm(a, w, bias=b, residual=r, act=act)
    assert bool(torch.isfinite(full.float()).all()) and float(full.float().abs().mean()) > 0.05
    for m in LADDER[:-1]:
        got = hip.gemm(a[:m], w, bias=b, residual=None if r is None else r[:m], act=act)
        diff = got != full[:m]
        assert not bool(diff.any()), (f"M = {m} ({plans[m]}) against M = {mx} ({plans[mx]}): {int(diff.sum())} elements differ, "
                                      f"first at {torch.nonzero(diff)[0].tolist()}")


@pytest.mark.parametrize("N,K,kind", LADDER_SHAPES)
def test_row_count_invariance_fp8(hip, device, N, K, kind):
    act = G.ACT_OF[kind]
    res = kind.endswith("residual")
    bias = kind.startswith("bias")
    ladder = LADDER[:-1] + [5200, LADDER[-1]]            # 5200: whole ping-pong rounds + 128x128 remainder columns
    plans = {m: hip.gemm_fp8_plan(m, N, K, act=act, residual=res)["kernels"] for m in ladder}
    assert len(set(plans.values())) >= 3, plans
    mx = ladder[-1]
    a = _randn((mx, K), device, 51)
    w = _randn((N, K), device, 52, 1.0 / math.sqrt(K))
    b = _randn((N,), device, 53) if bias else None
    r = _randn((mx, N), device, 54) if res else None
    aq, sa = hip.quant_rows_fp8(a)                      # row-wise: the same quantised rows at every M
    wq, sw = hip.quantize_fp8_rows(w)
    full = hip.gemm_fp8(aq, sa, wq, sw, bias=b, residual=r, act=act)
    assert bool(torch.isfinite(full.float()).all()) and float(full.float().abs().mean()) > 0.05
    for m in ladder[:-1]:
        got = hip.gemm_fp8(aq[:m], sa[:m], wq, sw, bias=b, residual=None if r is None else r[:m], act=act)
        diff = got != full[:m]
        assert not bool(diff.any()), (f"M = {m} ({plans[m]}) against M = {mx} ({plans[mx]}): {int(diff.sum())} elements differ, "
                                      f"first at {torch.nonzero(diff)[0].tolist()}")


@pytest.mark.parametrize("fp8", [False, True])
def test_row_count_invariance_splitk(hip, device, fp8):
    """The down projection's split-K at a fixed slice count: one kernel, but the rows' results must not depend on M either."""
    N, K, ks = 3584, 18944, 2
    ladder = [1, 100, 300, 2249]
    mx = ladder[-1]
    a = _randn((mx, K), device, 61)
    w = _randn((N, K), device, 62, 1.0 / math.sqrt(K))
    b = _randn((N,), device, 63)
    r = _randn((mx, N), device, 64)
    work = torch.empty(ks * mx * N, dtype=torch.float32, device=device)
    if fp8:
        aq, sa = hip.quant_rows_fp8(a)
        wq, sw = hip.quantize_fp8_rows(w)
        run = lambda m: hip.gemm_fp8(aq[:m], sa[:m], wq, sw, bias=b, residual=r[:m], work=work, ksplit=ks)
    else:
        run = lambda m: hip.gemm_splitk(a[:m], w, work, ks, bias=b, residual=r[:m])
    full = run(mx).clone()
    for m in ladder[:-1]:
        got = run(m)
        assert torch.equal(got, full[:m]), f"split-K rows differ between M = {m} and M = {mx}"
