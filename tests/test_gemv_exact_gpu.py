"""The bf16 and fp8 GEMV kernels (vis_gemv_bf16 / _rows / _argmax / _argmax_masked, vis_gemv_fp8w / _rows) against float64 on
operands for which f32 is exact in any order (tests/gemv_exact.py): every comparison is bit for bit, except the one bf16 ulp
silu_fast gets in the two SwiGLU tests.  One dropped or doubled 16-byte chunk, a stale accumulator, a wrong row of a clamped
pair or a wrong tie rule is a wrong integer here, whatever K is.

The line of csrc/decode.hip / csrc/decode_common.hip.h each shape was chosen to reach (checked in tests/test_gemv_exact.py
through the restated task walk):

bf16 (a task = one row pair x one segment of 8 x 64 chunks of 8 elements):
  (1, 8)        one row (gv_rows' clamped second row is the first), one chunk: 63 lanes of gv_consume read a clamped chunk
  (7, 704)      odd N; 88 chunks: the second lane wrap is partial; 4 pairs on 4 waves
  (6, 4096)     exactly one full segment, no clamped chunk; an idle wave (n_tasks = 0)
  (6, 4104)     nseg = 2, the second segment holds ONE live chunk; the accumulators carry across the ring A -> B
  (5, 18944)    the down projection's K, nseg = 5, gv_stage_x with 10 chunks per thread
  (6, 30720)    the launchers' K limit: gv_stage_x's last (15th) pass, nseg = 8
  (1001, 256)   odd N over 126 workgroups
  (8202, 4104)  1024 workgroups, waves that walk two pairs with nseg = 2: the accumulator reset in the B half, then B -> A
  (16400, 64)   waves with two pairs, nseg = 1: the reset in the A half, A -> B
  (24583, 64)   waves with three pairs, nseg = 1: both resets, A -> B and B -> A; odd N
fp8 (<2, 8>: a task = 2 rows x 8 x 64 chunks of 16 elements; <4, 4>: 4 rows x 4 x 64 chunks):
  (1, 16) (7, 1424) (6, 8192) (6, 8208) (5, 18944) (6, 30720) (1001, 256): the bf16 list's edges on <2, 8> (89 chunks; one
                full segment; nseg = 2 with a one-chunk tail; nseg = 3; the K limit, nseg = 4)
  (8197, 64)    <4, 4>, N % 4 = 1: three clamped rows in the last row group (gf_rows), gf_finish's `o >= N` break
  (8198, 4112)  <4, 4>, nseg = 2 with a one-chunk tail, N % 4 = 2
  (16402, 128)  <4, 4>, waves with two row groups (A -> B)
  (40962, 64)   <4, 4>, waves with three row groups (A -> B and B -> A)
"""
import pytest
import torch

import gemv_exact as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _ids(shapes):
    return [f"{n}x{k}" for n, k in shapes]


def _sentinel(shape, dtype, device):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), G.SENTINEL, dtype=dtype, device=device)


def _expect(ref, dtype):
    """The float64 reference as the kernel must store it: exact in f32 (asserted by the builders), rounded once to bf16."""
    return ref.float() if dtype == torch.float32 else ref.float().to(torch.bfloat16)


def _same(got, want, what):
    got = got.cpu()
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).flatten()).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} wrong, first at {i}: got {float(got.flatten()[i])!r} "
                             f"want {float(want.flatten()[i])!r} (last wrong {int(bad[-1])})")


# ----------------------------------------------------------------------------- 1. exact sums, bf16
@pytest.mark.parametrize("N,K", G.BF16_SHAPES, ids=_ids(G.BF16_SHAPES))
def test_bf16_exact_sums(hip, device, N, K):
    c = G.bf16_case(N, K)
    x, w = c["x"][0].to(device), c["W"].to(device)
    bias, r = c["bias"].to(device), c["R"][0].to(device)
    wide = G.padded(c["W"], 24).to(device) if N <= G.PADDED_MAX_N else None
    for dtype in (torch.float32, torch.bfloat16):
        for full in (False, True):
            kw = dict(bias=bias, residual=r) if full else {}
            want = _expect((c["ref_br"] if full else c["ref"])[0], dtype)
            y = _sentinel((N,), dtype, device)
            hip.gemv(x, w, y, **kw)
            _same(y, want, f"gemv {N}x{K} {dtype} bias+residual={full}")
            if wide is not None:            # ldw = K + 24, NaN in the padding: the same elements are read, nothing else
                y2 = _sentinel((N,), dtype, device)
                hip.gemv(x, wide[:, :K], y2, **kw)
                _same(y2, want, f"gemv {N}x{K} ldw={K + 24} {dtype} bias+residual={full}")


# ----------------------------------------------------------------------------- 2. position pick, bf16
@pytest.mark.parametrize("K", G.PICK_K)
def test_bf16_permuted_identity_picks_positions(hip, device, K):
    """W = I[perm]: output n is x[perm[n]] and nothing else - a chunk read at the wrong place, or the x chunk of another
    lane, moves a value.  K = 4104 crosses the segment boundary (chunk 512), K = 520 the 64-lane wrap."""
    c = G.pick_case(K)
    x, w = c["x"].to(device), c["W"].to(device)
    want = c["x"][c["perm"]]
    y = _sentinel((K,), torch.bfloat16, device)
    hip.gemv(x, w, y)
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), "bf16 output is not x[perm] bit for bit"
    y32 = _sentinel((K,), torch.float32, device)
    hip.gemv(x, w, y32)
    assert torch.equal(y32.cpu().view(torch.int32), want.float().view(torch.int32)), "f32 output is not x[perm] bit for bit"


def test_bf16_one_hot_returns_the_column(hip, device):
    """x = e_k returns column k of W exactly, at the chunk, lane-wrap and segment boundaries of K = 4104."""
    N, K = G.ONE_HOT_SHAPE
    c = G.bf16_case(N, K)
    w = c["W"].to(device)
    for k in G.ONE_HOT_K:
        x = torch.zeros(K, dtype=torch.bfloat16, device=device)
        x[k] = 1.0
        y = _sentinel((N,), torch.float32, device)
        hip.gemv(x, w, y)
        _same(y, c["W"][:, k].float(), f"x = e_{k}")


# ----------------------------------------------------------------------------- 3. SwiGLU, bf16
def _check_swiglu(c, got, what):
    """One bf16 ulp, here and in the fp8 SwiGLU test only: silu_fast (v_exp_f32 + v_rcp_f32) is not exact, gate and up sums
    are.  What this pins is the gate-up pairing, the row mapping ((pair >> 4) << 5) + (pair & 15) and the output index: up
    values differ inside every group of 32 outputs (asserted by the builder), so a wrong pairing is off by far more."""
    want = c["ref"].to(torch.bfloat16).double()
    err = (got.cpu().double() - want).abs()
    bad = err > G.swiglu_tolerance(c["ref"])
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs off by more than 1 bf16 ulp, first {int(torch.nonzero(bad)[0])}"
    exact = c["gate"] == 0                    # silu(0) * u = 0 exactly
    assert bool((got.cpu().double()[exact] == 0).all())


@pytest.mark.parametrize("N,K", G.BF16_SWIGLU_SHAPES, ids=_ids(G.BF16_SWIGLU_SHAPES))
def test_bf16_swiglu_pairing(hip, device, N, K):
    """N = 32: one 16-group; 1440: 45 groups, K = 520 (65 chunks); (16448, 64): the several-pairs-per-wave grid."""
    c = G.swiglu_case("bf16", N, K)
    y = _sentinel((N // 2,), torch.bfloat16, device)
    hip.gemv(c["x"].to(device), c["W"].to(device), y, act=hip.ACT_SWIGLU)
    _check_swiglu(c, y, f"gemv swiglu {N}x{K}")


# ----------------------------------------------------------------------------- 4. exact sums, fp8
@pytest.mark.parametrize("N,K", G.FP8_SHAPES, ids=_ids(G.FP8_SHAPES))
def test_fp8_exact_sums(hip, device, N, K):
    c = G.fp8_case(N, K)
    x, wq, sc = c["x"][0].to(device), c["Wq"].to(device), c["scale"].to(device)
    bias, r = c["bias"].to(device), c["R"][0].to(device)
    wide = G.padded(c["Wq"], 32).to(device) if N <= G.PADDED_MAX_N else None
    for dtype in (torch.float32, torch.bfloat16):
        for full in (False, True):
            kw = dict(bias=bias, residual=r) if full else {}
            want = _expect((c["ref_br"] if full else c["ref"])[0], dtype)
            y = _sentinel((N,), dtype, device)
            hip.gemv_fp8(x, wq, sc, y, **kw)
            _same(y, want, f"gemv_fp8 {N}x{K} {dtype} bias+residual={full}")
            if wide is not None:            # ldw = K + 32, the e4m3 NaN byte in the padding
                y2 = _sentinel((N,), dtype, device)
                hip.gemv_fp8(x, wide[:, :K], sc, y2, **kw)
                _same(y2, want, f"gemv_fp8 {N}x{K} ldw={K + 32} {dtype} bias+residual={full}")


@pytest.mark.parametrize("N,K", G.FP8_SWIGLU_SHAPES, ids=_ids(G.FP8_SWIGLU_SHAPES))
def test_fp8_swiglu_pairing(hip, device, N, K):
    """(64, 256): the <2, 8> task shape (one output per task); (16448, 64): <4, 4> (two outputs per task: gate rows r[0], r[2],
    up rows r[1], r[3], each with its own scale).  Tolerance and purpose: _check_swiglu."""
    c = G.swiglu_case("fp8", N, K)
    y = _sentinel((N // 2,), torch.bfloat16, device)
    hip.gemv_fp8(c["x"].to(device), c["Wq"].to(device), c["scale"].to(device), y, act=hip.ACT_SWIGLU)
    _check_swiglu(c, y, f"gemv_fp8 swiglu {N}x{K}")


# ----------------------------------------------------------------------------- 5. every e4m3 code
@pytest.mark.parametrize("scaled", [False, True], ids=["scale1", "scale_pow2"])
def test_fp8_every_code(hip, device, scaled):
    """Row n holds finite code n in column n % 16 and zeros elsewhere, x = 1: y[n] is the value of the code (times the row's
    scale).  Pins v_cvt_scalef32_pk_bf16_fp8 for all 254 finite bytes and the byte order within a 16-byte load.  Value
    equality: the -0 code sums to +0."""
    codes = torch.tensor(G.E4M3_FINITE, dtype=torch.uint8)
    N, K = 254, 16
    wq = torch.zeros((N, K), dtype=torch.uint8)
    wq[torch.arange(N), torch.arange(N) % 16] = codes
    scale = torch.ldexp(torch.ones(N), torch.arange(N) % 5 - 2) if scaled else torch.ones(N)
    want = codes.view(torch.float8_e4m3fn).float() * scale
    assert len(torch.unique(want)) > 250 or scaled
    y = _sentinel((N,), torch.float32, device)
    hip.gemv_fp8(torch.ones(K, dtype=torch.bfloat16, device=device), wq.to(device), scale.to(device), y)
    _same(y, want, "e4m3 codes")


# ----------------------------------------------------------------------------- 6. rows forms
def _rows_layout(c, B, N, K, dtype, device):
    """x as a view with ldx = K + 8 (NaN in the padding), out inside a wider sentinel buffer with a row below (ldy = N + 16),
    the residual likewise (ldr = N + 24, NaN around it)."""
    xb = torch.full((B, K + 8), G.NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    xb[:, :K] = c["x"]
    rb = torch.full((B + 1, N + 24), G.NAN_BF16, dtype=torch.int16).view(torch.bfloat16)
    rb[:B, :N] = c["R"]
    ob = _sentinel((B + 1, N + 16), dtype, device)
    return xb.to(device)[:, :K], rb.to(device)[:B, :N], ob


def _check_rows(c, ob, B, N, dtype, what):
    _same(ob[:B, :N], _expect(c["ref_br"], dtype), what)
    outside = torch.ones(ob.shape, dtype=torch.bool)
    outside[:B, :N] = False
    assert bool((ob.cpu()[outside] == G.SENTINEL).all()), f"{what}: a sentinel outside [B, N] was overwritten"


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("N,K", G.ROWS_BF16_SHAPES, ids=_ids(G.ROWS_BF16_SHAPES))
def test_bf16_rows_exact(hip, device, N, K, B):
    """B = 3 runs the NB = 4 kernel with a repeated last row that must not be stored."""
    c = G.bf16_case(N, K, B)
    w, bias = c["W"].to(device), c["bias"].to(device)
    for dtype in (torch.float32, torch.bfloat16):
        x, r, ob = _rows_layout(c, B, N, K, dtype, device)
        hip.gemv_rows(x, w, ob[:B, :N], bias=bias, residual=r)
        _check_rows(c, ob, B, N, dtype, f"gemv_rows B={B} {N}x{K} {dtype}")


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("N,K", G.ROWS_FP8_SHAPES, ids=_ids(G.ROWS_FP8_SHAPES))
def test_fp8_rows_exact(hip, device, N, K, B):
    """(7, 1424): <2, 8>; (8197, 64): <4, 4> with the clamped rows of the last row group."""
    c = G.fp8_case(N, K, B)
    wq, sc, bias = c["Wq"].to(device), c["scale"].to(device), c["bias"].to(device)
    for dtype in (torch.float32, torch.bfloat16):
        x, r, ob = _rows_layout(c, B, N, K, dtype, device)
        hip.gemv_fp8_rows(x, wq, sc, ob[:B, :N], bias=bias, residual=r)
        _check_rows(c, ob, B, N, dtype, f"gemv_fp8_rows B={B} {N}x{K} {dtype}")


# ----------------------------------------------------------------------------- 6b. the fused RMSNorm prologue, exactly
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_fused_rmsnorm_stages_an_exact_row(hip, device, kind):
    """gv_stage_x_rmsnorm<false> on gemv_exact.norm_operands: x = +-c, integer norm weights, so the staged row is
    sign * norm_w whatever rsqrtf's last bit and the output equals float64 bit for bit.  (6, 4104) / (6, 8208): 513 / 1026
    x-chunks, the loop path (more than 512 chunks) that no tolerance test runs with a norm."""
    N, K = G.BF16_NORM_SHAPE if kind == "bf16" else G.FP8_NORM_SHAPE
    c = G.bf16_norm_case(N, K) if kind == "bf16" else G.fp8_norm_case(N, K)
    x, nw = c["x"][0].to(device), c["norm_w"].to(device)
    bias, r = c["bias"].to(device), c["R"][0].to(device)
    for dtype in (torch.float32, torch.bfloat16):
        for full in (False, True):
            kw = dict(bias=bias, residual=r) if full else {}
            want = _expect((c["ref_br"] if full else c["ref"])[0], dtype)
            y = _sentinel((N,), dtype, device)
            if kind == "bf16":
                hip.gemv(x, c["W"].to(device), y, norm_w=nw, eps=G.NORM_EPS, **kw)
            else:
                hip.gemv_fp8(x, c["Wq"].to(device), c["scale"].to(device), y, norm_w=nw, eps=G.NORM_EPS, **kw)
            _same(y, want, f"{kind} gemv with norm {N}x{K} {dtype} bias+residual={full}")


# ----------------------------------------------------------------------------- 7. ties in the fused argmax
@pytest.mark.parametrize("N,K", G.ARGMAX_SHAPES, ids=_ids(G.ARGMAX_SHAPES))
def test_argmax_ties_take_the_first_index(hip, device, N, K):
    """The exact maximum logit sits in several rows (gemv_exact.argmax_case: the two rows of a pair, two pairs of one wave,
    two waves of a workgroup, workgroups of different and of the same merging thread, the last row of an odd N).  Greedy pick
    = torch.argmax of the float64 logits (first index); a mask that clears the first j maxima moves the pick to the next."""
    c = G.argmax_case(N, K)
    x, w = c["x"].to(device), c["W"].to(device)
    ties = c["ties"]
    assert int(torch.argmax(c["logits"])) == ties[0]

    def run(allow):
        logits = _sentinel((N,), torch.float32, device)
        wv = torch.empty(2048, dtype=torch.float32, device=device)
        wi = torch.empty(2048, dtype=torch.int32, device=device)
        tokens = torch.full((8,), -1, dtype=torch.int32, device=device)
        cur = torch.full((1,), -1, dtype=torch.int32, device=device)
        step = torch.tensor([2], dtype=torch.int32, device=device)
        if allow is None:
            hip.gemv_argmax(x, w, logits, wv, wi, tokens, cur, step)
        else:
            hip.gemv_argmax_masked(x, w, logits, wv, wi, tokens, cur, step, allow.to(device))
        _same(logits, c["logits"].float(), "logits")
        assert int(step) == 3 and tokens.tolist() == [-1, -1, int(cur)] + [-1] * 5
        return int(cur)

    assert run(None) == ties[0], "unmasked pick"
    for j in range(len(ties)):
        assert run(G.allow_mask(N, ties[:j])) == ties[j], f"pick with the first {j} maxima masked ({c['labels'][j]})"


# ----------------------------------------------------------------------------- 8. argument checks launch nothing
def test_argument_errors_launch_nothing(hip, device):
    """Every rejected call raises HipLibraryError (VIS_ERR_ARG from the host checks) and leaves the sentinel-filled output as
    it was; B = 0 and B = 5 are refused by the Python wrapper before the library is reached."""
    E = hip.HipLibraryError
    outs = []

    def out(shape, dtype=torch.bfloat16):
        outs.append(_sentinel(shape, dtype, device))
        return outs[-1]

    def bf(*shape):
        return torch.ones(shape, dtype=torch.bfloat16, device=device)

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device=device)

    def sc(n):
        return torch.ones(n, dtype=torch.float32, device=device)

    S = hip.ACT_SWIGLU
    bad = {
        "bf16 K % 8": lambda: hip.gemv(bf(12), bf(4, 12), out(4)),
        "fp8 K % 16": lambda: hip.gemv_fp8(bf(24), u8(4, 24), sc(4), out(4)),
        "bf16 K > 30720": lambda: hip.gemv(bf(30728), bf(2, 30728), out(2)),
        "fp8 K > 30720": lambda: hip.gemv_fp8(bf(30736), u8(2, 30736), sc(2), out(2)),
        "bf16 swiglu N % 32": lambda: hip.gemv(bf(64), bf(48, 64), out(24), act=S),
        "fp8 swiglu N % 64": lambda: hip.gemv_fp8(bf(64), u8(96, 64), sc(96), out(48), act=S),
        "bf16 swiglu + bias": lambda: hip.gemv(bf(64), bf(64, 64), out(32), bias=bf(64), act=S),
        "bf16 swiglu + residual": lambda: hip.gemv(bf(64), bf(64, 64), out(32), residual=bf(32), act=S),
        "bf16 swiglu f32 out": lambda: hip.gemv(bf(64), bf(64, 64), out(32, torch.float32), act=S),
        "fp8 swiglu + bias": lambda: hip.gemv_fp8(bf(64), u8(64, 64), sc(64), out(32), bias=bf(64), act=S),
        "fp8 swiglu + residual": lambda: hip.gemv_fp8(bf(64), u8(64, 64), sc(64), out(32), residual=bf(32), act=S),
        "fp8 swiglu f32 out": lambda: hip.gemv_fp8(bf(64), u8(64, 64), sc(64), out(32, torch.float32), act=S),
        "bf16 misaligned x": lambda: hip.gemv(bf(68)[4:], bf(4, 64), out(4)),
        "bf16 misaligned W": lambda: hip.gemv(bf(64), bf(4 * 64 + 4)[4:].view(4, 64), out(4)),
        "fp8 misaligned x": lambda: hip.gemv_fp8(bf(68)[4:], u8(4, 64), sc(4), out(4)),
        "fp8 misaligned W": lambda: hip.gemv_fp8(bf(64), u8(4 * 64 + 8)[8:].view(4, 64), sc(4), out(4)),
        "bf16 rows ldx < K": lambda: hip.gemv_rows(bf(2, 64).as_strided((2, 64), (56, 1)), bf(16, 64), out((2, 16))),
        "fp8 rows ldx < K": lambda: hip.gemv_fp8_rows(bf(2, 64).as_strided((2, 64), (56, 1)), u8(16, 64), sc(16), out((2, 16))),
        "bf16 rows ldy < N": lambda: hip.gemv_rows(bf(2, 64), bf(16, 64), out((2, 16)).as_strided((2, 16), (8, 1))),
        "fp8 rows ldy < N": lambda: hip.gemv_fp8_rows(bf(2, 64), u8(16, 64), sc(16), out((2, 16)).as_strided((2, 16), (8, 1))),
    }
    for what, call in bad.items():
        hip.call_trace_start()
        with pytest.raises(E, match="status 1"):
            call()
        assert sum(n for n, _ in hip.call_trace_stop().values()) == 1, f"{what}: the library's own check must refuse it"
    for B in (0, 5):
        for call in (lambda: hip.gemv_rows(bf(B, 64), bf(16, 64), out((B, 16))),
                     lambda: hip.gemv_fp8_rows(bf(B, 64), u8(16, 64), sc(16), out((B, 16)))):
            hip.call_trace_start()
            with pytest.raises(E):
                call()
            assert not hip.call_trace_stop(), f"B = {B} must be refused before the library is reached"
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == G.SENTINEL).all()), "a rejected call wrote to its output"
    # and the same calls with sound arguments run
    y = out((2, 16), torch.float32)
    hip.gemv_rows(bf(2, 64), bf(16, 64), y)
    assert bool((y == 64.0).all())
    hip.gemv_fp8_rows(bf(2, 64), u8(16, 64), sc(16), y)
    assert bool((y == 0.0).all())
