"""The batched decode projection in both forms (vis_decode_proj_bf16 / _fp8, stream-K: csrc/decode_stream.hip;
vis_decode_proj_colpar_bf16 / _fp8, column-parallel: csrc/decode_colpar.hip; the shared ds_epilogue) against float64 on
operands for which f32 sums are exact in any order (tests/decode_proj_exact.py).  Every comparison is bit for bit except the
three tolerances derived there (one bf16 ulp for silu_fast, gamma(31) for ssq_out, the rs bound).  The MX bytes of
RESID_NORMW are mx_quant of the float64 reference's y * nw; those of SWIGLU are mx_quant of the act the same launch wrote
(act itself is compared with float64 to one bf16 ulp, so no reference row predicts its bytes).

Every call uses padded operands (lda = K + 64 / + 128 with NaN behind the row, ldw likewise up to N = 1024, ldr = N + 24,
ldas = K / 32 + 4 with a scale byte in the padding that would change the sum) and outputs that are row slices of taller, wider
sentinel buffers: nothing outside the defined region may change.  The stream-K workspace's block area is filled with 0xFF
bytes (f32 NaN) before every launch - a gather that reads a block nobody wrote in this launch shows as NaN - the counters are
zero before and after, and a second launch on the same workspace, not refilled, is bitwise equal.  Where both forms cover a
shape they run the same operands and must agree bit for bit.

Stream-K shapes (bf16 K; fp8 doubles K so that nk is the same) and what each reaches - asserted on the restated geometry in
tests/test_decode_proj_exact.py:
  (128, 64)       one tile, one K-step: pre = nsteps = 1, total < 4
  (128, 256)      one range of 4 steps, nothing cut, the ring is never refilled
  (128, 1280)     one tile cut in ns = 5: at 33..64 rows two gather rounds, the second partial (GRP = 4)
  (128, 4096)     ns = 16, the maximum: one / two / four gather rounds for MB = 1 / 2 / 4
  (128, 6400)     ds_geometry halves wg down to 16: spb = 7 (= DEPTH for MB <= 2, DEPTH + 1 for MB = 4), ns = 15, lcm clipped
  (384, 640)      seams inside tiles, two tiles per range, ns = 3, lcm = 20 < total
  (256, 704)      ns = 3 and 4 in one launch, lcm clipped
  (1000, 192)     ragged N (N % 128 = 104, N % 32 != 0): clamped weight rows, live[j]; PLAIN, stream-K only
  (6144, 128)     uncut tiles, two per range (sole-owner path only)
  (262272, 64)    9 tiles per range: the overflow path for every MB (NSEG = 8 / 6), uncut; B in {4, 17, 33}
  (262272, 192)   spb = 25, 8..9 tiles per range: overflow path with tiles cut mid-range (ns = 2), tickets through set
                  NSEG - 1; B in {17, 64}; PLAIN with f32 output
  (3584, 18944)   the long-K projection (ns = 9..10); B in {4, 64}; RESID_NORMW
Column-parallel N (K-steps: 1 and one below / at / above the ring depth of every unit count in the launch;
decode_proj_exact.colpar_nks):
  32 one workgroup, one unit (B > 32: the narrow form alone) . 512 sixteen one-unit workgroups . 9600 cnt 2 and 1 (narrow
  next to non-narrow at B > 32) . 19200 cnt 3 and 2 . 35200 cnt 5 and 4 (wave 0's second unit) . 40960 every workgroup cnt = 5
"""
import pytest
import torch

import decode_proj_exact as D
import gemv_exact as G
from oracle import mx_ref

pytestmark = pytest.mark.gpu
PLAIN, SWIGLU, RESID = D.PLAIN, D.SWIGLU, D.RESID


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _same(got, want, what):
    if got.dtype != want.dtype or not torch.equal(got, want):
        bad = torch.nonzero((got != want).flatten() | (got != got).flatten()).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} wrong, first at {i}: got {float(got.flatten()[i])!r} "
                             f"want {float(want.flatten()[i])!r} (last wrong {int(bad[-1])})")


def _covered(hip, N, mode, mx):
    return bool(hip.load().vis_decode_proj_colpar_covers(N, mode, 1 if mx else 0))


class Ops:
    """Device operands of one case at B rows, padded as the module docstring says."""

    def __init__(self, hip, dev, c, B):
        self.hip, self.dev, self.c, self.B = hip, dev, c, B
        self.fp8 = c["kind"] == "fp8"
        N, K = c["N"], c["K"]
        self.N, self.K = N, K
        pad = 128 if self.fp8 else 64
        x, w = (c["xq"], c["Wq"]) if self.fp8 else (c["x"], c["W"])
        self.x = G.padded(x[:B], pad).to(dev)[:, :K]
        self.W = (G.padded(w, pad).to(dev)[:, :K]) if N <= 1024 else w.to(dev)
        if self.fp8:
            self.xs = D.padded_scales(c["xs"][:B]).to(dev)[:, :K // 32]
            self.sw = c["sw"].to(dev)
        self.bias = c["bias"].to(dev) if "bias" in c else None
        self.R = D.residual_buffer(c["R"], B).to(dev)[:B, :N] if "R" in c else None
        self.nw = c["nw"].to(dev) if "nw" in c else None
        self.ws = None

    def workspace(self):
        if self.ws is None:
            self.ws = self.hip.decode_proj_ws(self.dev, self.B, self.N, self.K, fp8=self.fp8)
            g = D.streamk_geometry(self.N, self.K, self.fp8)
            assert self.ws.numel() == g["ws_bytes"][D.rows_of(self.B)], "restated workspace size"
        return self.ws

    def launch(self, form, mode, dtype=torch.bfloat16, bias=False, norm=None, want=("out",), what=""):
        """One call (and its repeat) with sentinel buffers; returns the defined regions on the CPU."""
        hip, dev, B, N = self.hip, self.dev, self.B, self.N
        n_out = N // 2 if mode == SWIGLU else N
        bufs, views = {}, {}

        def buf(name, shape, dt, region):
            bufs[name] = torch.full(shape, G.SENTINEL, dtype=dt, device=dev)
            views[name] = bufs[name][region]

        if "out" in want:
            buf("out", (B + 2, n_out + 16), dtype, (slice(0, B), slice(0, n_out)))
        if "out_w" in want:
            buf("out_w", (B + 2, n_out + 16), torch.bfloat16, (slice(0, B), slice(0, n_out)))
        if "q" in want:
            buf("out_q", (B + 2, n_out + 32), torch.uint8, (slice(0, B), slice(0, n_out)))
            buf("out_qs", (B + 2, n_out // 32 + 4), torch.uint8, (slice(0, B), slice(0, n_out // 32)))
        units = (N + 31) // 32
        if mode == RESID:
            buf("ssq_out", (units + 2, 64), torch.float32, (slice(0, units), slice(0, B)))
        kw = dict(out=views.get("out"), out_w=views.get("out_w"), out_q=views.get("out_q"), out_qs=views.get("out_qs"),
                  bias=self.bias if bias else None, residual=self.R if mode == RESID else None,
                  norm_w=self.nw if mode == RESID else None, ssq_out=bufs.get("ssq_out"), form=form)
        if norm is not None:
            big = norm["big"].clone()
            big[:, B:] = float("nan")
            kw.update(ssq_in=big.to(dev)[:norm["tiles_in"]], norm_dim=norm["norm_dim"], eps=norm["eps"])
        ws = self.workspace() if form == "streamk" else None
        self.last_bufs = bufs

        def once():
            if ws is not None:
                assert int(ws[:D.CNT_BYTES].view(torch.int32).abs().sum()) == 0, "counters must be zero before a launch"
            if self.fp8:
                hip.decode_proj_fp8(self.x, self.xs, self.W, self.sw, ws, mode, **kw)
            else:
                hip.decode_proj(self.x, self.W, ws, mode, **kw)
            torch.cuda.synchronize()
            if ws is not None:
                assert int(ws[:D.CNT_BYTES].view(torch.int32).abs().sum()) == 0, f"{what}: counters not back at zero"
            return {k: v.clone() for k, v in bufs.items()}

        if ws is not None:
            ws[D.CNT_BYTES:].fill_(0xFF)
        first = once()
        second = once()                                    # same workspace, not refilled
        out = {}
        for name, full in first.items():
            assert torch.equal(full.view(torch.uint8), second[name].view(torch.uint8)), f"{what}: {name} differs on the second call"
            region = (slice(0, units), slice(0, B)) if name == "ssq_out" else \
                (slice(0, B), slice(0, n_out // 32 if name == "out_qs" else n_out))
            out[name] = full[region].cpu()
            full[region] = G.SENTINEL                      # (a clone: what is left must be the sentinel everywhere)
            assert bool((full == G.SENTINEL).all()), f"{what}: {name} written outside its region"
        return out


def _forms(hip, N, mode, mx=False, only=None):
    forms = ["streamk"] + (["colpar"] if _covered(hip, N, mode, mx) else [])
    return [f for f in forms if only is None or f == only]


def _both(ops, forms, mode, what, **kw):
    """The call in every form; the forms must agree bit for bit.  Returns the first form's outputs."""
    res = [ops.launch(f, mode, what=f"{what} {f}", **kw) for f in forms]
    for f, r in zip(forms[1:], res[1:]):
        for name in r:
            assert torch.equal(r[name].view(torch.uint8), res[0][name].view(torch.uint8)), \
                f"{what}: {name} differs between {forms[0]} and {f}"
    return res[0]


def _as(t, dtype):
    return t.float() if dtype == torch.float32 else t.float().to(torch.bfloat16)


def check_plain(ops, forms, what, tiles_in):
    c, B = ops.c, ops.B
    acc, biasd = c["acc"][:B], c["bias"].double()
    for dtype in (torch.float32, torch.bfloat16):
        for bias in (False, True):
            r = _both(ops, forms, PLAIN, f"{what} plain {dtype} bias={bias}", dtype=dtype, bias=bias)
            _same(r["out"], _as(acc + biasd[None, :] if bias else acc, dtype), f"{what} plain {dtype} bias={bias}")
    check_norm(ops, forms, what, D.norm_case(tiles_in))


def check_norm(ops, forms, what, nc, report=None):
    """Deferred norm: (a) one f32 factor per row explains every element, (b) it is within the bound of float64."""
    c, B = ops.c, ops.B
    acc, biasd = c["acc"][:B], c["bias"].double()
    r = _both(ops, forms, PLAIN, f"{what} rs f32", dtype=torch.float32, norm=nc)
    col = c["nstar"]
    rb = (r["out"][:, col].double() / acc[:, col]).float()
    assert bool(torch.isfinite(rb).all()) and torch.equal(rb.double() * acc[:, col], r["out"][:, col].double())
    _same(r["out"], D.scaled_candidates(acc, rb, None)[0], f"{what} rs tiles_in={nc['tiles_in']}: one factor per row")
    rel = (rb.double() / nc["r64"][:B] - 1).abs()
    if report is not None:
        report.append(float(rel.max()))
    print(f"{what} tiles_in={nc['tiles_in']} B={B}: worst relative error of rs {float(rel.max()):.3e}")
    assert float(rel.max()) <= D.RS_REL_BOUND, f"{what}: rs off by {float(rel.max()):.3e} (row {int(rel.argmax())})"
    for dtype, bias in ((torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)):
        o = _both(ops, forms, PLAIN, f"{what} rs {dtype} bias={bias}", dtype=dtype, bias=bias, norm=nc)["out"]
        cands = [_as(t, dtype) for t in D.scaled_candidates(acc, rb, biasd if bias else None)]
        ok = torch.zeros(o.shape, dtype=torch.bool)
        for t in cands:
            ok |= o == t
        assert bool(ok.all()), f"{what} rs {dtype} bias={bias}: {int((~ok).sum())} elements are neither rounding of acc * rs + bias"


def check_resid(ops, forms, what):
    c, B = ops.c, ops.B
    r = _both(ops, forms, RESID, f"{what} resid", want=("out", "out_w"))
    _same(r["out"], c["y"][:B], f"{what} y")
    _same(r["out_w"], c["yw"][:B], f"{what} y * nw")
    ref = D.ssq_ref(c["y"], B)
    err = (r["ssq_out"].double() - ref).abs()
    assert bool((err <= D.ssq_tolerance(ref)).all()), f"{what} ssq_out: worst {float((err / ref.clamp_min(1e-30)).max()):.3e} relative"
    # the engine's fp8 configuration: out + the MX copy of y * nw, no out_w
    q_ref, s_ref = mx_ref.mx_quant(c["yw"][:B].float())
    m = _both(ops, forms, RESID, f"{what} resid mx", want=("out", "q"))
    _same(m["out"], c["y"][:B], f"{what} y (MX call)")
    _same(m["out_qs"], s_ref, f"{what} E8M0 scales of y * nw")
    _same(m["out_q"], q_ref, f"{what} e4m3 codes of y * nw")
    assert torch.equal(m["ssq_out"], r["ssq_out"])


def check_swiglu(hip, dev, kind, N, K, B, what, only=None):
    c = D.swiglu_case(kind, N, K)
    ops = Ops(hip, dev, c, B)
    forms = _forms(hip, N, SWIGLU, only=only)
    r = _both(ops, forms, SWIGLU, f"{what} swiglu")
    ref = c["ref"][:B]
    got = r["out"].double()
    want = ref.to(torch.bfloat16).double()
    bad = (got - want).abs() > G.swiglu_tolerance(ref)
    if bool(bad.any()):
        b, o = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what} swiglu: {int(bad.sum())} outputs off by more than 1 bf16 ulp, first [{b}, {o}]: got "
                             f"{float(got[b, o])!r} want {float(want[b, o])!r} (gate {float(c['gate'][b, o])}, up {float(c['up'][b, o])})")
    assert bool((got[c["gate"][:B] == 0] == 0).all())
    if "colpar" in forms:                                  # with an MX output the column-parallel form refuses
        with pytest.raises(hip.HipLibraryError, match="status 3"):
            ops.launch("colpar", SWIGLU, want=("out", "q"), what=f"{what} swiglu mx colpar")
        torch.cuda.synchronize()
        assert all(bool((b == G.SENTINEL).all()) for b in ops.last_bufs.values()), "the refused call wrote to an output"
    if only in (None, "streamk"):
        m = ops.launch("streamk", SWIGLU, want=("out", "q"), what=f"{what} swiglu mx")
        _same(m["out"], r["out"], f"{what} act (MX call)")
        # act is known only to one bf16 ulp (silu_fast), so no float64 row predicts these bytes: the reference is mx_quant of
        # the act this launch wrote, which was just asserted equal to the act checked against float64 above
        q_ref, s_ref = mx_ref.mx_quant(r["out"].float())
        _same(m["out_qs"], s_ref, f"{what} E8M0 scales of act")
        _same(m["out_q"], q_ref, f"{what} e4m3 codes of act")
        e = ops.launch("streamk", SWIGLU, want=("q",), what=f"{what} swiglu mx only")       # the engine's fp8 gate/up call
        _same(e["out_q"], m["out_q"], f"{what} codes without out")
        _same(e["out_qs"], m["out_qs"], f"{what} scales without out")


def run_shape(hip, dev, kind, N, K, B, modes, what, idx=0):
    if modes in ("all", "plain", "plain_f32", "resid"):
        c = D.case(kind, N, K)
        ops = Ops(hip, dev, c, B)
        if modes == "plain_f32":
            r = _both(ops, _forms(hip, N, PLAIN), PLAIN, f"{what} plain f32", dtype=torch.float32)
            _same(r["out"], c["acc"][:B].float(), f"{what} plain f32")
        if modes in ("all", "plain"):
            check_plain(ops, _forms(hip, N, PLAIN), what, D.TILES_IN[(idx + B) % len(D.TILES_IN)])
        if modes in ("all", "resid") and N % 32 == 0:
            check_resid(ops, _forms(hip, N, RESID, mx=True), what)
    if modes == "all" and N % 64 == 0:
        check_swiglu(hip, dev, kind, N, K, B, what)


STREAMK_CASES = [pytest.param(kind, N, K * (2 if kind == "fp8" else 1), B, modes, i, id=f"{kind}-{N}x{K}-{what}-B{B}")
                 for kind in ("bf16", "fp8") for i, (N, K, Bs, modes, what) in enumerate(D.STREAMK_SHAPES) for B in Bs]


@pytest.mark.parametrize("kind,N,K,B,modes,idx", STREAMK_CASES)
def test_streamk_shapes(hip, device, kind, N, K, B, modes, idx):
    run_shape(hip, device, kind, N, K, B, modes, f"{kind} {N}x{K} B={B}", idx)


def _colpar_cases():
    """One test per (N, K-steps, B), ordered so that the tests of one (N, K) follow each other and share its operands."""
    out = []
    for kind in ("bf16", "fp8"):
        for N, what in D.COLPAR_N:
            todo = [(nk, B, i) for B in D.BATCHES for i, nk in enumerate(D.colpar_nks(N, B, kind == "fp8"))]
            out += [pytest.param(kind, N, nk, B, i, id=f"{kind}-N{N}-{what}-nk{nk}-B{B}") for nk, B, i in sorted(todo)]
    return out


@pytest.mark.parametrize("kind,N,nk,B,idx", _colpar_cases())
def test_colpar_shapes(hip, device, kind, N, nk, B, idx):
    K = nk * (128 if kind == "fp8" else 64)
    run_shape(hip, device, kind, N, K, B, "all", f"{kind} {N}x{K} (nk={nk}) B={B}", idx)


# ----------------------------------------------------------------------------- the deferred norm factor
@pytest.mark.parametrize("tiles_in", D.TILES_IN)
def test_deferred_norm(hip, device, tiles_in):
    """ssq_in = big[:tiles_in] of a taller NaN-filled tensor, NaN in columns >= B: a read past tiles_in, or of another row's
    column, is a NaN.  Prints the worst relative error of rs (the figure RS_MEASURED_REL records)."""
    worst = []
    for kind, N, K in (("bf16", 384, 640), ("fp8", 384, 1280)):
        c = D.case(kind, N, K)
        for B in (1, 17, 64):
            check_norm(Ops(hip, device, c, B), _forms(hip, N, PLAIN), f"{kind} {N}x{K} B={B}", D.norm_case(tiles_in), worst)
    print(f"tiles_in={tiles_in}: worst relative error of rs over all rows {max(worst):.3e} (bound {D.RS_REL_BOUND:.3e})")


# ----------------------------------------------------------------------------- fp8: codes, scales, the scale-to-block map
def _fp8_call(hip, dev, form, xq, xs, wq, sw, B, N):
    c = dict(kind="fp8", N=N, K=xq.shape[1], xq=xq, xs=xs, Wq=wq, sw=sw)
    return Ops(hip, dev, c, B).launch(form, PLAIN, dtype=torch.float32, what=f"fp8 sweep {form}")["out"]


@pytest.mark.parametrize("form", ["streamk", "colpar"])
def test_fp8_every_code_and_scale(hip, device, form):
    """Every finite e4m3 code once as a weight (x = 1.0, scale byte 127) and once as an activation (one-hot weight rows,
    block scales 2^-16 .. 2^16 over the rows and blocks), and the unit activation under each of those scales; f32 output,
    compared exactly (values: the -0 code sums to +0)."""
    codes = torch.tensor(G.E4M3_FINITE, dtype=torch.uint8)
    one = 0x38
    assert float(G.E4M3[one]) == 1.0
    # weights: row n holds code n in column n % 128
    N, K, B = 256, 128, 3
    wq = torch.zeros((N, K), dtype=torch.uint8)
    wq[torch.arange(254), torch.arange(254) % K] = codes
    got = _fp8_call(hip, device, form, torch.full((B, K), one, dtype=torch.uint8), torch.full((B, K // 32), 127, dtype=torch.uint8),
                    wq, torch.ones(N), B, N)
    _same(got.double(), G.E4M3[wq.long()].sum(1)[None, :].expand(B, N).contiguous(), "weight codes")
    # activations: x[b, k] = code (k + 7 b) % 254, W = identity (code 1.0), scale byte 111 + (b + block) % 33
    N, K, B = 256, 256, 33
    k, b = torch.arange(K)[None, :], torch.arange(B)[:, None]
    xq = torch.where(k < 254, codes[(k + 7 * b) % 254], torch.zeros((), dtype=torch.uint8))
    xs = (111 + (b + torch.arange(K // 32)[None, :]) % 33).to(torch.uint8)
    assert set(xs.flatten().tolist()) == set(range(111, 144))
    eye = torch.zeros((N, K), dtype=torch.uint8)
    eye[torch.arange(N), torch.arange(K)] = one
    sw = G.fp8_scales(N).float()
    scale = torch.ldexp(torch.ones((B, K), dtype=torch.float64), (xs.long() - 127).repeat_interleave(32, 1))
    got = _fp8_call(hip, device, form, xq, xs, eye, sw, B, N)
    _same(got.double(), G._exact_f32(G.E4M3[xq.long()] * scale * sw.double()[None, :], "code * scale * sw"), "activation codes")
    got = _fp8_call(hip, device, form, torch.full((B, K), one, dtype=torch.uint8), xs, eye, sw, B, N)
    _same(got.double(), scale * sw.double()[None, :], "unit activation under every scale")


@pytest.mark.parametrize("form", ["streamk", "colpar"])
@pytest.mark.parametrize("B", [1, 17, 64])
def test_fp8_scale_to_block_mapping(hip, device, form, B):
    """One K-step whose four blocks carry four different scales; identity weights (a one-hot in each of the 4 blocks x 2
    halves of the lane layout, and everywhere else): out[b, n] = code * 2^(s - 127) * sw[n] exactly."""
    c = D.case("fp8", 128, 128)
    assert all(len(set(row.tolist())) == 4 for row in c["xs"])
    eye = torch.zeros((128, 128), dtype=torch.uint8)
    eye[torch.arange(128), torch.arange(128)] = 0x38
    scale = torch.ldexp(torch.ones((64, 128), dtype=torch.float64), (c["xs"].long() - 127).repeat_interleave(32, 1))
    want = G._exact_f32(G.E4M3[c["xq"].long()] * scale * c["sw"].double()[None, :], "code * scale * sw")[:B]
    got = _fp8_call(hip, device, form, c["xq"], c["xs"], eye, c["sw"], B, 128)
    _same(got.double(), want, "identity weights")


# ----------------------------------------------------------------------------- argument checks launch nothing
def test_argument_checks_launch_nothing(hip, device):
    """Every rejected call is refused by the library's own checks (one library call, status 1; status 3 for the shapes
    the column-parallel form does not cover) and leaves the sentinel outputs as they were.  A row stride shorter than its row
    (ldc, ldr, ldcq, ldcqs) would let the epilogue write into the next row and past the last one: ds_check_common refuses it."""
    E = hip.HipLibraryError
    dev = device
    outs = []

    def out(B, n, dtype=torch.bfloat16, ld=None):
        outs.append(torch.full((B + 1, n + 16), G.SENTINEL, dtype=dtype, device=dev))
        return outs[-1][:B, :n] if ld is None else outs[-1].flatten().as_strided((B, n), (ld, 1))

    def bf(*shape):
        return torch.ones(shape, dtype=torch.bfloat16, device=dev)

    def u8(*shape, v=0):
        return torch.full(shape, v, dtype=torch.uint8, device=dev)

    def f32(*shape):
        return torch.ones(shape, dtype=torch.float32, device=dev)

    B, N, K = 4, 512, 256
    ws = hip.decode_proj_ws(dev, B, 40992, K)
    ws8 = hip.decode_proj_ws(dev, B, N, K, fp8=True)
    res = dict(residual=bf(B, N), norm_w=bf(N))
    bad = {}
    for form in ("streamk", "colpar"):
        w = ws if form == "streamk" else None
        w8 = ws8 if form == "streamk" else None
        bad.update({
            f"{form} ldc < N": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K), bf(N, K), w, PLAIN, out=out(B, N, ld=N - 8), form=form)),
            f"{form} ldc < N, out_w": (1, lambda w=w, form=form: hip.decode_proj(
                bf(B, K), bf(N, K), w, RESID, out=out(B, N, ld=N - 8), out_w=out(B, N, ld=N - 8), ssq_out=f32(N // 32, 64), form=form, **res)),
            f"{form} ldc < N / 2, swiglu": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K), bf(N, K), w, SWIGLU, out=out(B, N // 2, ld=N // 2 - 8), form=form)),
            f"{form} ldr < N": (1, lambda w=w, form=form: hip.decode_proj(
                bf(B, K), bf(N, K), w, RESID, out=out(B, N), ssq_out=f32(N // 32, 64), form=form, norm_w=bf(N),
                residual=bf(B, N).as_strided((B, N), (N - 8, 1)))),
            f"{form} ldcq < N": (1, lambda w=w, form=form: hip.decode_proj(
                bf(B, K), bf(N, K), w, RESID, out=out(B, N), out_q=out(B, N, torch.uint8, ld=N - 8), out_qs=out(B, N // 32, torch.uint8),
                ssq_out=f32(N // 32, 64), form=form, **res)),
            f"{form} ldcqs < N / 32": (1, lambda w=w, form=form: hip.decode_proj(
                bf(B, K), bf(N, K), w, RESID, out=out(B, N), out_q=out(B, N, torch.uint8), out_qs=out(B, N // 32, torch.uint8, ld=N // 32 - 1),
                ssq_out=f32(N // 32, 64), form=form, **res)),
            f"{form} lda < K": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K).as_strided((B, K), (K - 8, 1)), bf(N, K), w, PLAIN, out=out(B, N), form=form)),
            f"{form} misaligned x": (1, lambda w=w, form=form: hip.decode_proj(bf(B * K + 4)[4:].view(B, K), bf(N, K), w, PLAIN, out=out(B, N), form=form)),
            f"{form} N % 4": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K), bf(510, K), w, PLAIN, out=out(B, 510), form=form)),
            f"{form} swiglu N % 64": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K), bf(96, K), w, SWIGLU, out=out(B, 48), form=form)),
            f"{form} resid without ssq_out": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K), bf(N, K), w, RESID, out=out(B, N), form=form, **res)),
            f"{form} tiles_in = 129": (1, lambda w=w, form=form: hip.decode_proj(bf(B, K), bf(N, K), w, PLAIN, out=out(B, N), ssq_in=f32(129, 64),
                                                                              norm_dim=4128, form=form)),
            f"{form} fp8 ldas < K / 32": (1, lambda w8=w8, form=form: hip.decode_proj_fp8(
                u8(B, K), u8(B, K // 32, v=127).as_strided((B, K // 32), (4, 1)), u8(N, K), f32(N), w8, PLAIN, out=out(B, N), form=form)),
        })
    w = ws                                                 # SWIGLU with an MX output: the stream-K form alone
    bad["streamk ldcq < N / 2, swiglu"] = (1, lambda: hip.decode_proj(
        bf(B, K), bf(N, K), w, SWIGLU, out_q=out(B, N // 2, torch.uint8, ld=N // 2 - 8), out_qs=out(B, N // 64, torch.uint8), form="streamk"))
    bad["streamk ldcqs < N / 64, swiglu"] = (1, lambda: hip.decode_proj(
        bf(B, K), bf(N, K), w, SWIGLU, out_q=out(B, N // 2, torch.uint8), out_qs=out(B, N // 64, torch.uint8, ld=N // 64 - 1), form="streamk"))
    bad["colpar N = 40992"] = (3, lambda: hip.decode_proj(bf(B, 64), bf(40992, 64), None, PLAIN, out=out(B, 40992), form="colpar"))
    for what, (status, call) in bad.items():
        hip.call_trace_start()
        with pytest.raises(E, match=f"status {status}"):
            call()
        # (the stream-K wrapper asks vis_decode_proj_ws_bytes, a host function, before the entry point)
        assert sum(n for n, _ in hip.call_trace_stop().values()) == (2 if what.startswith("streamk") else 1), \
            f"{what}: the library's own check must refuse it"
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == G.SENTINEL).all()), "a rejected call wrote to its output"
    # and the same call with sound arguments runs, on either form
    for form in ("streamk", "colpar"):
        y = out(B, N, torch.float32)
        hip.decode_proj(bf(B, K), bf(N, K), ws if form == "streamk" else None, PLAIN, out=y, form=form)
        assert bool((y == float(K)).all())
