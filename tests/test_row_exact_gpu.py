"""Interval-exact tests of the row-pass kernels between the GEMMs: vis_rmsnorm_bf16, vis_layernorm_bf16,
vis_rmsnorm_heads_bf16, vis_splitk_finalize_norm (csrc/norm.hip), vis_quant_rows_fp8 with and without a fused norm
(csrc/gemm_fp8.hip), vis_qkv_rope_split and vis_qkv_rope_split_many (csrc/rope.hip).

Inputs and float64 references come from tests/row_exact.py; tests/test_row_exact.py shows without a GPU that the intervals
reject subtly wrong norms and that every case stays under the 2 % ambiguity cap (re-asserted here).  Every input and output
lives in a larger sentinel-filled buffer with a row stride different from its width; the sentinels must survive bit for bit.
"""
import numpy as np
import pytest
import torch

import row_exact as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def _in_interval(got, lo, hi, what):
    """lo <= got <= hi elementwise on the decoded values (exact wherever lo == hi), under the ambiguity cap."""
    assert X.ambiguous_share(lo, hi) <= X.AMBIGUOUS_CAP, f"{what}: case over the ambiguity cap"
    bad = X.outside(got, lo, hi)
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their interval, first at {i}: got "
                             f"{got[i].item()!r}, allowed [{lo[i].item()!r}, {hi[i].item()!r}]")


def _emb_out(rows, cols, ld, dtype=torch.bfloat16):
    return X.Emb(X.blank((rows, cols), dtype), ld)


# ----------------------------------------------------------------------------- 1: rmsnorm / layernorm
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("N,rows", [(N, r) for N in X.NORM_N for r in X.NORM_ROWS])
def test_norm_interval(hip, device, N, rows, ln):
    x, w, b = X.norm_inputs(N, rows)
    xe, ye = X.Emb(x, N + 8), _emb_out(rows, N, N + 16)
    x_flat = xe.flat.to(device)
    wd, bd = w.to(device), b.to(device)
    kinds = X.row_kinds(rows)
    for eps in X.NORM_EPS:
        y_flat = ye.flat.to(device)
        if ln:
            hip.layernorm(xe.view(x_flat), wd, bd, eps, out=ye.view(y_flat))
        else:
            hip.rmsnorm(xe.view(x_flat), wd, eps, out=ye.view(y_flat))
        got = ye.view(y_flat.cpu()).double()
        lo, hi = X.norm_interval(x, w, b if ln else None, eps, X.chunks(N))
        _in_interval(got, lo, hi, f"{'layernorm' if ln else 'rmsnorm'} N={N} rows={rows} eps={eps} ({kinds})")
        z = kinds.index("zero")
        assert torch.equal(got[z], b.double() if ln else torch.zeros(N, dtype=torch.float64))
        assert X.sentinels_intact(ye, y_flat), "the kernel wrote outside y"
    assert torch.equal(X.raw(x_flat.cpu()), X.raw(xe.flat))


@pytest.mark.parametrize("N", [5128, 12])
def test_norm_rejects(hip, device, N):
    x = torch.zeros((3, N), dtype=torch.bfloat16, device=device)
    w = torch.ones(N, dtype=torch.bfloat16, device=device)
    ye = _emb_out(3, N, N)
    y_flat = ye.flat.to(device)
    with pytest.raises(hip.HipLibraryError, match="vis_rmsnorm_bf16 failed with status 1 "):
        hip.rmsnorm(x, w, 1e-6, out=ye.view(y_flat))
    with pytest.raises(hip.HipLibraryError, match="vis_layernorm_bf16 failed with status 1 "):
        hip.layernorm(x, w, w, 1e-6, out=ye.view(y_flat))
    torch.cuda.synchronize()
    assert torch.equal(X.raw(y_flat.cpu()), X.raw(ye.flat))


# ----------------------------------------------------------------------------- 2: rmsnorm_heads
@pytest.mark.parametrize("extra", [0, 128])
@pytest.mark.parametrize("tokens", [1, 5])
@pytest.mark.parametrize("heads", [1, 3, 4, 5, 8])
def test_rmsnorm_heads_interval(hip, device, heads, tokens, extra):
    x, w = X.heads_inputs(tokens, heads, extra)
    width = heads * 128
    lo, hi = X.norm_interval(x[:, :width].reshape(tokens * heads, 128), w, None, 1e-6, X.chunks(128, "heads"))
    xe = X.Emb(x, width + extra + 8)
    wd = w.to(device)
    for inplace in (True, False):
        x_flat = xe.flat.to(device)
        oe = xe if inplace else _emb_out(tokens, width + extra, width + extra + 24)
        o_flat = x_flat if inplace else oe.flat.to(device)
        hip.rmsnorm_heads(xe.view(x_flat), wd, heads, 1e-6, out=None if inplace else oe.view(o_flat))
        out = oe.view(o_flat.cpu())
        _in_interval(out[:, :width].double().reshape(tokens * heads, 128), lo, hi,
                     f"rmsnorm_heads heads={heads} tokens={tokens} extra={extra} inplace={inplace}")
        # everything but the head columns is bit-unchanged: the extra columns, the sentinels, and (with `out`) all of x
        keep = oe.outside()
        oe.view(keep)[:, width:] = True
        assert torch.equal(X.raw(o_flat.cpu())[keep], X.raw(oe.flat)[keep])
        if not inplace:
            assert torch.equal(X.raw(x_flat.cpu()), X.raw(xe.flat))


# ----------------------------------------------------------------------------- 3: splitk_finalize_norm
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("ks", X.FIN_KS)
@pytest.mark.parametrize("N", X.FIN_N)
def test_splitk_finalize_norm(hip, device, N, ks, ln):
    """Synthetic partials: x_out bit-equal to the f32 additions in their fixed order, y_out inside the interval of the
    rounded x_out.  (bias, residual aliasing x_out, y), (no bias, a separate residual, y) and (bias, aliased, no y)."""
    part, bias, R, w, b = X.finalize_inputs(N, ks)
    M = X.FIN_M
    work = part.reshape(-1).to(device)
    wd, bd, bias_d = w.to(device), (b.to(device) if ln else None), bias.to(device)
    re_ = X.Emb(R, N + 24)
    for use_bias, alias, with_y in ((True, True, True), (False, False, True), (True, True, False)):
        want_x = X.finalize_x(part, bias if use_bias else None, R)
        xe = X.Emb(R, N + 8) if alias else _emb_out(M, N, N + 8)
        x_flat = xe.flat.to(device)
        r_flat = x_flat if alias else re_.flat.to(device)
        ye = _emb_out(M, N, N + 16)
        y_flat = ye.flat.to(device)
        hip.splitk_finalize_norm(work, ks, xe.view(x_flat), bias=bias_d if use_bias else None,
                                 residual=(xe if alias else re_).view(r_flat), norm_w=wd if with_y else None,
                                 norm_b=bd if with_y else None, y_out=ye.view(y_flat) if with_y else None, eps=1e-6)
        what = f"finalize_norm N={N} ks={ks} ln={ln} bias={use_bias} alias={alias} y={with_y}"
        assert torch.equal(X.raw(xe.view(x_flat.cpu())), X.raw(want_x)), f"{what}: x_out differs from the f32 sum"
        assert X.sentinels_intact(xe, x_flat), f"{what}: wrote outside x_out"
        if not alias:
            assert torch.equal(X.raw(r_flat.cpu()), X.raw(re_.flat))
        if with_y:
            lo, hi = X.norm_interval(want_x, w, b if ln else None, 1e-6, X.chunks(N, "finalize"))
            _in_interval(ye.view(y_flat.cpu()).double(), lo, hi, what)
            assert X.sentinels_intact(ye, y_flat), f"{what}: wrote outside y_out"
        else:
            assert torch.equal(X.raw(y_flat.cpu()), X.raw(ye.flat))
    assert torch.equal(work.cpu(), part.reshape(-1))


# ----------------------------------------------------------------------------- 4: quant_rows_fp8 without a norm
def _scale_buf(M, device):
    flat = torch.full((M + 2,), float("nan"), dtype=torch.float32, device=device)
    return flat, flat[1:M + 1]


@pytest.mark.parametrize("K", X.QUANT_K, ids=lambda K: f"{K}-{X.quant_kernel(K)}")
def test_quant_rows_exact(hip, device, K):
    x, pos = X.quant_inputs(K)
    M = x.shape[0]
    want_q, want_sc = X.quant_expect(x)
    xe, qe = X.Emb(x, K + 8), _emb_out(M, K, K + 16, torch.uint8)
    x_flat, q_flat = xe.flat.to(device), qe.flat.to(device)
    s_flat, sc = _scale_buf(M, device)
    hip.quant_rows_fp8(xe.view(x_flat), q=qe.view(q_flat), scale=sc)
    got_q, got_sc = qe.view(q_flat.cpu()), sc.cpu().numpy()
    three = np.float32(3.0) / np.float32(448.0)
    for r, p in enumerate(pos):
        if p >= 0:
            assert got_sc[r].view(np.int32) == three.view(np.int32), f"K={K} row {r} (plant at {p}): scale {got_sc[r]!r}"
            assert float(X.e4m3_value(got_q)[r, p]) == (448.0 if r % 2 == 0 else -448.0), f"K={K} row {r}: planted byte"
    z = pos.index(-1)
    assert got_sc[z].view(np.int32) == np.float32(1e-12).view(np.int32) and int(got_q[z].max()) == 0
    assert np.array_equal(got_sc.view(np.int32), want_sc.view(np.int32)), f"K={K}: scales differ"
    bad = got_q != want_q
    assert not bool(bad.any()), f"K={K}: {int(bad.sum())} bytes differ, first at {torch.nonzero(bad)[0].tolist()}"
    assert X.sentinels_intact(qe, q_flat), f"K={K}: wrote outside q"
    nan = s_flat.cpu()
    assert bool(torch.isnan(nan[0])) and bool(torch.isnan(nan[-1]))
    assert torch.equal(X.raw(x_flat.cpu()), X.raw(xe.flat))


# ----------------------------------------------------------------------------- 5 + 6: quant_rows_fp8 with a fused norm
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("K", X.FUSED_K)
def test_quant_rows_fused_interval(hip, device, K, ln):
    for rows in X.NORM_ROWS:
        x, w, b = X.norm_inputs(K, rows)
        xe, qe = X.Emb(x, K + 8), _emb_out(rows, K, K + 16, torch.uint8)
        x_flat = xe.flat.to(device)
        wd, bd = w.to(device), (b.to(device) if ln else None)
        for eps in X.NORM_EPS:
            q_flat = qe.flat.to(device)
            s_flat, sc = _scale_buf(rows, device)
            hip.quant_rows_fp8(xe.view(x_flat), q=qe.view(q_flat), scale=sc, norm_w=wd, norm_b=bd, eps=eps)
            got_sc = sc.cpu().numpy()
            lo, hi = X.norm_interval(x, w, b if ln else None, eps, X.chunks(K, "quant"))
            what = f"fused {'layernorm' if ln else 'rmsnorm'} quantiser K={K} rows={rows} eps={eps}"
            s_lo, s_hi = X.fused_scale_interval(lo, hi)
            ok = (s_lo <= got_sc) & (got_sc <= s_hi)
            assert bool(ok.all()), f"{what}: scale of row {int(np.argmin(ok))} = {got_sc[np.argmin(ok)]!r} outside " \
                                   f"[{s_lo[np.argmin(ok)]!r}, {s_hi[np.argmin(ok)]!r}]"
            if not ln:                                        # RMSNorm of the all-zero row is exactly 0: the scale floor, bit for bit
                z = X.row_kinds(rows).index("zero")
                assert got_sc[z].view(np.int32) == np.float32(1e-12).view(np.int32), f"{what}: zero row scale {got_sc[z]!r}"
                assert int((qe.view(q_flat.cpu())[z] & 0x7F).max()) == 0      # (0 * a negative weight is -0: byte 0x80)
            blo, bhi = X.fused_byte_interval(lo, hi, got_sc)
            _in_interval(X.e4m3_value(qe.view(q_flat.cpu())), blo, bhi, what)
            assert X.sentinels_intact(qe, q_flat), f"{what}: wrote outside q"


def test_quant_rows_fused_rejects_long_rows(hip, device):
    x = torch.zeros((2, 4104), dtype=torch.bfloat16, device=device)
    w = torch.ones(4104, dtype=torch.bfloat16, device=device)
    q = X.blank((2, 4104), torch.uint8).to(device)
    with pytest.raises(hip.HipLibraryError, match="vis_quant_rows_fp8 failed with status 1 "):
        hip.quant_rows_fp8(x, q=q, norm_w=w)
    torch.cuda.synchronize()
    assert int(q.min()) == X.FILL_U8 == int(q.max())


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("K", X.FUSED_K)
def test_quant_rows_fused_equals_unfused(hip, device, K, ln):
    """The fused norm writes "exactly the bf16 values vis_rmsnorm_bf16 / vis_layernorm_bf16 would have written": the same
    bytes and the same scale bits as quantising the norm kernel's output."""
    for rows in X.NORM_ROWS:
        x, w, b = (t.to(device) for t in X.norm_inputs(K, rows))
        for eps in X.NORM_EPS:
            q1, s1 = hip.quant_rows_fp8(x, norm_w=w, norm_b=b if ln else None, eps=eps)
            y = hip.layernorm(x, w, b, eps) if ln else hip.rmsnorm(x, w, eps)
            q2, s2 = hip.quant_rows_fp8(y)
            what = f"K={K} rows={rows} eps={eps} ln={ln}"
            assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)), \
                f"{what}: scale bits differ on rows {torch.nonzero(s1 != s2).flatten().tolist()}"
            bad = q1 != q2
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} bytes differ, first at {torch.nonzero(bad)[0].tolist()}"


# ----------------------------------------------------------------------------- 7: qkv_rope_split
def _eq(got, want, what):
    """Value equality of a written region against the exact float64 expectation."""
    got = got.double().cpu()
    bad = ~(got == want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} wrong, first at {torch.nonzero(bad)[0].tolist()}: " \
                                f"got {got[tuple(torch.nonzero(bad)[0].tolist())].item()!r}"


def _untouched(t, what):
    assert bool((X.raw(t) == X.raw(X.blank((1,)))[0]).all()), f"{what}: sentinel overwritten"


def _check_rope(case, hip, exp, q, k, v, vt, what, interval=False):
    S, p0, c0 = case.S, case.k_pos0, case.vt_col0
    for name, t in (("q", q), ("k", None if k is None else k[:, p0:p0 + S])):
        if t is None:
            continue
        if interval:
            _in_interval(t.double().cpu(), *exp[name], f"{what} {name}")
        else:
            _eq(t, exp[name], f"{what} {name}")
    for name, t in (("k", k), ("v", v)):
        if t is not None:
            _untouched(t[:, :p0].cpu(), f"{what} {name} rows before k_pos0")
            _untouched(t[:, p0 + S:].cpu(), f"{what} {name} rows after the block")
    if v is not None:
        _eq(v[:, p0:p0 + S], exp["v"], f"{what} v")
    if vt is not None:
        w64 = (S + 63) // 64 * 64
        assert torch.equal(hip.vt_key_order(w64).cpu(), X.vt_key_order(w64))
        _eq(vt[:, :, c0:c0 + w64], exp["vt"], f"{what} vt")                 # pad columns up to round_up(S, 64): zero
        _untouched(vt[:, :, :c0].cpu(), f"{what} vt columns before vt_col0")
        _untouched(vt[:, :, c0 + w64:].cpu(), f"{what} vt columns beyond round_up(S, 64)")


def _run_rope(hip, device, case, qkv, cos, sin):
    S, HD, Hq, Hkv = case.S, case.HD, case.Hq, case.Hkv
    qe = X.Emb(qkv, case.width + case.ld_pad)
    qkv_flat = qe.flat.to(device)
    # sentinel-filled outputs: q inside a flat buffer with 64-element margins, k / v with rows around [k_pos0, k_pos0 + S),
    # vt with columns around [vt_col0, vt_col0 + round_up(S, 64))
    T, ld = case.k_pos0 + S + 2, case.vt_col0 + (S + 63) // 64 * 64 + 64
    q_flat = X.blank((128 + Hq * S * HD,)).to(device) if Hq else None
    q = q_flat[64:64 + Hq * S * HD].view(Hq, S, HD) if Hq else None
    k = X.blank((Hkv, T, HD)).to(device) if Hkv else None
    v = X.blank((Hkv, T, HD)).to(device) if Hkv and case.v else None
    vt = X.blank((Hkv, HD, ld)).to(device) if Hkv and case.vt else None
    hip.qkv_rope_split(qe.view(qkv_flat), None if cos is None else cos.to(device), None if sin is None else sin.to(device),
                       q, k, v, vt, Hq, Hkv, HD, k_pos0=case.k_pos0, vt_col0=case.vt_col0)
    if Hq:
        _untouched(q_flat[:64].cpu(), f"{case.id} before q")
        _untouched(q_flat[64 + Hq * S * HD:].cpu(), f"{case.id} after q")
    assert torch.equal(X.raw(qkv_flat.cpu()), X.raw(qe.flat))
    return q, k, v, vt


@pytest.mark.parametrize("case", X.ROPE_CASES, ids=lambda c: c.id)
def test_rope_split_exact(hip, device, case):
    qkv, cos, sin, exp = X.rope_build(case)
    q, k, v, vt = _run_rope(hip, device, case, qkv, cos, sin)
    _check_rope(case, hip, exp, q, k, v, vt, case.id)
    if not case.rot:                                          # a pure head split: the input bits
        x = qkv.reshape(case.S, -1, case.HD).permute(1, 0, 2)
        if q is not None:
            assert torch.equal(X.raw(q.cpu()), X.raw(x[:case.Hq].contiguous()))
        assert torch.equal(X.raw(k[:, case.k_pos0:case.k_pos0 + case.S].cpu()), X.raw(x[case.Hq:case.Hq + case.Hkv].contiguous()))


@pytest.mark.parametrize("case", X.ROPE_GENERAL, ids=lambda c: c.id)
def test_rope_split_general_angles(hip, device, case):
    qkv, cos, sin = X.rope_inputs(case)
    exp = X.rope_expect(case, qkv, cos, sin, slack=2.0 ** -22)
    q, k, v, vt = _run_rope(hip, device, case, qkv, cos, sin)
    _check_rope(case, hip, exp, q, k, v, vt, case.id, interval=True)


# ----------------------------------------------------------------------------- 8: qkv_rope_split_many
@pytest.mark.parametrize("HD,S,nreq,Hq,Hkv", X.MANY_CASES)
def test_rope_split_many_exact(hip, device, HD, S, nreq, Hq, Hkv):
    case = X.Rope(HD, S, Hq, Hkv, ld_pad=64, k_pos0=3, vt_col0=64)
    T, w64 = case.k_pos0 + S + 2, (S + 63) // 64 * 64
    ld = case.vt_col0 + w64 + 64
    qkv_all, cos, sin = X.rope_inputs(case, rows=nreq * S)
    qe = X.Emb(qkv_all, case.width + 64)
    qkv_flat = qe.flat.to(device)
    q_flat = X.blank((128 + nreq * Hq * S * HD,)).to(device)
    q = q_flat[64:64 + nreq * Hq * S * HD].view(nreq, Hq, S, HD)
    slot, gap = Hkv * T * HD, 40
    order = {1: [0], 3: [1, 2, 0], 8: [2, 7, 4, 1, 6, 3, 0, 5]}[nreq]        # request r lives in cache slot order[r]
    assert sorted(order) == list(range(nreq)) and (nreq < 3 or order not in (sorted(order), sorted(order, reverse=True)))
    kv_off = [gap + o * (slot + gap) for o in order]
    k_base = X.blank((gap + nreq * (slot + gap),)).to(device)
    v_base = X.blank((gap + nreq * (slot + gap),)).to(device)
    vt_all = X.blank((nreq, Hkv * HD * ld + 72)).to(device)
    vt = vt_all[:, :Hkv * HD * ld].view(nreq, Hkv, HD, ld)
    hip.qkv_rope_split_many(qe.view(qkv_flat), cos.to(device), sin.to(device), q, k_base, v_base, vt, Hq, Hkv, HD, kv_off, T,
                            k_pos0=case.k_pos0, vt_col0=case.vt_col0)
    written = torch.zeros(k_base.numel(), dtype=torch.bool)
    for r in range(nreq):
        exp = X.rope_expect(case, qkv_all[r * S:(r + 1) * S], cos, sin)
        k = k_base[kv_off[r]:kv_off[r] + slot].view(Hkv, T, HD)
        v = v_base[kv_off[r]:kv_off[r] + slot].view(Hkv, T, HD)
        _check_rope(case, hip, exp, q[r], k, v, vt[r], f"many nreq={nreq} request {r}")
        written[kv_off[r]:kv_off[r] + slot] = True
    for base in (k_base, v_base):                                            # the gaps between the slots
        _untouched(base.cpu()[~written], "cache gap")
    _untouched(vt_all[:, Hkv * HD * ld:].cpu(), "between the requests' vt")
    _untouched(q_flat[:64].cpu(), "before q")
    _untouched(q_flat[64 + nreq * Hq * S * HD:].cpu(), "after q")


def test_rope_split_many_rejects(hip, device):
    HD, S, Hq, Hkv, T = 128, 17, 2, 1, 20
    mk = lambda *s: X.blank(s).to(device)
    cos = torch.ones((S, HD), dtype=torch.float32, device=device)
    k_base, v_base = mk(10 * T * HD), mk(10 * T * HD)

    def run(offs):
        n = len(offs)
        qkv = torch.zeros((n * S, (Hq + 2 * Hkv) * HD), dtype=torch.bfloat16, device=device)
        hip.qkv_rope_split_many(qkv, cos, cos, mk(n, Hq, S, HD), k_base, v_base, mk(n, Hkv, HD, 64), Hq, Hkv, HD, offs, T)
    with pytest.raises(hip.HipLibraryError, match="requests per launch"):
        run([i * T * HD for i in range(9)])
    with pytest.raises(hip.HipLibraryError, match="multiples of 8"):
        run([0, T * HD + 4])                                  # even, but not the multiple of 8 (16 bytes) a cache slot starts at
    with pytest.raises(hip.HipLibraryError, match="multiples of 8"):
        run([0, T * HD + 1])                                  # odd
    torch.cuda.synchronize()
    _untouched(k_base.cpu(), "k after rejected calls")
    _untouched(v_base.cpu(), "v after rejected calls")
    run([T * HD, 0])                                          # the same call with sound offsets is accepted: only they were refused
    torch.cuda.synchronize()
    assert all(float(k_base[o:o + S * HD].float().abs().max()) == 0.0 for o in (0, T * HD))      # written: 0, no sentinel
