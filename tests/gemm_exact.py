"""Exact operands for the prefill GEMM tests: inputs whose every rounded value is representable, so the expected output is
known bit for bit and a wrong integer says which tile / K-step / column went wrong.

  C[M, N(/2)] = act((A W^T) (* sa[m] sw[n]) + bias) + R

* A holds integers in [-2, 2] (non-zero at ~4/5 of its k), W holds -1 / 0 / +1 with at most 120 non-zeros per row, so every
  f32 partial sum is an integer of magnitude <= 240 whatever the summation order.  bias and R are small integers.  The
  builder ASSERTS from the float64 reference that the pre-activation is exact in f32 and (no activation) that the stored
  value is exact in bf16: `ref == ref.to(bfloat16)`.
* Every row of W draws its OWN support, and the builder forces and asserts coverage (`assert_live_k`):
    K <= 2048: every k is non-zero in some row of every full 128-row block of W;
    K  > 2048: every k is non-zero somewhere in W, and every block has a non-zero in every K-step (64 wide, fp8: 128);
    ragged tail blocks (fewer than 128 rows) get the K-step form when they have the entries for it (rows * 120 >= 4 * steps).
  A skipped, repeated or swapped K-step, LDS half-tile or fragment then changes an integer in every tile.
* fp8: the same integers as e4m3 bytes, with power-of-two sa[m] (period 3) and sw[n] (period 2, and a jump every 256
  columns): a scale taken from a neighbouring row / column or from another column round is a factor of two.
* Activations: A is scaled by 1/16 (bf16) or the scales are <= 1/16 (fp8), bias is a multiple of 1/4: the pre-activation
  stays exact and |x| <= 16; the reference applies the activation in float64 and `act_tolerance` derives the bound.
* Layouts: `Emb` places a tensor in a larger NaN-filled buffer (ld > width, rows below, optional 8-byte offset).

CPU only: float64 torch, never the library under test.
"""
import dataclasses
import functools
import math

import numpy as np
import torch

KINDS = ("plain", "bias", "bias_quickgelu", "bias_gelu", "residual", "bias_residual", "swiglu", "bias_swiglu")
ACT_OF = {"plain": 0, "bias": 0, "bias_quickgelu": 1, "bias_gelu": 2, "residual": 0, "bias_residual": 0, "swiglu": 3,
          "bias_swiglu": 3}
LAYOUTS = ("packed", "padded", "offset8")   # padded: every ld > width, rows below, ldr != ldc; offset8: padded + C 8 bytes off
NAN_BF16 = 0x7FC1          # a quiet NaN with a payload bit, as int16
NAN_E4M3 = 0x7F
SUPPORT = 120


@dataclasses.dataclass(frozen=True)
class Case:
    entry: str      # "bf16" | "fp8"
    M: int
    N: int          # rows of W (SwiGLU: gate and up rows together, the output has N / 2 columns)
    K: int
    kind: str
    layout: str = "packed"

    @property
    def id(self):
        return f"{self.entry}-{self.M}x{self.N}x{self.K}-{self.kind}-{self.layout}"

    @property
    def act(self):
        return ACT_OF[self.kind]

    @property
    def n_out(self):
        return self.N // 2 if self.act == 3 else self.N

    @property
    def has_bias(self):
        return self.kind.startswith("bias")

    @property
    def has_residual(self):
        return self.kind.endswith("residual")

    @property
    def kstep(self):
        return 64 if self.entry == "bf16" else 128

    def ld(self):
        """(lda, ldw, ldc, ldr, C offset in elements) of the layout."""
        if self.layout == "packed":
            return self.K, self.K, self.n_out, self.n_out, 0
        pad_k = 64 if self.entry == "bf16" else 128     # lda % 8 (fp8: % 16) and 16-byte row starts must survive
        return self.K + pad_k, self.K + 2 * pad_k, self.n_out + 24, self.n_out + 40, 4 if self.layout == "offset8" else 0


class Emb:
    """A [rows, cols] tensor inside a flat NaN-filled buffer: element (r, c) at offset + r * ld + c, `below` rows after it."""

    def __init__(self, t, ld, below=3, offset=0, fill=None):
        rows, cols = t.shape
        assert ld >= cols
        self.rows, self.cols, self.ld, self.offset, self.below = rows, cols, ld, offset, below
        n = offset + (rows + below) * ld
        if t.dtype == torch.bfloat16:
            self.flat = torch.full((n,), NAN_BF16 if fill is None else fill, dtype=torch.int16).view(torch.bfloat16)
        else:
            assert t.dtype == torch.uint8
            self.flat = torch.full((n,), NAN_E4M3 if fill is None else fill, dtype=torch.uint8)
        self.view(self.flat).copy_(t)

    def view(self, flat):
        return flat.as_strided((self.rows, self.cols), (self.ld, 1), self.offset)

    def inside(self):
        """bool mask over the flat buffer: True inside the logical tensor."""
        m = torch.zeros(self.flat.numel(), dtype=torch.bool)
        self.view(m).fill_(True)
        return m


def canary_intact(emb, flat_after):
    """Every element of the buffer outside the logical tensor still holds the fill pattern, bit for bit."""
    bits = torch.int16 if emb.flat.dtype == torch.bfloat16 else torch.uint8
    out = ~emb.inside()
    return torch.equal(flat_after.cpu().view(bits)[out], emb.flat.view(bits)[out])


# ----------------------------------------------------------------------------- operands
def draw_w(N, K, kstep, rng):
    """W [N, K] in {-1, 0, 1}, <= 120 non-zeros per row, each row its own support, with the coverage assert_live_k checks
    forced (score -1 = taken first) rather than hoped for."""
    score = rng.random((N, K), dtype=np.float32)
    steps = K // kstep
    if K > 2048 and N * 100 >= K:                       # every k somewhere in W
        perm = rng.permutation(K)
        score[np.arange(K) % N, perm] = -1.0
    for b0 in range(0, N, 128):
        R = min(128, N - b0)
        if K <= 2048 and R == 128:                      # every k in every full block
            perm = rng.permutation(K)
            score[b0 + np.arange(K) % R, perm] = -1.0
        elif R * SUPPORT >= 4 * steps:                  # a non-zero in every K-step of the block
            ks = rng.permutation(steps)
            score[b0 + np.arange(steps) % R, ks * kstep + rng.integers(0, kstep, steps)] = -1.0
    assert int((score < 0).sum(1).max()) <= SUPPORT, "forced coverage does not fit the per-row support"
    keep = np.ones((N, K), dtype=bool)
    if K > SUPPORT:
        keep[:] = False
        np.put_along_axis(keep, np.argpartition(score, SUPPORT - 1, axis=1)[:, :SUPPORT], True, axis=1)
    sign = rng.integers(0, 2, (N, K), dtype=np.int8) * 2 - 1
    return torch.from_numpy((sign * keep).astype(np.float32))


def assert_live_k(w, kstep):
    """The coverage the module docstring promises, checked on the finished W."""
    N, K = w.shape
    nz = w != 0
    assert int(nz.sum(1).max()) <= SUPPORT
    steps = K // kstep
    if K > 2048 and N * 100 >= K:
        assert bool(nz.any(0).all()), "a k index is zero in every row of W"
    for b0 in range(0, N, 128):
        blk = nz[b0:b0 + 128]
        R = blk.shape[0]
        if K <= 2048 and R == 128:
            assert bool(blk.any(0).all()), f"block {b0}: a k index is dead"
        elif R * SUPPORT >= 4 * steps:
            assert bool(blk.any(0).view(steps, kstep).any(1).all()), f"block {b0}: a K-step is dead"


def interleave16(gate, up):
    """[I, K] x 2 -> [2 I, K], rows g0..g15, u0..u15, g16..: the layout the SwiGLU epilogue pairs (weights.interleave_gate_up)."""
    I, K = gate.shape
    return torch.stack((gate.reshape(I // 16, 16, K), up.reshape(I // 16, 16, K)), 1).reshape(2 * I, K).contiguous()


def act_f64(x, act):
    if act == 1:
        return x * torch.sigmoid(1.702 * x)
    if act == 2:
        return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x


def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (float64 tensor); the smallest normal's spacing below it."""
    e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))[1] - 1
    return torch.ldexp(torch.ones_like(ref), e - 7)


def act_tolerance(kind, pre, ref, up=None):
    """Accepted |kernel - ref| for an activation epilogue: one bf16 ulp of the reference (the kernel's f32 activation may land
    on the other side of a rounding boundary; the allowance also covers its f32 roundings) plus the absolute error the
    approximation documents in the code, nothing else:
    * x sigmoid(k x) = x * rcp(1 + exp2(-k log2e x)) with v_exp_f32 and v_rcp_f32 "1 ulp each" (common.hip.h): an ulp of
      e = exp(-k x) moves sigma by sigma (1 - sigma) 2^-23, an ulp of the reciprocal by sigma 2^-23; times |x|;
    * erf-GELU by Abramowitz-Stegun 7.1.26, |erfc error| <= 1.5e-7 (gemm_epilogue.hip.h), times |x| / 2;
    * SwiGLU: silu(g) * u - the silu bound times |u|."""
    ulp = bf16_ulp(ref)
    if kind == "bias_gelu":
        return ulp + 1.5e-7 * pre.abs() / 2
    k = 1.702 if kind == "bias_quickgelu" else 1.0
    s = torch.sigmoid(k * pre)
    err = pre.abs() * (s * (1 - s) + s) * 2.0 ** -23
    if up is not None:
        err = err * up.abs()
    return ulp + err


def expected_flat(emb, ref):
    """The whole buffer of `emb` as it must look after a launch that is exact: `ref` (rounded to bf16 - exact for the kinds
    without an activation) inside, the fill pattern everywhere else."""
    flat = emb.flat.clone()
    emb.view(flat).copy_(ref.to(torch.bfloat16))
    return flat


@functools.lru_cache(maxsize=2)
def _product(M, N, K, kstep, swiglu, seed):
    """(A integers, W, their float64 product): shared by every epilogue kind and layout of one problem."""
    rng = np.random.default_rng((seed * 1000003 + M * 31 + N * 17 + K) & 0x7FFFFFFF)
    a_int = torch.from_numpy(rng.integers(-2, 3, (M, K)).astype(np.float32))
    assert 0.7 < float((a_int != 0).float().mean()) < 0.9
    if swiglu:
        wg, wu = draw_w(N // 2, K, kstep, rng), draw_w(N // 2, K, kstep, rng)
        assert_live_k(wg, kstep)
        assert_live_k(wu, kstep)
        w = interleave16(wg, wu)
    else:
        w = draw_w(N, K, kstep, rng)
        assert_live_k(w, kstep)
    acc = a_int.double() @ w.double().t()                       # integers, |acc| <= 240
    assert float(acc.abs().max()) <= 2 * SUPPORT
    return a_int, w, acc


def build(case, seed=0):
    """Operands (CPU, in their layout) and the exact float64 reference of `case`.  Returns a dict:
    A, W, C (Emb), R (Emb or None; C's shape), bias, sa, sw (tensors or None), ref [M, n_out] float64, tol (None = exact),
    acc (the integer product) and pre (the pre-activation)."""
    M, N, K, act = case.M, case.N, case.K, case.act
    fp8 = case.entry == "fp8"
    a_int, w, acc = _product(M, N, K, case.kstep, act == 3, seed)
    rng = np.random.default_rng((seed * 7919 + M * 13 + N * 7 + K + 12345) & 0x7FFFFFFF)
    small = act != 0                                            # activation cases: |pre-activation| <= 16
    sa = sw = None
    if fp8:
        sa = torch.from_numpy(np.array([0.25, 0.5, 1.0])[np.arange(M) % 3]) * (1 / 16 if small else 1.0)
        sw = torch.from_numpy(np.array([1.0, 0.5])[np.arange(N) % 2] * np.array([1.0, 2.0, 0.5])[(np.arange(N) // 256) % 3])
        if act == 3:                                            # gate / up rows of a pair 16 apart: give them different scales
            sw = sw * torch.from_numpy(np.array([1.0, 0.5])[(np.arange(N) // 16) % 2])
        pre = acc * sa[:, None] * sw[None, :]
        a_val = a_int
    else:
        a_val = a_int / 16 if small else a_int
        pre = acc / 16 if small else acc.clone()
    bias = None
    if case.has_bias:
        bias = torch.from_numpy(rng.integers(-3, 4, N).astype(np.float64)) * (0.25 if small else 1.0)
        pre = pre + bias[None, :]
    assert torch.equal(pre, pre.float().double()), "pre-activation not exact in f32"
    up = None
    if act == 3:
        assert float(pre.abs().max()) <= 16
        g = pre.view(M, N // 32, 2, 16)
        gate, up = g[:, :, 0].reshape(M, N // 2), g[:, :, 1].reshape(M, N // 2)
        ref = gate * torch.sigmoid(gate) * up
        tol = act_tolerance(case.kind, gate, ref, up)
    elif act:
        assert float(pre.abs().max()) <= 16
        ref = act_f64(pre, act)
        tol = act_tolerance(case.kind, pre, ref)
    else:
        ref, tol = pre, None
    lda, ldw, ldc, ldr, coff = case.ld()
    r_emb = None
    if case.has_residual:
        r = torch.from_numpy(rng.integers(-3, 4, (M, case.n_out)).astype(np.float64))
        ref = ref + r
        r_emb = Emb(r.to(torch.bfloat16), ldr, offset=coff)
    if tol is None:                                             # the one value the kernel rounds to bf16 is representable
        assert torch.equal(ref, ref.to(torch.bfloat16).double()), "expected output not exact in bf16"
    if fp8:
        aq = a_val.to(torch.float8_e4m3fn)
        wq = w.to(torch.float8_e4m3fn)
        assert torch.equal(aq.float(), a_val) and torch.equal(wq.float(), w)
        A, W = Emb(aq.view(torch.uint8), lda), Emb(wq.view(torch.uint8), ldw)
    else:
        assert torch.equal(a_val.to(torch.bfloat16).float(), a_val)
        A, W = Emb(a_val.to(torch.bfloat16), lda), Emb(w.to(torch.bfloat16), ldw)
    C = Emb(torch.zeros(M, case.n_out, dtype=torch.bfloat16), ldc, offset=coff)
    C.view(C.flat.view(torch.int16)).fill_(NAN_BF16)            # the output starts as NaN too: an unwritten element shows
    return dict(A=A, W=W, C=C, R=r_emb, bias=None if bias is None else bias.to(torch.bfloat16),
                sa=None if sa is None else sa.float(), sw=None if sw is None else sw.float(),
                ref=ref, tol=tol, acc=acc, pre=pre)


def check(case, ops, c_flat, what=""):
    """The output inside `c_flat` (C's whole buffer after the launch) against the reference: bit-exact without an activation,
    within the derived bound with one; canaries around C untouched; no NaN (from operand padding) anywhere in the output."""
    got = ops["C"].view(c_flat.cpu()).double()
    assert canary_intact(ops["C"], c_flat), f"{case.id} {what}: the kernel wrote outside C"
    assert bool(torch.isfinite(got).all()), f"{case.id} {what}: NaN / unwritten output at {torch.nonzero(~torch.isfinite(got))[0].tolist()}"
    ref = ops["ref"]
    if ops["tol"] is None:
        bad = got != ref
    else:
        bad = (got - ref).abs() > ops["tol"]
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        m, n = idx[0].tolist()
        raise AssertionError(f"{case.id} {what}: {idx.shape[0]} wrong elements, rows {int(idx[:, 0].min())}..{int(idx[:, 0].max())} "
                             f"cols {int(idx[:, 1].min())}..{int(idx[:, 1].max())}; first ({m}, {n}): got {got[m, n].item()!r} "
                             f"want {ref[m, n].item()!r}")


# ----------------------------------------------------------------------------- the case table
def _cases():
    c = []
    # one base problem per kernel / plan; every epilogue kind runs on it in the packed (wide where N % 8 == 0) layout and,
    # 8 bytes off in a padded buffer, through the direct epilogue
    bases = {
        "bf16": [(100, 384, 512), (300, 512, 576), (1030, 7680, 576), (1030, 13312, 1024), (1030, 13216, 1024)],
        #        128x128          128x256 half     256x256 pp       mixed + half-tiles   mixed + 128x128 remainder
        "fp8": [(300, 512, 512), (1100, 640, 512), (1030, 7680, 1152), (1270, 13312, 1024)],
        #       128x128 (M < 1024) 128x128 by cost  256x256 pp          mixed
    }
    for entry, shapes in bases.items():
        for (M, N, K) in shapes:
            for kind in KINDS:
                if entry == "fp8" and kind == "bias_swiglu":
                    continue                                    # vis_gemm_fp8 takes no bias with SwiGLU
                c.append(Case(entry, M, N, K, kind, "packed"))
                c.append(Case(entry, M, N, K, kind, "offset8"))
    # M edges x N tails (N % 8 == 4: the direct epilogue by shape), K-tile counts odd and even, bias + residual
    for entry in ("bf16", "fp8"):
        for M, N, K in [(1, 4, 128), (127, 124, 128), (128, 132, 512), (129, 252, 1152), (255, 260, 512), (256, 132, 1152),
                        (257, 260, 1152), (257, 516, 512), (513, 772, 1152)]:
            c.append(Case(entry, M, N, K, "bias_residual", "padded"))
    for M, N, K in [(1, 4, 64), (129, 260, 576), (257, 260, 1088), (513, 772, 1088), (520, 768, 576)]:
        c.append(Case("bf16", M, N, K, "bias_residual", "padded"))
    # ragged M and N edges on the 256 x 256 ping-pong kernels, odd K-tile counts (17 / 9)
    c.append(Case("bf16", 1030, 7684, 1088, "bias_residual", "padded"))
    c.append(Case("fp8", 1030, 7684, 1152, "bias_residual", "padded"))
    # long K (the down projection's): K = 18944, M <= 600
    c.append(Case("bf16", 257, 260, 18944, "bias_residual", "padded"))
    c.append(Case("bf16", 100, 252, 18944, "residual", "packed"))
    c.append(Case("bf16", 300, 512, 18944, "plain", "packed"))
    c.append(Case("fp8", 257, 260, 18944, "bias_residual", "padded"))
    c.append(Case("fp8", 300, 512, 18944, "plain", "packed"))
    # non-temporal stores: >= 64 MB of output
    c.append(Case("bf16", 4096, 8192, 64, "bias", "packed"))
    c.append(Case("fp8", 4096, 8192, 128, "bias", "packed"))
    return c


CASES = _cases()
