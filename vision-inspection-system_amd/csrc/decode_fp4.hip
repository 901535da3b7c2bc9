// vis_gemv_mxfp4w / vis_gemv_mxfp4w_rows: the decode GEMV on OCP Microscaling FP4 weights ("W4A16").
//   y = act(sum_k deq(Wq, Ws)[n][k] * bf16(x[k]) + bias) + R,  f32 accumulation
//   Wq uint8 [N][ldq]: byte j of a row = E2M1 codes of elements 2j (low nibble) and 2j+1 (high nibble)
//   Ws uint8 [N][lds]: one E8M0 byte b per 32 consecutive K-elements of a row, X = 2^(b-127); no row scale
// Structure of vis_gemv_fp8w (decode.hip): x in LDS as bf16 with the optional fused RMSNorm prologue, weights streamed
// exactly once with non-temporal 16-byte loads, two register sets in flight.  A 16-byte load is now exactly one MX block
// (32 weights), so ONE scale byte travels with it: v_cvt_scalef32_pk_bf16_fp4 turns a byte (two codes) times the block
// scale into an EXACT bf16 pair (E2M1 has one mantissa bit; scale bytes 3..250 keep every product a normal bf16), which
// feeds the same v_dot2c_f32_bf16.  Algorithmic bytes per launch: N*K/2 (codes) + N*K/32 (scales).
//
// LDS: a lane now reads the 64 bytes of x that go with its block as four ds_read_b128 at a 64-byte lane stride.  Laid out
// linearly that is a 4-way bank conflict (a ds_read_b128 serves 16 lanes per cycle from one 256-byte bank row; lanes l and
// l+4 of a group would hit the same 16-byte slot).  So x is staged SWIZZLED (gv_slot<true>): 16-byte piece j of block c
// sits at piece j ^ ((c >> 2) & 3) - the 16 lanes of every group then cover the 16 slots of the bank row once.
//
// Task shape <ROWS, SEG> (ROWS weight rows x SEG blocks per lane per register set), chosen by the launcher:
//   <8, 2>  short rows, many of them (K <= 4096: at most 2 blocks per lane; gate/up, lm_head)
//   <2, 2>  short rows, few of them (qkv, o: one row pair per wave keeps ~7 waves per CU)
//   <2, 5>  long rows (down: K = 18944 = 9.25 blocks per lane -> two segments of 5)
#include "decode_common.hip.h"

struct GemvF4Args {
  const bf16_t* x;
  const uint8_t* W;
  const uint8_t* S;
  const bf16_t* bias;
  const bf16_t* R;
  const bf16_t* norm_w;
  void* y;
  int N, K, ldq, lds;
  int act, out_f32;
  float eps;
  int nb, ldx, ldy, ldr;   // vis_gemv_mxfp4w_rows: as in GemvArgs
};

template <int ROWS, int SEG>
struct G4Buf {
  u32x4 w[ROWS][SEG];
  uint32_t s[ROWS][SEG];   // the block's E8M0 byte
};

template <int ROWS>
__device__ __forceinline__ void g4_rows(const GemvF4Args& p, bool swiglu, int grp, int* r) {
  if (swiglu) {  // ROWS/2 consecutive outputs of one 16-group: gate rows r[0], r[2], ..., up rows r[1], r[3], ...
    const int o = (ROWS / 2) * grp;
    const int g0 = ((o >> 4) << 5) + (o & 15);
#pragma unroll
    for (int i = 0; i < ROWS / 2; ++i) { r[2 * i] = g0 + i; r[2 * i + 1] = g0 + 16 + i; }
  } else {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) r[i] = min(ROWS * grp + i, p.N - 1);
  }
}

template <int ROWS, int SEG>
__device__ __forceinline__ void g4_load(G4Buf<ROWS, SEG>& b, const GemvF4Args& p, bool swiglu, int grp, int seg, int lane,
                                        int nch) {
  int r[ROWS];
  g4_rows<ROWS>(p, swiglu, grp, r);
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const uint8_t* w = p.W + (size_t)r[i] * p.ldq;
    const uint8_t* s = p.S + (size_t)r[i] * p.lds;
#pragma unroll
    for (int u = 0; u < SEG; ++u) {
      const int c = min(lane + 64 * (seg * SEG + u), nch - 1);  // unconditional, clamped (see gv_load)
      b.w[i][u] = __builtin_nontemporal_load((const u32x4*)(w + (size_t)c * 16));
      b.s[i][u] = __builtin_nontemporal_load(s + c);             // 64 consecutive bytes per wave
    }
  }
}

// the 32 weights of a block as sixteen EXACT bf16 pairs (converted once, used for every input row):
// word i of w holds elements 8i..8i+7, its byte b the elements 8i+2b (low nibble) and 8i+2b+1 (high nibble)
struct G4x32 {
  bf16x2 v[16];
};
__device__ __forceinline__ G4x32 cvt32_f4(const u32x4& w, float scale) {
  G4x32 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r.v[4 * i] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[i], scale, 0);
    r.v[4 * i + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[i], scale, 1);
    r.v[4 * i + 2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[i], scale, 2);
    r.v[4 * i + 3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[i], scale, 3);
  }
  return r;
}
// x[j] = elements 8j..8j+7 of the block
__device__ __forceinline__ float dot32_f4(const G4x32& w, const u32x4 (&x)[4], float acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x8 xv = __builtin_bit_cast(bf16x8, x[j]);
    acc = __builtin_amdgcn_fdot2_f32_bf16(w.v[4 * j], __builtin_shufflevector(xv, xv, 0, 1), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(w.v[4 * j + 1], __builtin_shufflevector(xv, xv, 2, 3), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(w.v[4 * j + 2], __builtin_shufflevector(xv, xv, 4, 5), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(w.v[4 * j + 3], __builtin_shufflevector(xv, xv, 6, 7), acc, false);
  }
  return acc;
}

template <int ROWS, int SEG, int NB>
__device__ __forceinline__ void g4_consume(const G4Buf<ROWS, SEG>& b, const bf16_t* xs, int K, int seg, int lane, int nch,
                                           float (&a)[NB][ROWS]) {
#pragma unroll
  for (int u = 0; u < SEG; ++u) {
    const int c = lane + 64 * (seg * SEG + u);
    const int cc = min(c, nch - 1);
    const int rot = (cc >> 2) & 3;   // the staging swizzle of this block (gv_slot<true>)
    u32x4 xv[NB][4];
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xv[r][j] = *(const u32x4*)(xs + (size_t)r * K + cc * 32 + ((j ^ rot) << 3));
        if (c >= nch) xv[r][j] = (u32x4){0u, 0u, 0u, 0u};  // clamped duplicate block contributes nothing
      }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const G4x32 wv = cvt32_f4(b.w[i][u], __builtin_bit_cast(float, b.s[i][u] << 23));   // 2^(byte - 127)
#pragma unroll
      for (int r = 0; r < NB; ++r) a[r][i] = dot32_f4(wv, xv[r], a[r][i]);
    }
  }
}

template <int ROWS, int NB>
__device__ __forceinline__ void g4_finish(const GemvF4Args& p, bool swiglu, int grp, int lane, float (&a)[NB][ROWS]) {
#pragma unroll
  for (int r = 0; r < NB; ++r)
#pragma unroll
    for (int i = 0; i < ROWS; ++i) a[r][i] = wave_sum(a[r][i]);
  if (lane != 0) return;
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    if (r >= p.nb) break;
    if (swiglu) {
#pragma unroll
      for (int i = 0; i < ROWS / 2; ++i)
        ((bf16_t*)p.y)[(size_t)r * p.ldy + (ROWS / 2) * grp + i] = f2bf(silu_fast(a[r][2 * i]) * a[r][2 * i + 1]);
      continue;
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int o = ROWS * grp + i;
      if (o >= p.N) break;
      float v = a[r][i];
      if (p.bias) v += bf2f(p.bias[o]);
      if (p.R) v += bf2f(p.R[(size_t)r * p.ldr + o]);
      if (p.out_f32) ((float*)p.y)[(size_t)r * p.ldy + o] = v;
      else ((bf16_t*)p.y)[(size_t)r * p.ldy + o] = f2bf(v);
    }
  }
}

template <int ROWS, int SEG, int NB>
__global__ __launch_bounds__(256) void gemv_mxfp4w_kernel(GemvF4Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = (bf16_t*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch8 = p.K >> 3;   // 16-byte chunks of x (bf16)
  const int nch = p.K >> 5;    // 16-byte chunks of a weight row = MX blocks
  const bool swiglu = (p.act == GV_ACT_SWIGLU);
  const int n_out = swiglu ? (p.N >> 1) : p.N;
  const int n_grps = swiglu ? (n_out / (ROWS / 2)) : ((n_out + ROWS - 1) / ROWS);
  const int n_waves = gridDim.x * 4;
  const int wid = blockIdx.x * 4 + wave;
  const int g_begin = (int)((long long)n_grps * wid / n_waves);
  const int g_end = (int)((long long)n_grps * (wid + 1) / n_waves);
  const int nseg = ((nch + 63) / 64 + SEG - 1) / SEG;
  const int n_tasks = (g_end - g_begin) * nseg;

  G4Buf<ROWS, SEG> A, B;
  if (n_tasks > 0) g4_load(A, p, swiglu, g_begin, 0, lane, nch);  // in flight while x is staged

#pragma unroll
  for (int r = 0; r < NB; ++r) {
    if (r > 0) __syncthreads();   // the norm's reduction scratch is reused
    gv_stage_row<true>(p.x + (size_t)min(r, p.nb - 1) * p.ldx, p.norm_w, xs + (size_t)r * p.K, nch8, p.K, p.eps, tid, lane,
                       wave);
  }
  __syncthreads();

  float acc[NB][ROWS];
#pragma unroll
  for (int r = 0; r < NB; ++r)
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[r][i] = 0.f;
  int grp = g_begin, seg = 0;
  for (int t = 0; t < n_tasks; t += 2) {
    int grp1 = grp, seg1 = seg + 1;
    if (seg1 == nseg) { seg1 = 0; ++grp1; }
    if (t + 1 < n_tasks) g4_load(B, p, swiglu, grp1, seg1, lane, nch);
    g4_consume<ROWS, SEG, NB>(A, xs, p.K, seg, lane, nch, acc);
    if (seg == nseg - 1) {
      g4_finish<ROWS, NB>(p, swiglu, grp, lane, acc);
#pragma unroll
      for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int i = 0; i < ROWS; ++i) acc[r][i] = 0.f;
    }
    if (t + 1 >= n_tasks) break;
    int grp2 = grp1, seg2 = seg1 + 1;
    if (seg2 == nseg) { seg2 = 0; ++grp2; }
    if (t + 2 < n_tasks) g4_load(A, p, swiglu, grp2, seg2, lane, nch);
    g4_consume<ROWS, SEG, NB>(B, xs, p.K, seg1, lane, nch, acc);
    if (seg1 == nseg - 1) {
      g4_finish<ROWS, NB>(p, swiglu, grp1, lane, acc);
#pragma unroll
      for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int i = 0; i < ROWS; ++i) acc[r][i] = 0.f;
    }
    grp = grp2;
    seg = seg2;
  }
}

template <int ROWS, int SEG>
static int gemv_mxfp4w_launch_shape(const GemvF4Args& p, int n_out, hipStream_t stream) {
  const int n_grps = (p.act == GV_ACT_SWIGLU) ? n_out / (ROWS / 2) : (n_out + ROWS - 1) / ROWS;
  int blocks = (n_grps + 3) / 4;   // one row group per wave until ~4096 waves, then several per wave
  if (blocks > 1024) blocks = 1024 + (blocks - 1024) / 8;
  if (blocks > 2048) blocks = 2048;
  vis_clear_error();
  const dim3 g(blocks), b(256);
  if (p.nb == 1) {
    hipLaunchKernelGGL((gemv_mxfp4w_kernel<ROWS, SEG, 1>), g, b, (size_t)p.K * 2, stream, p);
    return vis_check_launch();
  }
  static const bool attr_ok = [] {
    return hipFuncSetAttribute((const void*)gemv_mxfp4w_kernel<ROWS, SEG, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, GV_ROWS_LDS_MAX) == hipSuccess &&
           hipFuncSetAttribute((const void*)gemv_mxfp4w_kernel<ROWS, SEG, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, GV_ROWS_LDS_MAX) == hipSuccess;
  }();
  if (!attr_ok) return VIS_ERR_LAUNCH;
  if (p.nb == 2) hipLaunchKernelGGL((gemv_mxfp4w_kernel<ROWS, SEG, 2>), g, b, (size_t)p.K * 4, stream, p);
  else hipLaunchKernelGGL((gemv_mxfp4w_kernel<ROWS, SEG, 4>), g, b, (size_t)p.K * 8, stream, p);
  return vis_check_launch();
}

static int gemv_mxfp4w_launch(const GemvF4Args& p, hipStream_t stream) {
  const int n_out = (p.act == GV_ACT_SWIGLU) ? p.N / 2 : p.N;
  if (p.K > 4096) return gemv_mxfp4w_launch_shape<2, 5>(p, n_out, stream);
  if (n_out <= 8192) return gemv_mxfp4w_launch_shape<2, 2>(p, n_out, stream);
  return gemv_mxfp4w_launch_shape<8, 2>(p, n_out, stream);
}

// checks shared by both entry points (nbk = input rows the kernel instance stages: 1, 2 or 4)
static int gemv_mxfp4w_args_ok(const void* x, const void* Wq, const void* Ws, const void* bias, const void* R,
                               const void* norm_w, const void* y, int N, int K, int ldq, int lds, int act, int out_f32,
                               int nbk) {
  if (!x || !Wq || !Ws || !y || N <= 0 || K <= 0) return 0;
  if (K % 32 != 0 || ldq % 16 != 0 || ldq < K / 2 || lds < K / 32) return 0;
  if ((size_t)K * 2 * nbk > (size_t)(nbk == 1 ? 60 * 1024 : GV_ROWS_LDS_MAX)) return 0;
  if (act != GV_ACT_NONE && act != GV_ACT_SWIGLU) return 0;
  if (act == GV_ACT_SWIGLU && (N % 64 != 0 || bias || R || out_f32)) return 0;
  if (((uintptr_t)x | (uintptr_t)Wq | (uintptr_t)norm_w) & 15) return 0;
  return 1;
}

extern "C" int vis_gemv_mxfp4w(const void* x, const void* Wq, const void* Ws, const void* bias, const void* R,
                               const void* norm_w, void* y, int N, int K, int ldq, int lds, int act, int out_f32,
                               float eps, hipStream_t stream) {
  if (!gemv_mxfp4w_args_ok(x, Wq, Ws, bias, R, norm_w, y, N, K, ldq, lds, act, out_f32, 1)) return VIS_ERR_ARG;
  GemvF4Args p;
  p.x = (const bf16_t*)x; p.W = (const uint8_t*)Wq; p.S = (const uint8_t*)Ws; p.bias = (const bf16_t*)bias;
  p.R = (const bf16_t*)R; p.norm_w = (const bf16_t*)norm_w; p.y = y;
  p.N = N; p.K = K; p.ldq = ldq; p.lds = lds; p.act = act; p.out_f32 = out_f32; p.eps = eps;
  p.nb = 1; p.ldx = 0; p.ldy = 0; p.ldr = 0;
  return gemv_mxfp4w_launch(p, stream);
}

// vis_gemv_mxfp4w for B <= 4 input rows: the codes and scales are streamed and converted once for all rows; each row's
// arithmetic is vis_gemv_mxfp4w's, so a handful of in-flight sequences decode bit-identically to one.
extern "C" int vis_gemv_mxfp4w_rows(const void* x, const void* Wq, const void* Ws, const void* bias, const void* R,
                                    const void* norm_w, void* y, int B, int N, int K, int ldq, int lds, int ldx, int ldy,
                                    int ldr, int act, int out_f32, float eps, hipStream_t stream) {
  if (B < 1 || B > 4) return VIS_ERR_ARG;
  const int nbk = (B == 1) ? 1 : (B == 2 ? 2 : 4);
  if (!gemv_mxfp4w_args_ok(x, Wq, Ws, bias, R, norm_w, y, N, K, ldq, lds, act, out_f32, nbk)) return VIS_ERR_ARG;
  if (ldx % 8 != 0 || ldx < K) return VIS_ERR_ARG;
  if (ldy < ((act == GV_ACT_SWIGLU) ? N / 2 : N) || (R && ldr < N)) return VIS_ERR_ARG;
  GemvF4Args p;
  p.x = (const bf16_t*)x; p.W = (const uint8_t*)Wq; p.S = (const uint8_t*)Ws; p.bias = (const bf16_t*)bias;
  p.R = (const bf16_t*)R; p.norm_w = (const bf16_t*)norm_w; p.y = y;
  p.N = N; p.K = K; p.ldq = ldq; p.lds = lds; p.act = act; p.out_f32 = out_f32; p.eps = eps;
  p.nb = B; p.ldx = ldx; p.ldy = ldy; p.ldr = ldr;
  return gemv_mxfp4w_launch(p, stream);   // three rows run on the four-row kernel (the fourth repeats the third, not stored)
}
