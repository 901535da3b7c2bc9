// Decode-step cross-attention over fp8 (OCP e4m3) copies of the image's static keys / values (MllamaEngine cross_kv="fp8").
//
// Storage, per slot and cross layer: codes uint8 [Hkv][key_tokens][128] for K and for V, one f32 scale per (kv head, key row)
// for each, [Hkv][key_tokens].  The codes and scales are written once per prompt pass by vis_quant_rows_fp8 (no norm) over the
// bf16 rows: scale = max(amax / 448, 1e-12), code = e4m3_rne_saturating(x * (1 / scale)).  Its all-zero-row rule: amax = 0
// gives scale 1e-12 (never 0) and 128 codes 0, so a zero row dequantises to exact zeros and no scale is ever 0 or inf.
//
// vis_decode_cross_attn_fp8[_batch] follow vis_decode_cross_attn[_batch] in everything but the operand bytes: the q_norm RMS
// of the q heads (HF rounding), one workgroup per (kv head, split of 64 keys, sequence), keys [0, *nkeys_m1 + 1) with the
// count read from device memory and clamped into [.., key_tokens) before it bounds anything, the (m, l, o) partials of the
// split in the layout decode_attn_combine_body merges (reused unchanged).  A row at or past the key count is loaded (its
// address lies inside the buffers: key_tokens is a multiple of 64) but never used: its score is never read, its weight and
// its value codes are replaced by zeros with selects, so NaN codes and inf scales there change nothing.
//
// Arithmetic.  Softmax scheme: that of the split decode attention (decode_attn_split_body), NOT the prompt pass's: statistics
// per head over the split's keys in f32, p = exp2(s - m) kept in f32 - P is never rounded to bf16 - and P * V on the VALU in f32.
//   score   s_j = (kscale_j * sum_d q_d * kcode_jd) * (scale * log2 e): the codes are converted exactly to bf16 (every e4m3
//           value is a bf16 value) and the sum runs on the MFMA (v_mfma_f32_16x16x32_bf16, f32 accumulation);
//   weight  w_j = p_j * vscale_j, one f32 rounding (the V row scale folded into the softmax weight);
//   output  o_d = sum_j w_j * vcode_jd in f32, the codes converted exactly to f32; l = sum_j p_j without the scale.
//
// Loads.  A key row is 128 bytes of codes.  K: the lane that holds key (lane & 15) of its wave's 16 keys loads bytes
// [32 h, 32 h + 32) of the row (h = lane >> 4) as two 16-byte loads - the MFMA's contraction index is free as long as both
// operands agree, so q is read from LDS in the same order.  V: thread t loads the 16-byte chunk (t & 7) of rows (t >> 3) and
// (t >> 3) + 32, a wave instruction covering eight whole rows; the chunks go through LDS so that P * V reads one dword (four
// dims) per key and thread.  Scales: the four K scales a lane needs are one 16-byte load, the 64 V scales one dword per lane
// of wave 0; all of them are requested with the codes, before the key count has arrived.
#include "decode_common.hip.h"

struct XkvArgs {
  const bf16_t* q;         // [Hq * 128] of the q projection
  const bf16_t* q_norm_w;  // [128]
  const uint8_t* kq;       // [Hkv][key_tokens][128]
  const uint8_t* vq;
  const float* ksc;        // [Hkv][key_tokens]
  const float* vsc;
  const int* nkeys_m1;
  float* part_o;           // [Hq][nsplit][128]
  float* part_ml;          // [Hq][nsplit][2]
  int Hq, Hkv, key_tokens, nsplit;
  float scale_log2, eps;
  long long q_bs, kv_bs, sc_bs;   // element strides between sequences: q, codes, scales
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// four e4m3 codes of one dword -> four f32 (exact)
__device__ __forceinline__ void xkv_cvt4(uint32_t w, float* f) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0]; f[1] = lo[1]; f[2] = hi[0]; f[3] = hi[1];
}

// eight e4m3 codes (two dwords) -> eight bf16 (exact: the upper half of the f32)
__device__ __forceinline__ bf16x8 xkv_cvt8_bf16(uint32_t w0, uint32_t w1) {
  float f[8];
  xkv_cvt4(w0, f);
  xkv_cvt4(w1, f + 4);
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (__float_as_uint(f[2 * i]) >> 16) | (__float_as_uint(f[2 * i + 1]) & 0xffff0000u);
  return __builtin_bit_cast(bf16x8, r);
}

#define XKV_KEYS DA_MAXKEYS   // 64: the split of vis_decode_cross_attn

template <int G>
__global__ __launch_bounds__(256) void cross_attn_fp8_kernel(XkvArgs p) {
  constexpr int HD = 128;
  static_assert(XKV_KEYS == 64, "one key per lane in the softmax, 16 keys per wave on the MFMA");
  // rows padded by 16 bytes: at a 256-byte stride the 16 heads a lane group reads for the B operand would share their banks
  __shared__ __attribute__((aligned(16))) bf16_t q_s[16][HD + 8];   // heads >= G are zero
  __shared__ __attribute__((aligned(16))) uint32_t v_s[XKV_KEYS][HD / 4];
  __shared__ float vsc_s[XKV_KEYS];
  __shared__ float sc[G][XKV_KEYS];
  __shared__ float pw[G][XKV_KEYS];
  __shared__ float red[8][G][HD];
  __shared__ float ml[G][2];
  const int hkv = blockIdx.x, split = blockIdx.y, seq = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, h = lane >> 4;
  const int ks = split * XKV_KEYS;
  if (ks >= p.key_tokens) return;   // workgroup-uniform; key_tokens % 64 == 0: every row of a split that runs lies inside the buffers
  const size_t row0 = (size_t)hkv * p.key_tokens + ks;
  const uint8_t* Kr = p.kq + (size_t)seq * p.kv_bs + row0 * HD;
  const uint8_t* Vr = p.vq + (size_t)seq * p.kv_bs + row0 * HD;
  const float* Ks = p.ksc + (size_t)seq * p.sc_bs + row0;
  const float* Vs = p.vsc + (size_t)seq * p.sc_bs + row0;
  const bf16_t* q = p.q + (size_t)seq * p.q_bs;

  // ---- every read of the split up front (addresses do not depend on the key count)
  const u32x4 k0 = *(const u32x4*)(Kr + (size_t)(16 * wave + l15) * HD + 32 * h);
  const u32x4 k1 = *(const u32x4*)(Kr + (size_t)(16 * wave + l15) * HD + 32 * h + 16);
  const f32x4 ksc4 = *(const f32x4*)(Ks + 16 * wave + 4 * h);
  const u32x4 va = *(const u32x4*)(Vr + (size_t)tid * 16);
  const u32x4 vb = *(const u32x4*)(Vr + (size_t)(tid + 256) * 16);
  const float vsc1 = Vs[lane];

  const int slot = min(p.nkeys_m1[seq], p.key_tokens - 1);
  const int ctx = slot + 1;
  if (ks >= ctx) return;            // nothing to attend to: the combine never reads this split's partials
  const int nk = min(ks + XKV_KEYS, ctx) - ks;

  // ---- q_norm (RMSNorm over the 128 dims of each head, HF rounding), one wave per head: vis_decode_cross_attn's
  for (int g = wave; g < G; g += 4) {
    const bf16_t* qh = q + (size_t)(hkv * G + g) * HD;
    const float a = bf2f(qh[lane]), b = bf2f(qh[lane + 64]);
    const float ss = wave_sum(a * a + b * b);
    const float rstd = rsqrtf(ss * (1.0f / HD) + p.eps);
    q_s[g][lane] = f2bf(bf2f(f2bf(a * rstd)) * bf2f(p.q_norm_w[lane]));
    q_s[g][lane + 64] = f2bf(bf2f(f2bf(b * rstd)) * bf2f(p.q_norm_w[lane + 64]));
  }
  for (int it = tid; it < (16 - G) * HD; it += 256) q_s[G + it / HD][it % HD] = 0;
  *(u32x4*)(&v_s[0][0] + (size_t)tid * 4) = va;
  *(u32x4*)(&v_s[0][0] + (size_t)(tid + 256) * 4) = vb;
  if (wave == 0) vsc_s[lane] = vsc1;
  __syncthreads();

  // ---- scores on the MFMA: A = the wave's 16 keys (row = lane & 15), B = q^T; contraction index of step ds, lane group h,
  //      element j = dim 32 h + 8 ds + j in both
  if (16 * wave < nk) {   // wave-uniform
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      const u32x4 kk = (ds < 2) ? k0 : k1;
      const bf16x8 kf = xkv_cvt8_bf16(kk[2 * (ds & 1)], kk[2 * (ds & 1) + 1]);
      const bf16x8 qf = *(const bf16x8*)(&q_s[l15][32 * h + 8 * ds]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, acc, 0, 0, 0);
    }
    // acc[r] = sum_d kcode[key = 16 wave + 4 h + r][d] * q[head = l15][d]
    if (l15 < G) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[l15][16 * wave + 4 * h + r] = (acc[r] * ksc4[r]) * p.scale_log2;
    }
  }
  __syncthreads();

  // ---- per-head softmax statistics over this split (one wave per head, one key per lane); keys past the count: p = 0 by select
  for (int g = wave; g < G; g += 4) {
    const bool live = lane < nk;
    const float s = live ? sc[g][lane] : -1.0e30f;
    const float mx = wave_max(s);
    const float e = live ? exp2f(s - mx) : 0.f;
    const float ls = wave_sum(e);
    pw[g][lane] = live ? e * vsc_s[lane] : 0.f;
    if (lane == 0) { ml[g][0] = mx; ml[g][1] = ls; }
  }
  __syncthreads();

  // ---- O[g][d] += w[g][key] * vcode[key][d]: thread = (key group kg, dims 4 d4 .. 4 d4 + 3), keys kg + 8 i ascending
  const int d4 = tid & 31, kg = tid >> 5;
  float acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) { acc[g][0] = 0.f; acc[g][1] = 0.f; acc[g][2] = 0.f; acc[g][3] = 0.f; }
#pragma unroll
  for (int i = 0; i < XKV_KEYS / 8; ++i) {
    const int key = kg + 8 * i;
    uint32_t w = v_s[key][d4];
    if (key >= nk) w = 0u;          // a row past the count: code 0 = +0.0 whatever it holds, and its weight is 0
    float v[4];
    xkv_cvt4(w, v);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float pg = pw[g][key];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[g][j] += pg * v[j];
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) *(f32x4*)(&red[kg][g][4 * d4]) = (f32x4){acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
  __syncthreads();
  float* po = p.part_o + (size_t)seq * p.Hq * p.nsplit * HD;
  float* pm = p.part_ml + (size_t)seq * p.Hq * p.nsplit * 2;
  for (int i = tid; i < G * HD; i += 256) {
    const int g = i / HD, d = i - g * HD;
    float v = red[0][g][d];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += red[k][g][d];
    const int hq = hkv * G + g;
    po[((size_t)hq * p.nsplit + split) * HD + d] = v;
    if (d == 0) {
      pm[((size_t)hq * p.nsplit + split) * 2 + 0] = ml[g][0];
      pm[((size_t)hq * p.nsplit + split) * 2 + 1] = ml[g][1];
    }
  }
}

// merge the per-split partials of one query head (decode_attn_combine_body, decode_common.hip.h: the bf16 kernels' merge)
__global__ __launch_bounds__(256) void cross_attn_fp8_combine_kernel(const float* __restrict__ part_o,
                                                                     const float* __restrict__ part_ml,
                                                                     bf16_t* __restrict__ out, int nsplit,
                                                                     const int* __restrict__ nkeys_m1, int key_tokens) {
  decode_attn_combine_body(part_o, part_ml, out, nsplit, nkeys_m1, key_tokens, 0);
}

static int cross_attn_fp8_impl(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                               const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o, void* part_ml,
                               void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit, float scale, float eps,
                               int batch, long long q_bs, long long kv_bs, long long sc_bs, hipStream_t stream) {
  if (!q || !q_norm_w || !k_codes || !k_scale || !v_codes || !v_scale || !nkeys_m1 || !part_o || !part_ml || !out)
    return VIS_ERR_ARG;
  if (HD != 128 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return VIS_ERR_ARG;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 7 && G != 8) return VIS_ERR_ARG;
  if (nsplit <= 0 || nsplit > 256 || key_tokens <= 0 || key_tokens % XKV_KEYS != 0) return VIS_ERR_ARG;
  if ((long long)nsplit * XKV_KEYS < key_tokens) return VIS_ERR_ARG;   // every key must be covered
  if (batch <= 0 || batch > 64 || (batch > 1 && (q_bs <= 0 || kv_bs <= 0 || sc_bs <= 0))) return VIS_ERR_ARG;
  if ((q_bs % 8) || (kv_bs % 16) || (sc_bs % 4)) return VIS_ERR_ARG;
  if (((uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)k_scale | (uintptr_t)v_scale) & 15) return VIS_ERR_ARG;
  if (((uintptr_t)nkeys_m1 | (uintptr_t)part_o | (uintptr_t)part_ml) & 3) return VIS_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)q_norm_w | (uintptr_t)out) & 1) return VIS_ERR_ARG;
  XkvArgs p;
  p.q = (const bf16_t*)q; p.q_norm_w = (const bf16_t*)q_norm_w;
  p.kq = (const uint8_t*)k_codes; p.vq = (const uint8_t*)v_codes;
  p.ksc = (const float*)k_scale; p.vsc = (const float*)v_scale;
  p.nkeys_m1 = (const int*)nkeys_m1; p.part_o = (float*)part_o; p.part_ml = (float*)part_ml;
  p.Hq = Hq; p.Hkv = Hkv; p.key_tokens = key_tokens; p.nsplit = nsplit;
  p.scale_log2 = scale * 1.4426950408889634f; p.eps = eps;
  p.q_bs = q_bs; p.kv_bs = kv_bs; p.sc_bs = sc_bs;
  vis_clear_error();
  const dim3 grid(Hkv, nsplit, batch), block(256);
  switch (G) {
    case 1: hipLaunchKernelGGL(cross_attn_fp8_kernel<1>, grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL(cross_attn_fp8_kernel<2>, grid, block, 0, stream, p); break;
    case 4: hipLaunchKernelGGL(cross_attn_fp8_kernel<4>, grid, block, 0, stream, p); break;
    case 7: hipLaunchKernelGGL(cross_attn_fp8_kernel<7>, grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL(cross_attn_fp8_kernel<8>, grid, block, 0, stream, p); break;
  }
  hipLaunchKernelGGL(cross_attn_fp8_combine_kernel, dim3(Hq, batch), dim3(256), 0, stream, (const float*)part_o,
                     (const float*)part_ml, (bf16_t*)out, nsplit, (const int*)nkeys_m1, key_tokens);
  return vis_check_launch();
}

extern "C" int vis_decode_cross_attn_fp8(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                                         const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o,
                                         void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                         float scale, float eps, hipStream_t stream) {
  return cross_attn_fp8_impl(q, q_norm_w, k_codes, k_scale, v_codes, v_scale, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD,
                             key_tokens, nsplit, scale, eps, 1, 0, 0, 0, stream);
}

// Batch form: sequence b reads q + b * q_bs, its codes at k_codes / v_codes + b * kv_bs, its scales at k_scale / v_scale +
// b * sc_bs (element strides) and nkeys_m1[b]; out [batch][Hq * 128]; workspaces sized batch x the single-sequence ones.
extern "C" int vis_decode_cross_attn_fp8_batch(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                                               const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o,
                                               void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                               float scale, float eps, int batch, long long q_bs, long long kv_bs,
                                               long long sc_bs, hipStream_t stream) {
  return cross_attn_fp8_impl(q, q_norm_w, k_codes, k_scale, v_codes, v_scale, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD,
                             key_tokens, nsplit, scale, eps, batch, q_bs, kv_bs, sc_bs, stream);
}

// ----------------------------------------------------------------------------------------- vis_decode_cross_attn_fp8_draft
// vis_decode_cross_attn_fp8 for the R rows of one speculative step (spec.hip: vis_decode_cross_attn_draft is the bf16 form): the
// split's codes and scales are loaded ONCE, row r's normalised heads take MFMA columns r G .. r G + G - 1, statistics and weights
// run per column.  P * V and the merge of the eight key groups run row after row through the single-row kernel's `red` - at 16
// columns a `red` for all rows would be 64 KB and leave one workgroup per CU - with the V codes converted once, in registers.
// Per (row, head) the arithmetic, key order and accumulation order are cross_attn_fp8_kernel's: output row r is bit-identical to
// vis_decode_cross_attn_fp8 on q row r alone.
struct XkvDraftArgs {
  XkvArgs a;     // q_bs = the row stride q_ld; kv_bs = sc_bs = 0 (one sequence); part_o / part_ml [rows][Hq][nsplit][..]
  int rows;
};

template <int G>
__global__ __launch_bounds__(256) void cross_attn_fp8_draft_kernel(XkvDraftArgs pa) {
  constexpr int HD = 128;
  constexpr int CMAX = (4 * G <= 16 ? 4 : 16 / G) * G;   // MFMA columns whole rows can fill: G = 1, 2, 4: 4 rows; 7, 8: 2
  const XkvArgs& p = pa.a;
  __shared__ __attribute__((aligned(16))) bf16_t q_s[16][HD + 8];   // columns >= rows * G are zero
  __shared__ __attribute__((aligned(16))) uint32_t v_s[XKV_KEYS][HD / 4];
  __shared__ float vsc_s[XKV_KEYS];
  __shared__ float sc[CMAX][XKV_KEYS];
  __shared__ float pw[CMAX][XKV_KEYS];
  __shared__ __attribute__((aligned(16))) float red[8][G][HD];      // one row at a time
  __shared__ float ml[CMAX][2];
  const int hkv = blockIdx.x, split = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, h = lane >> 4;
  const int rows = min(pa.rows, CMAX / G);   // (the host has checked rows * G <= 16)
  const int cols = rows * G;
  const int ks = split * XKV_KEYS;
  if (ks >= p.key_tokens) return;   // workgroup-uniform; key_tokens % 64 == 0: every row of a split that runs lies inside the buffers
  const size_t row0 = (size_t)hkv * p.key_tokens + ks;
  const uint8_t* Kr = p.kq + row0 * HD;
  const uint8_t* Vr = p.vq + row0 * HD;
  const float* Ks = p.ksc + row0;
  const float* Vs = p.vsc + row0;

  // ---- every read of the split up front, once for all rows
  const u32x4 k0 = *(const u32x4*)(Kr + (size_t)(16 * wave + l15) * HD + 32 * h);
  const u32x4 k1 = *(const u32x4*)(Kr + (size_t)(16 * wave + l15) * HD + 32 * h + 16);
  const f32x4 ksc4 = *(const f32x4*)(Ks + 16 * wave + 4 * h);
  const u32x4 va = *(const u32x4*)(Vr + (size_t)tid * 16);
  const u32x4 vb = *(const u32x4*)(Vr + (size_t)(tid + 256) * 16);
  const float vsc1 = Vs[lane];

  const int slot = min(p.nkeys_m1[0], p.key_tokens - 1);
  const int ctx = slot + 1;
  if (ks >= ctx) return;            // nothing to attend to: the combine never reads this split's partials
  const int nk = min(ks + XKV_KEYS, ctx) - ks;

  // ---- q_norm of every row's G heads, one wave per column
  for (int c = wave; c < cols; c += 4) {
    const int r = c / G, g = c - r * G;
    const bf16_t* qh = p.q + (size_t)r * p.q_bs + (size_t)(hkv * G + g) * HD;
    const float a = bf2f(qh[lane]), b = bf2f(qh[lane + 64]);
    const float ss = wave_sum(a * a + b * b);
    const float rstd = rsqrtf(ss * (1.0f / HD) + p.eps);
    q_s[c][lane] = f2bf(bf2f(f2bf(a * rstd)) * bf2f(p.q_norm_w[lane]));
    q_s[c][lane + 64] = f2bf(bf2f(f2bf(b * rstd)) * bf2f(p.q_norm_w[lane + 64]));
  }
  for (int it = tid; it < (16 - cols) * HD; it += 256) q_s[cols + it / HD][it % HD] = 0;
  *(u32x4*)(&v_s[0][0] + (size_t)tid * 4) = va;
  *(u32x4*)(&v_s[0][0] + (size_t)(tid + 256) * 4) = vb;
  if (wave == 0) vsc_s[lane] = vsc1;
  __syncthreads();

  // ---- scores on the MFMA, one pass over the keys for all columns (operand order: cross_attn_fp8_kernel's)
  if (16 * wave < nk) {   // wave-uniform
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      const u32x4 kk = (ds < 2) ? k0 : k1;
      const bf16x8 kf = xkv_cvt8_bf16(kk[2 * (ds & 1)], kk[2 * (ds & 1) + 1]);
      const bf16x8 qf = *(const bf16x8*)(&q_s[l15][32 * h + 8 * ds]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, acc, 0, 0, 0);
    }
    if (l15 < cols) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[l15][16 * wave + 4 * h + r] = (acc[r] * ksc4[r]) * p.scale_log2;
    }
  }
  __syncthreads();

  // ---- per-column softmax statistics over this split (one wave per column, one key per lane)
  for (int c = wave; c < cols; c += 4) {
    const bool live = lane < nk;
    const float s = live ? sc[c][lane] : -1.0e30f;
    const float mx = wave_max(s);
    const float e = live ? exp2f(s - mx) : 0.f;
    const float ls = wave_sum(e);
    pw[c][lane] = live ? e * vsc_s[lane] : 0.f;
    if (lane == 0) { ml[c][0] = mx; ml[c][1] = ls; }
  }
  __syncthreads();

  // ---- O[g][d] += w[g][key] * vcode[key][d] per row: thread = (key group kg, dims 4 d4 .. 4 d4 + 3), keys kg + 8 i ascending
  const int d4 = tid & 31, kg = tid >> 5;
  float vf[XKV_KEYS / 8][4];
#pragma unroll
  for (int i = 0; i < XKV_KEYS / 8; ++i) {
    const int key = kg + 8 * i;
    uint32_t w = v_s[key][d4];
    if (key >= nk) w = 0u;          // a row past the count: code 0 = +0.0 whatever it holds, and its weight is 0
    xkv_cvt4(w, vf[i]);
  }
  for (int r = 0; r < rows; ++r) {  // workgroup-uniform trip count
    float acc[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) { acc[g][0] = 0.f; acc[g][1] = 0.f; acc[g][2] = 0.f; acc[g][3] = 0.f; }
#pragma unroll
    for (int i = 0; i < XKV_KEYS / 8; ++i) {
      const int key = kg + 8 * i;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pg = pw[r * G + g][key];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[g][j] += pg * vf[i][j];
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) *(f32x4*)(&red[kg][g][4 * d4]) = (f32x4){acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
    __syncthreads();
    float* po = p.part_o + (size_t)r * p.Hq * p.nsplit * HD;
    float* pm = p.part_ml + (size_t)r * p.Hq * p.nsplit * 2;
    for (int i = tid; i < G * HD; i += 256) {
      const int g = i / HD, d = i - g * HD;
      float v = red[0][g][d];
#pragma unroll
      for (int k = 1; k < 8; ++k) v += red[k][g][d];
      const int hq = hkv * G + g;
      po[((size_t)hq * p.nsplit + split) * HD + d] = v;
      if (d == 0) {
        pm[((size_t)hq * p.nsplit + split) * 2 + 0] = ml[r * G + g][0];
        pm[((size_t)hq * p.nsplit + split) * 2 + 1] = ml[r * G + g][1];
      }
    }
    __syncthreads();                // the next row reuses red
  }
}

// grid (Hq, rows): the plain merge per (head, row), every row over the one shared key count
__global__ __launch_bounds__(256) void cross_attn_fp8_draft_combine_kernel(const float* __restrict__ part_o,
                                                                           const float* __restrict__ part_ml,
                                                                           bf16_t* __restrict__ out, int nsplit,
                                                                           const int* __restrict__ nkeys_m1, int key_tokens) {
  decode_attn_combine_body(part_o, part_ml, out, nsplit, nkeys_m1, key_tokens, 2);
}

extern "C" int vis_decode_cross_attn_fp8_draft(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                                               const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o,
                                               void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                               float scale, float eps, int rows, long long q_ld, hipStream_t stream) {
  if (!q || !q_norm_w || !k_codes || !k_scale || !v_codes || !v_scale || !nkeys_m1 || !part_o || !part_ml || !out)
    return VIS_ERR_ARG;
  if (HD != 128 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return VIS_ERR_ARG;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 7 && G != 8) return VIS_ERR_ARG;
  if (nsplit <= 0 || nsplit > 256 || key_tokens <= 0 || key_tokens % XKV_KEYS != 0) return VIS_ERR_ARG;
  if ((long long)nsplit * XKV_KEYS < key_tokens) return VIS_ERR_ARG;   // every key must be covered
  if (rows < 1 || rows > 4 || rows * G > 16) return VIS_ERR_ARG;       // every row's heads in the 16 MFMA columns
  if (q_ld < (long long)Hq * 128 || (q_ld % 8)) return VIS_ERR_ARG;
  if (((uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)k_scale | (uintptr_t)v_scale) & 15) return VIS_ERR_ARG;
  if (((uintptr_t)nkeys_m1 | (uintptr_t)part_o | (uintptr_t)part_ml) & 3) return VIS_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)q_norm_w | (uintptr_t)out) & 1) return VIS_ERR_ARG;
  XkvDraftArgs pa;
  XkvArgs& p = pa.a;
  p.q = (const bf16_t*)q; p.q_norm_w = (const bf16_t*)q_norm_w;
  p.kq = (const uint8_t*)k_codes; p.vq = (const uint8_t*)v_codes;
  p.ksc = (const float*)k_scale; p.vsc = (const float*)v_scale;
  p.nkeys_m1 = (const int*)nkeys_m1; p.part_o = (float*)part_o; p.part_ml = (float*)part_ml;
  p.Hq = Hq; p.Hkv = Hkv; p.key_tokens = key_tokens; p.nsplit = nsplit;
  p.scale_log2 = scale * 1.4426950408889634f; p.eps = eps;
  p.q_bs = q_ld; p.kv_bs = 0; p.sc_bs = 0;
  pa.rows = rows;
  vis_clear_error();
  const dim3 grid(Hkv, nsplit), block(256);
  switch (G) {
    case 1: hipLaunchKernelGGL(cross_attn_fp8_draft_kernel<1>, grid, block, 0, stream, pa); break;
    case 2: hipLaunchKernelGGL(cross_attn_fp8_draft_kernel<2>, grid, block, 0, stream, pa); break;
    case 4: hipLaunchKernelGGL(cross_attn_fp8_draft_kernel<4>, grid, block, 0, stream, pa); break;
    case 7: hipLaunchKernelGGL(cross_attn_fp8_draft_kernel<7>, grid, block, 0, stream, pa); break;
    default: hipLaunchKernelGGL(cross_attn_fp8_draft_kernel<8>, grid, block, 0, stream, pa); break;
  }
  hipLaunchKernelGGL(cross_attn_fp8_draft_combine_kernel, dim3(Hq, rows), dim3(256), 0, stream, (const float*)part_o,
                     (const float*)part_ml, (bf16_t*)out, nsplit, (const int*)nkeys_m1, key_tokens);
  return vis_check_launch();
}
