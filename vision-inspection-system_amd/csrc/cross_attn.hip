// Decode-step cross-attention over the image's static keys / values (Mllama's cross layers, the Auditor): all six entry points.
//
//   vis_decode_cross_attn, _batch, _draft                  bf16 keys / values          cross_attn_bf16_kernel
//   vis_decode_cross_attn_fp8, _fp8_batch, _fp8_draft      fp8 (OCP e4m3) copies       cross_attn_fp8_kernel    (cross_kv="fp8")
//
// One split body per key format, template <G, MAXROWS>, grid (Hkv, nsplit, batch): a workgroup takes one (kv head, split of 64
// keys, sequence), applies the q_norm RMS (HF rounding) to its query heads while it stages them, attends keys [0, nkeys_m1[seq] +
// 1) - the count is read from device memory and clamped into [.., key_tokens) before it bounds anything - and leaves the (m, l,
// o) partials of the split in the layout decode_attn_combine_body (decode_common.hip.h) merges.  Every K / V read of the split
// is issued before the count has arrived; splits at or past the count exit (the combine never reads their partials).
//
// MAXROWS says how many query ROWS share the pass over the keys.  The score MFMA's B operand has 16 columns, a row needs G:
//   MAXROWS = 1           single and batch forms: columns 0 .. G - 1, the rest zero; the row loops fold at compile time.
//   MAXROWS = SP_MAXROWS  draft forms: the R rows of ONE sequence's speculative step (batch 1, one shared key count), row r's
//                         normalised heads in columns r G .. r G + G - 1; rows * G <= 16 (G = 1, 2, 4: 4 rows; 7, 8: 2).
// An MFMA output column depends on its own B column only, and everything behind the scores - statistics, P, P * V, the merge -
// runs per column in one key order and one accumulation order, so output row r of a draft launch is, bit for bit, the single
// launch on q row r alone, whatever the other rows hold.  (A batch launch with a batch stride of 0 would read the image's K / V
// once per row: 212 MB per step at 11B shapes, times R.)
//
// The two formats keep their own arithmetic and LDS layout; see the comment in front of each body.  vis_decode_cross_attn_batch
// at Hkv * batch >= 128 runs the STREAMING form instead (decode_attn_stream_kernel, decode.hip: different summation order,
// equal to f32 rounding, not bit for bit) - da_use_stream_form() is the one place that decides.
#include "decode_common.hip.h"

// MFMA columns a group size fills with whole rows
template <int G, int MAXROWS>
struct XCols { static constexpr int value = (MAXROWS * G <= 16 ? MAXROWS : 16 / G) * G; };

// merge the per-split partials of one query head (decode_attn_combine_body, decode_common.hip.h): grid (Hq, batch) with
// POS_MODE 0 (sequence y at its own count), grid (Hq, rows) with POS_MODE 2 (row y over the one shared count)
template <int POS_MODE>
__global__ __launch_bounds__(256) void cross_attn_combine_kernel(const float* __restrict__ part_o,
                                                                 const float* __restrict__ part_ml,
                                                                 bf16_t* __restrict__ out, int nsplit,
                                                                 const int* __restrict__ nkeys_m1, int key_tokens) {
  decode_attn_combine_body(part_o, part_ml, out, nsplit, nkeys_m1, key_tokens, POS_MODE);
}

// q_norm of the launch's query heads (RMSNorm over the 128 dims of each head, HF rounding: normalised value to bf16, then times
// the weight), one wave per MFMA column, into q_s[column]; columns >= cols are zeroed.  Row r of sequence `seq`: q + seq * q_bs
// + r * q_ld.  QS: the row type of q_s (the two formats pad it differently).
template <int G, int MAXROWS, class QS>
__device__ __forceinline__ void xattn_stage_q(QS* q_s, const bf16_t* q, const bf16_t* q_norm_w, long long q_ld, float eps,
                                              int hkv, int cols) {
  constexpr int HD = 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = wave; c < cols; c += 4) {
    const int r = MAXROWS == 1 ? 0 : c / G, g = c - r * G;
    const bf16_t* qh = q + (size_t)r * q_ld + (size_t)(hkv * G + g) * HD;
    const float a = bf2f(qh[lane]), b = bf2f(qh[lane + 64]);
    const float ss = wave_sum(a * a + b * b);
    const float rstd = rsqrtf(ss * (1.0f / HD) + eps);
    q_s[c][lane] = f2bf(bf2f(f2bf(a * rstd)) * bf2f(q_norm_w[lane]));
    q_s[c][lane + 64] = f2bf(bf2f(f2bf(b * rstd)) * bf2f(q_norm_w[lane + 64]));
  }
  for (int it = tid; it < (16 - cols) * HD; it += 256) q_s[cols + it / HD][it % HD] = 0;
}

// ------------------------------------------------------------------------------------------------------------ bf16 keys
// The arithmetic, key order and LDS score layout (da_pos) of the split self-attention item (decode_attn_split_body) without
// its rope, append and new-row selects: S^T = K Q^T on the MFMA straight from the cache rows (clamped into the buffer: any
// key_tokens), statistics per column in f32, P kept in f32, P * V on the VALU with a lane owning two output dims and its
// wave's keys (wave + 4 i, ascending), the four waves merged through `red`.
struct XAttnArgs {
  const bf16_t* q;         // sequence s, row r: q + s * q_bs + r * q_ld, Hq * 128 leading columns
  const bf16_t* q_norm_w;  // [128]
  const bf16_t* k;         // [Hkv][key_tokens][128], sequence s at + s * kv_bs
  const bf16_t* v;
  const int* nkeys_m1;     // [batch]; the draft form's rows share nkeys_m1[0]
  float* part_o;           // [batch or rows][Hq][nsplit][128]
  float* part_ml;          // [batch or rows][Hq][nsplit][2]
  int Hq, Hkv, key_tokens, nsplit;
  float scale_log2, eps;
  long long q_bs, kv_bs;   // element strides between sequences
  long long q_ld;          // draft form: element stride between rows, and their number
  int rows;
};

template <int G, int MAXROWS>
__global__ __launch_bounds__(256) void cross_attn_bf16_kernel(XAttnArgs p) {
  constexpr int HD = 128;
  constexpr int CMAX = XCols<G, MAXROWS>::value;
  constexpr int KGRP = DA_MAXKEYS / 16 / 4;  // 16-key groups per wave (2)
  constexpr int VROWS = DA_MAXKEYS / 4;      // V rows per wave (32)
  __shared__ __attribute__((aligned(16))) bf16_t q_s[16][HD];   // columns >= rows * G are zero
  __shared__ __attribute__((aligned(16))) float sc[CMAX][DA_MAXKEYS];
  __shared__ __attribute__((aligned(16))) float red[4][CMAX][HD];   // 32 KB at 16 columns
  __shared__ float ml[CMAX][2];
  const int hkv = blockIdx.x, split = blockIdx.y, seq = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, h = lane >> 4;
  const int rows = MAXROWS == 1 ? 1 : min(p.rows, CMAX / G);    // (the host has checked rows * G <= 16)
  const int cols = rows * G;
  const bf16_t* Kr = p.k + (size_t)seq * p.kv_bs + (size_t)hkv * p.key_tokens * HD;
  const bf16_t* Vr = p.v + (size_t)seq * p.kv_bs + (size_t)hkv * p.key_tokens * HD;
  const int ks = split * DA_MAXKEYS;

  // ---- every K / V read of the split up front, ONCE for all rows (clamped rows: addresses do not depend on the key count)
  u32x4 kreg[KGRP][4];
#pragma unroll
  for (int gi = 0; gi < KGRP; ++gi) {
    const int row = min(ks + (wave + 4 * gi) * 16 + l15, p.key_tokens - 1);
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) kreg[gi][ds] = *(const u32x4*)(Kr + (size_t)row * HD + ds * 32 + 8 * h);
  }
  uint32_t vreg[VROWS];
#pragma unroll
  for (int i = 0; i < VROWS; ++i) {
    const int row = min(ks + wave + 4 * i, p.key_tokens - 1);
    vreg[i] = *(const uint32_t*)(Vr + (size_t)row * HD + 2 * lane);
  }

  const int slot = min(p.nkeys_m1[seq], p.key_tokens - 1);
  const int ctx = slot + 1;
  if (ks >= ctx) return;  // whole block: nothing to attend to (its partials are never read by the combine)
  const int nk = min(ks + DA_MAXKEYS, ctx) - ks;

  xattn_stage_q<G, MAXROWS>(q_s, p.q + (size_t)seq * p.q_bs, p.q_norm_w, p.q_ld, p.eps, hkv, cols);
  __syncthreads();

  // ---- scores on the MFMA: one pass over the keys for all columns
  bf16x8 qf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) qf[ds] = *(const bf16x8*)(&q_s[l15][ds * 32 + 8 * h]);
#pragma unroll
  for (int gi = 0; gi < KGRP; ++gi) {
    const int kbase = (wave + 4 * gi) * 16;
    if (kbase < nk) {  // wave-uniform
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < 4; ++ds)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kreg[gi][ds]), qf[ds], acc, 0, 0, 0);
      // acc[r] = S^T[key = kbase + 4h + r][column = l15]
      if (l15 < cols) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[l15][da_pos(kbase + 4 * h + r)] = acc[r] * p.scale_log2;
      }
    }
  }
  __syncthreads();

  // ---- per-column softmax statistics over this split (one wave per column)
  for (int c = wave; c < cols; c += 4) {
    float mx = -1.0e30f;
    for (int i = lane; i < nk; i += 64) mx = fmaxf(mx, sc[c][da_pos(i)]);
    mx = wave_max(mx);
    float ls = 0.f;
    for (int i = lane; i < DA_MAXKEYS; i += 64) {      // slots past the split's end get p = 0: P * V runs branch-free
      const float e = (i < nk) ? exp2f(sc[c][da_pos(i)] - mx) : 0.f;
      sc[c][da_pos(i)] = e;
      if (i < nk) ls += e;
    }
    ls = wave_sum(ls);
    if (lane == 0) { ml[c][0] = mx; ml[c][1] = ls; }
  }
  __syncthreads();

  // ---- O[c][d] += p[c][key] * V[key][d]; lane owns d = 2 * lane, 2 * lane + 1; the V registers serve every column.  This
  //      wave's keys (wave + 4 i) sit at 16 consecutive floats of a column's row (da_pos): four ds_read_b128 per column
  float v0[VROWS], v1[VROWS];
#pragma unroll
  for (int i = 0; i < VROWS; ++i) {
    uint32_t raw = vreg[i];
    if (wave + 4 * i >= nk) raw = 0u;      // (a clamped duplicate row: whatever it holds, 0 x 0 adds nothing)
    v0[i] = __uint_as_float(raw << 16);
    v1[i] = __uint_as_float(raw & 0xffff0000u);
  }
  for (int c = 0; c < cols; ++c) {
    f32x4 pq[VROWS / 4];
#pragma unroll
    for (int q = 0; q < VROWS / 4; ++q) pq[q] = *(const f32x4*)(&sc[c][wave * VROWS + 4 * q]);
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int i = 0; i < VROWS; ++i) {      // keys in ascending order per accumulator; past the split's end p = 0 and v = 0
      const float pw = pq[i >> 2][i & 3];
      a0 += pw * v0[i];
      a1 += pw * v1[i];
    }
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    *(f32x2_*)(&red[wave][c][2 * lane]) = (f32x2_){a0, a1};
  }
  __syncthreads();
  for (int i = tid; i < cols * HD; i += 256) {
    const int c = i / HD, d = i - c * HD;
    const int r = MAXROWS == 1 ? 0 : c / G, g = c - r * G;
    const float v = red[0][c][d] + red[1][c][d] + red[2][c][d] + red[3][c][d];
    const int hq = hkv * G + g;
    float* po = p.part_o + (size_t)(seq * rows + r) * p.Hq * p.nsplit * HD;
    float* pm = p.part_ml + (size_t)(seq * rows + r) * p.Hq * p.nsplit * 2;
    po[((size_t)hq * p.nsplit + split) * HD + d] = v;
    if (d == 0) {
      pm[((size_t)hq * p.nsplit + split) * 2 + 0] = ml[c][0];
      pm[((size_t)hq * p.nsplit + split) * 2 + 1] = ml[c][1];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- fp8 keys
// Storage, per slot and cross layer: codes uint8 [Hkv][key_tokens][128] for K and for V, one f32 scale per (kv head, key row)
// for each, [Hkv][key_tokens].  The codes and scales are written once per prompt pass by vis_quant_rows_fp8 (no norm) over the
// bf16 rows: scale = max(amax / 448, 1e-12), code = e4m3_rne_saturating(x * (1 / scale)).  Its all-zero-row rule: amax = 0
// gives scale 1e-12 (never 0) and 128 codes 0, so a zero row dequantises to exact zeros and no scale is ever 0 or inf.
//
// A row at or past the key count is loaded (its address lies inside the buffers: key_tokens is a multiple of 64) but never
// used: its score is never read, its weight and its value codes are replaced by zeros with selects, so NaN codes and inf scales
// there change nothing.
//
// Arithmetic.  Softmax scheme: that of the bf16 body, NOT the prompt pass's: statistics per column over the split's keys in
// f32, p = exp2(s - m) kept in f32 - P is never rounded to bf16 - and P * V on the VALU in f32.
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
//
// Rows.  P * V and the merge of the eight key groups run row after row through ONE row's `red` - at 16 columns a `red` for all
// rows would be 64 KB and leave one workgroup per CU - with the V codes converted once, in registers.
struct XkvArgs {
  const bf16_t* q;         // sequence s, row r: q + s * q_bs + r * q_ld, Hq * 128 leading columns
  const bf16_t* q_norm_w;  // [128]
  const uint8_t* kq;       // [Hkv][key_tokens][128], sequence s at + s * kv_bs
  const uint8_t* vq;
  const float* ksc;        // [Hkv][key_tokens], sequence s at + s * sc_bs
  const float* vsc;
  const int* nkeys_m1;     // [batch]; the draft form's rows share nkeys_m1[0]
  float* part_o;           // [batch or rows][Hq][nsplit][128]
  float* part_ml;          // [batch or rows][Hq][nsplit][2]
  int Hq, Hkv, key_tokens, nsplit;
  float scale_log2, eps;
  long long q_bs, kv_bs, sc_bs;   // element strides between sequences: q, codes, scales
  long long q_ld;                 // draft form: element stride between rows, and their number
  int rows;
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

#define XKV_KEYS DA_MAXKEYS   // 64: the split of the bf16 body

template <int G, int MAXROWS>
__global__ __launch_bounds__(256) void cross_attn_fp8_kernel(XkvArgs p) {
  constexpr int HD = 128;
  constexpr int CMAX = XCols<G, MAXROWS>::value;
  static_assert(XKV_KEYS == 64, "one key per lane in the softmax, 16 keys per wave on the MFMA");
  // rows padded by 16 bytes: at a 256-byte stride the 16 columns a lane group reads for the B operand would share their banks
  __shared__ __attribute__((aligned(16))) bf16_t q_s[16][HD + 8];   // columns >= rows * G are zero
  __shared__ __attribute__((aligned(16))) uint32_t v_s[XKV_KEYS][HD / 4];
  __shared__ float vsc_s[XKV_KEYS];
  __shared__ float sc[CMAX][XKV_KEYS];
  __shared__ float pw[CMAX][XKV_KEYS];
  __shared__ __attribute__((aligned(16))) float red[8][G][HD];      // one row at a time
  __shared__ float ml[CMAX][2];
  const int hkv = blockIdx.x, split = blockIdx.y, seq = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, h = lane >> 4;
  const int rows = MAXROWS == 1 ? 1 : min(p.rows, CMAX / G);   // (the host has checked rows * G <= 16)
  const int cols = rows * G;
  const int ks = split * XKV_KEYS;
  if (ks >= p.key_tokens) return;   // workgroup-uniform; key_tokens % 64 == 0: every row of a split that runs lies inside the buffers
  const size_t row0 = (size_t)hkv * p.key_tokens + ks;
  const uint8_t* Kr = p.kq + (size_t)seq * p.kv_bs + row0 * HD;
  const uint8_t* Vr = p.vq + (size_t)seq * p.kv_bs + row0 * HD;
  const float* Ks = p.ksc + (size_t)seq * p.sc_bs + row0;
  const float* Vs = p.vsc + (size_t)seq * p.sc_bs + row0;

  // ---- every read of the split up front, once for all rows (addresses do not depend on the key count)
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

  xattn_stage_q<G, MAXROWS>(q_s, p.q + (size_t)seq * p.q_bs, p.q_norm_w, p.q_ld, p.eps, hkv, cols);
  *(u32x4*)(&v_s[0][0] + (size_t)tid * 4) = va;
  *(u32x4*)(&v_s[0][0] + (size_t)(tid + 256) * 4) = vb;
  if (wave == 0) vsc_s[lane] = vsc1;
  __syncthreads();

  // ---- scores on the MFMA, one pass over the keys for all columns: A = the wave's 16 keys (row = lane & 15), B = q^T;
  //      contraction index of step ds, lane group h, element j = dim 32 h + 8 ds + j in both
  if (16 * wave < nk) {   // wave-uniform
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      const u32x4 kk = (ds < 2) ? k0 : k1;
      const bf16x8 kf = xkv_cvt8_bf16(kk[2 * (ds & 1)], kk[2 * (ds & 1) + 1]);
      const bf16x8 qf = *(const bf16x8*)(&q_s[l15][32 * h + 8 * ds]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, acc, 0, 0, 0);
    }
    // acc[r] = sum_d kcode[key = 16 wave + 4 h + r][d] * q[column = l15][d]
    if (l15 < cols) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[l15][16 * wave + 4 * h + r] = (acc[r] * ksc4[r]) * p.scale_log2;
    }
  }
  __syncthreads();

  // ---- per-column softmax statistics over this split (one wave per column, one key per lane); keys past the count: p = 0 by select
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
    float* po = p.part_o + (size_t)(seq * rows + r) * p.Hq * p.nsplit * HD;
    float* pm = p.part_ml + (size_t)(seq * rows + r) * p.Hq * p.nsplit * 2;
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
    if (MAXROWS > 1) __syncthreads();   // the next row reuses red
  }
}

// ------------------------------------------------------------------------------------------------------------- the host
template <int G, int MAXROWS>
static void xattn_launch_split(const XAttnArgs& p, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((cross_attn_bf16_kernel<G, MAXROWS>), grid, dim3(256), 0, stream, p);
}
template <int G, int MAXROWS>
static void xattn_launch_split(const XkvArgs& p, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((cross_attn_fp8_kernel<G, MAXROWS>), grid, dim3(256), 0, stream, p);
}

// split launch + combine of either format.  draft: p.rows rows of one sequence; else `batch` sequences of one row
template <class Args>
static int xattn_launch(const Args& p, void* out, int batch, bool draft, hipStream_t stream) {
  vis_clear_error();
  da_dispatch_g(p.Hq / p.Hkv, [&](auto g) {
    constexpr int G = decltype(g)::value;
    if (draft) xattn_launch_split<G, SP_MAXROWS>(p, dim3(p.Hkv, p.nsplit), stream);
    else xattn_launch_split<G, 1>(p, dim3(p.Hkv, p.nsplit, batch), stream);
  });
  if (draft)
    hipLaunchKernelGGL(cross_attn_combine_kernel<2>, dim3(p.Hq, p.rows), dim3(256), 0, stream, (const float*)p.part_o,
                       (const float*)p.part_ml, (bf16_t*)out, p.nsplit, p.nkeys_m1, p.key_tokens);
  else
    hipLaunchKernelGGL(cross_attn_combine_kernel<0>, dim3(p.Hq, batch), dim3(256), 0, stream, (const float*)p.part_o,
                       (const float*)p.part_ml, (bf16_t*)out, p.nsplit, p.nkeys_m1, p.key_tokens);
  return vis_check_launch();
}

// what all forms of both formats refuse: head shapes without an instantiation, a split plan that does not cover the keys
static bool xattn_bad_shape(int Hq, int Hkv, int HD, int key_tokens, int nsplit) {
  if (HD != 128 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return true;
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 7 && G != 8) return true;
  return nsplit <= 0 || nsplit > 256 || key_tokens <= 0 || (long long)nsplit * DA_MAXKEYS < key_tokens;   // every key must be covered
}
// the draft forms: every row's heads in the 16 MFMA columns, q rows inside a packed buffer
static bool xattn_bad_rows(int Hq, int Hkv, int rows, long long q_ld) {
  return rows < 1 || rows > SP_MAXROWS || rows * (Hq / Hkv) > 16 || q_ld < (long long)Hq * 128 || (q_ld % 8);
}
static bool xattn_misaligned(const void* q, const void* q_norm_w, const void* nkeys_m1, const void* part_o, const void* part_ml,
                             const void* out) {
  return ((((uintptr_t)nkeys_m1 | (uintptr_t)part_o | (uintptr_t)part_ml) & 3) |
          (((uintptr_t)q | (uintptr_t)q_norm_w | (uintptr_t)out) & 1)) != 0;
}

// bf16: VIS_OK or VIS_ERR_ARG before anything is launched (no refused call touches its buffers)
static int xattn_bf16_check(const void* q, const void* q_norm_w, const void* k, const void* v, const void* nkeys_m1,
                            const void* part_o, const void* part_ml, const void* out, int Hq, int Hkv, int HD, int key_tokens,
                            int nsplit) {
  if (!q || !q_norm_w || !k || !v || !nkeys_m1 || !part_o || !part_ml || !out) return VIS_ERR_ARG;
  if (xattn_bad_shape(Hq, Hkv, HD, key_tokens, nsplit)) return VIS_ERR_ARG;
  if (((uintptr_t)k | (uintptr_t)v) & 15) return VIS_ERR_ARG;
  return VIS_OK;
}

static XAttnArgs xattn_bf16_args(const void* q, const void* q_norm_w, const void* k, const void* v, const void* nkeys_m1,
                                 void* part_o, void* part_ml, int Hq, int Hkv, int key_tokens, int nsplit, float scale, float eps,
                                 long long q_bs, long long kv_bs, int rows, long long q_ld) {
  XAttnArgs p;
  p.q = (const bf16_t*)q; p.q_norm_w = (const bf16_t*)q_norm_w; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.nkeys_m1 = (const int*)nkeys_m1; p.part_o = (float*)part_o; p.part_ml = (float*)part_ml;
  p.Hq = Hq; p.Hkv = Hkv; p.key_tokens = key_tokens; p.nsplit = nsplit; p.rows = rows;
  p.scale_log2 = scale * 1.4426950408889634f; p.eps = eps;
  p.q_bs = q_bs; p.kv_bs = kv_bs; p.q_ld = q_ld;
  return p;
}

// Cross-attention of one new token over a static key/value set: q [Hq*128] straight from the q projection (q_norm applied
// inside), keys/values [Hkv][key_tokens][128] written once per request by the prefill; *nkeys_m1 (device int) = number of
// valid keys - 1.  Batch form (mllama batched decode): sequence b reads q + b * q_bs, its own static keys / values k, v + b *
// kv_bs (element strides) and nkeys_m1[b]; out [batch][Hq * 128]; workspaces sized batch x the single-sequence ones.
static int cross_attn_bf16_impl(const void* q, const void* q_norm_w, const void* k, const void* v, const void* nkeys_m1,
                                void* part_o, void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                float scale, float eps, int batch, long long q_bs, long long kv_bs, hipStream_t stream) {
  if (xattn_bf16_check(q, q_norm_w, k, v, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD, key_tokens, nsplit)) return VIS_ERR_ARG;
  if (batch <= 0 || batch > 64 || (batch > 1 && (q_bs <= 0 || kv_bs <= 0)) || (q_bs % 8) || (kv_bs % 8)) return VIS_ERR_ARG;
  if (da_use_stream_form(Hkv, batch)) {   // the streaming form's cross mode: the self-attention arguments, no rope tables
    DecAttnArgs s;
    s.qkv = (const bf16_t*)q; s.cos_t = nullptr; s.sin_t = nullptr;
    s.k_cache = (bf16_t*)k; s.v_cache = (bf16_t*)v; s.step_ptr = (const int*)nkeys_m1;
    s.part_o = (float*)part_o; s.part_ml = (float*)part_ml;
    s.Hq = Hq; s.Hkv = Hkv; s.cache_tokens = key_tokens; s.nsplit = nsplit;
    s.scale_log2 = scale * 1.4426950408889634f;
    s.qkv_bs = q_bs; s.cache_bs = kv_bs; s.tab_bs = 0;
    s.q_norm_w = (const bf16_t*)q_norm_w; s.q_eps = eps;
    s.shared_len = 0;
    s.fork_parent = nullptr; s.fork_len = nullptr;
    da_no_parts(s);
    return decode_attn_stream_launch(s, out, batch, stream);
  }
  return xattn_launch(xattn_bf16_args(q, q_norm_w, k, v, nkeys_m1, part_o, part_ml, Hq, Hkv, key_tokens, nsplit, scale, eps, q_bs,
                                      kv_bs, 1, 0),
                      out, batch, false, stream);
}

extern "C" int vis_decode_cross_attn(const void* q, const void* q_norm_w, const void* k, const void* v,
                                     const void* nkeys_m1, void* part_o, void* part_ml, void* out, int Hq, int Hkv,
                                     int HD, int key_tokens, int nsplit, float scale, float eps, hipStream_t stream) {
  return cross_attn_bf16_impl(q, q_norm_w, k, v, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD, key_tokens, nsplit, scale, eps, 1,
                              0, 0, stream);
}

extern "C" int vis_decode_cross_attn_batch(const void* q, const void* q_norm_w, const void* k, const void* v,
                                           const void* nkeys_m1, void* part_o, void* part_ml, void* out, int Hq,
                                           int Hkv, int HD, int key_tokens, int nsplit, float scale, float eps,
                                           int batch, long long q_bs, long long kv_bs, hipStream_t stream) {
  return cross_attn_bf16_impl(q, q_norm_w, k, v, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD, key_tokens, nsplit, scale, eps,
                              batch, q_bs, kv_bs, stream);
}

// The R rows of one speculative step: row r = q + r * q_ld, all rows over the one count *nkeys_m1; part_o / part_ml / out
// [rows][..].  Row r is bit-identical to vis_decode_cross_attn on q row r alone.
extern "C" int vis_decode_cross_attn_draft(const void* q, const void* q_norm_w, const void* k, const void* v,
                                           const void* nkeys_m1, void* part_o, void* part_ml, void* out, int Hq, int Hkv,
                                           int HD, int key_tokens, int nsplit, float scale, float eps, int rows,
                                           long long q_ld, hipStream_t stream) {
  if (xattn_bf16_check(q, q_norm_w, k, v, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD, key_tokens, nsplit)) return VIS_ERR_ARG;
  if (xattn_bad_rows(Hq, Hkv, rows, q_ld) || xattn_misaligned(q, q_norm_w, nkeys_m1, part_o, part_ml, out)) return VIS_ERR_ARG;
  return xattn_launch(xattn_bf16_args(q, q_norm_w, k, v, nkeys_m1, part_o, part_ml, Hq, Hkv, key_tokens, nsplit, scale, eps, 0, 0,
                                      rows, q_ld),
                      out, 1, true, stream);
}

// fp8: VIS_OK or VIS_ERR_ARG before anything is launched; whole splits only, 16-byte aligned codes and scales
static int xattn_fp8_check(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale, const void* v_codes,
                           const void* v_scale, const void* nkeys_m1, const void* part_o, const void* part_ml, const void* out,
                           int Hq, int Hkv, int HD, int key_tokens, int nsplit) {
  if (!q || !q_norm_w || !k_codes || !k_scale || !v_codes || !v_scale || !nkeys_m1 || !part_o || !part_ml || !out)
    return VIS_ERR_ARG;
  if (xattn_bad_shape(Hq, Hkv, HD, key_tokens, nsplit) || key_tokens % XKV_KEYS != 0) return VIS_ERR_ARG;
  if (((uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)k_scale | (uintptr_t)v_scale) & 15) return VIS_ERR_ARG;
  return xattn_misaligned(q, q_norm_w, nkeys_m1, part_o, part_ml, out) ? VIS_ERR_ARG : VIS_OK;
}

static XkvArgs xattn_fp8_args(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale, const void* v_codes,
                              const void* v_scale, const void* nkeys_m1, void* part_o, void* part_ml, int Hq, int Hkv,
                              int key_tokens, int nsplit, float scale, float eps, long long q_bs, long long kv_bs, long long sc_bs,
                              int rows, long long q_ld) {
  XkvArgs p;
  p.q = (const bf16_t*)q; p.q_norm_w = (const bf16_t*)q_norm_w;
  p.kq = (const uint8_t*)k_codes; p.vq = (const uint8_t*)v_codes;
  p.ksc = (const float*)k_scale; p.vsc = (const float*)v_scale;
  p.nkeys_m1 = (const int*)nkeys_m1; p.part_o = (float*)part_o; p.part_ml = (float*)part_ml;
  p.Hq = Hq; p.Hkv = Hkv; p.key_tokens = key_tokens; p.nsplit = nsplit; p.rows = rows;
  p.scale_log2 = scale * 1.4426950408889634f; p.eps = eps;
  p.q_bs = q_bs; p.kv_bs = kv_bs; p.sc_bs = sc_bs; p.q_ld = q_ld;
  return p;
}

static int cross_attn_fp8_impl(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                               const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o, void* part_ml,
                               void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit, float scale, float eps,
                               int batch, long long q_bs, long long kv_bs, long long sc_bs, hipStream_t stream) {
  if (xattn_fp8_check(q, q_norm_w, k_codes, k_scale, v_codes, v_scale, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD, key_tokens,
                      nsplit))
    return VIS_ERR_ARG;
  if (batch <= 0 || batch > 64 || (batch > 1 && (q_bs <= 0 || kv_bs <= 0 || sc_bs <= 0))) return VIS_ERR_ARG;
  if ((q_bs % 8) || (kv_bs % 16) || (sc_bs % 4)) return VIS_ERR_ARG;
  return xattn_launch(xattn_fp8_args(q, q_norm_w, k_codes, k_scale, v_codes, v_scale, nkeys_m1, part_o, part_ml, Hq, Hkv,
                                     key_tokens, nsplit, scale, eps, q_bs, kv_bs, sc_bs, 1, 0),
                      out, batch, false, stream);
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

// vis_decode_cross_attn_draft over the fp8 copies: row r is bit-identical to vis_decode_cross_attn_fp8 on q row r alone.
extern "C" int vis_decode_cross_attn_fp8_draft(const void* q, const void* q_norm_w, const void* k_codes, const void* k_scale,
                                               const void* v_codes, const void* v_scale, const void* nkeys_m1, void* part_o,
                                               void* part_ml, void* out, int Hq, int Hkv, int HD, int key_tokens, int nsplit,
                                               float scale, float eps, int rows, long long q_ld, hipStream_t stream) {
  if (xattn_fp8_check(q, q_norm_w, k_codes, k_scale, v_codes, v_scale, nkeys_m1, part_o, part_ml, out, Hq, Hkv, HD, key_tokens,
                      nsplit) || xattn_bad_rows(Hq, Hkv, rows, q_ld))
    return VIS_ERR_ARG;
  return xattn_launch(xattn_fp8_args(q, q_norm_w, k_codes, k_scale, v_codes, v_scale, nkeys_m1, part_o, part_ml, Hq, Hkv,
                                     key_tokens, nsplit, scale, eps, 0, 0, 0, rows, q_ld),
                      out, 1, true, stream);
}
