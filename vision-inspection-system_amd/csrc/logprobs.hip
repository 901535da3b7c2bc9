// Token log-probabilities of the pick just made (vis_logprobs_f32): runs after vis_argmax_f32 / vis_gemv_bf16_argmax has
// advanced the step, so the position of the token just written is pos = step[b] - 1.  For every sequence b:
//   lse = max + log(sum exp(x - max)) over the row's V logits (the raw logits: temperature 1, no Gumbel noise),
//   lp[b][pos][0] = logits[tok] - lse for the token the pick stored (tokens[b][pos]),
//   lp[b][pos][1 + i] = logits[id_i] - lse, top_ids[b][pos][i] = id_i for the top_k largest logits, descending, ties to the
//   lower index (the order of argmax_stage1/2_kernel, so at temperature 0 top_ids[..][0] == tok and lp[1] == lp[0] bitwise).
// Positions past max_tokens are left alone, as the pick stores nothing there either.
//
// Stage 1: grid (chunks, batch), one 256-thread workgroup per LP_CHUNK logits; thread t holds the 16 logits
// chunk * 4096 + j * 1024 + 4 t + e (j, e < 4), read as four 16-byte loads (scalar loads at the row's end or when the row is
// not 16-byte aligned - same elements, same order).  Each thread's (max, sum of exp), then a butterfly over the wave and the
// four waves in order.  Top-k: k rounds per wave of a wave-wide max over every lane's best element below the previous pick
// (only the winning lane rescans its 16), then wave 0 merges the four sorted wave lists.  Stage 2: one wave per row merges
// the chunks' (max, sum) and their sorted top-k lists, a chunk per lane.  The reduction layout depends on V alone, never on
// the batch or the row's slot, so a row's results are bitwise the same alone or in any batch.
#include "common.hip.h"
#include <math.h>

#define LP_CHUNK 4096            // logits per stage-1 workgroup (256 threads x 16)
#define LP_MAXK 20               // OpenAI's top_logprobs limit
#define LP_REC 64                // floats per (row, chunk) workspace record: [0] max, [1] sum, [2..21] values, [32..51] ids
#define LP_MAXCHUNKS 64          // stage 2 merges one chunk per lane: V <= 64 x 4096 = 262144
#define LP_MAXBATCH 64           // the engines' largest batch

// a precedes b: larger value, or equal value and lower index (the argmax rule)
__device__ __forceinline__ bool lp_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// (m, s) <- (m, s) + (om, os): symmetric in its operands, so both lanes of a butterfly pair get the same bits
__device__ __forceinline__ void lp_lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm == -INFINITY) return;                      // both empty (all -inf so far)
  s = s * __expf(m - nm) + os * __expf(om - nm);
  m = nm;
}

__device__ __forceinline__ void lp_wave_lse(float& m, float& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lp_lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
}

// wave-wide first element in the argmax order; every lane ends with the same (v, i)
__device__ __forceinline__ void lp_wave_best(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (lp_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

template <bool TOPK>
__global__ __launch_bounds__(256) void logprobs_stage1_kernel(const float* __restrict__ logits, int V, int ld,
                                                              const int* __restrict__ step_ptr, int max_tokens, int k,
                                                              float* __restrict__ ws, int nchunks) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, chunk = blockIdx.x, row = blockIdx.y;
  const int pos = step_ptr[row] - 1;
  if (pos < 0 || pos >= max_tokens) return;        // uniform over the workgroup
  const float* __restrict__ x = logits + (size_t)row * ld;
  float* __restrict__ rec = ws + ((size_t)row * nchunks + chunk) * LP_REC;
  const int base = chunk * LP_CHUNK + tid * 4;
  const bool vec = (((uintptr_t)x) & 15) == 0;
  float v[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i0 = base + j * 1024;
    if (vec && i0 + 3 < V) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(x + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = q[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = (i0 + e < V) ? x[i0 + e] : -INFINITY;
    }
  }
  float m = v[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) m = fmaxf(m, v[j]);
  float s = 0.f;
  if (m != -INFINITY) {
#pragma unroll
    for (int j = 0; j < 16; ++j) s += __expf(v[j] - m);
  }
  lp_wave_lse(m, s);
  __shared__ float sm[4], ss[4];
  __shared__ float cv[4][LP_MAXK];
  __shared__ int ci[4][LP_MAXK];
  if (lane == 0) { sm[wid] = m; ss[wid] = s; }
  if (TOPK) {
    // this lane's best element below the previous pick (initially: its best)
    auto idx = [&](int j) { return base + (j >> 2) * 1024 + (j & 3); };
    float pv = INFINITY;
    int pi = -1;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    auto rescan = [&]() {
      bv = -INFINITY; bi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int ij = idx(j);
        if (lp_before(pv, pi, v[j], ij) && lp_before(v[j], ij, bv, bi)) { bv = v[j]; bi = ij; }
      }
    };
    rescan();
    for (int r = 0; r < k; ++r) {
      float wv = bv;
      int wi = bi;
      lp_wave_best(wv, wi);
      if (lane == 0) { cv[wid][r] = wv; ci[wid][r] = wi; }
      pv = wv; pi = wi;
      if (bi == wi) rescan();
    }
  }
  __syncthreads();
  if (wid != 0) return;
  if (lane == 0) {
    float M = sm[0], S = ss[0];
    for (int w = 1; w < 4; ++w) lp_lse_merge(M, S, sm[w], ss[w]);
    rec[0] = M;
    rec[1] = S;
  }
  if (TOPK) {
    // merge the four sorted wave lists: lane w < 4 holds the head of wave w's list
    int h = 0;
    float hv = lane < 4 ? cv[lane][0] : -INFINITY;
    int hi = lane < 4 ? ci[lane][0] : 0x7fffffff;
    for (int r = 0; r < k; ++r) {
      float wv = hv;
      int wi = hi;
#pragma unroll
      for (int o = 2; o > 0; o >>= 1) {            // lanes 0..3 hold the heads; the others are never read
        const float ov = __shfl_xor(wv, o, 64);
        const int oi = __shfl_xor(wi, o, 64);
        if (lp_before(ov, oi, wv, wi)) { wv = ov; wi = oi; }
      }
      if (lane == 0) { rec[2 + r] = wv; reinterpret_cast<int*>(rec)[32 + r] = wi; }
      if (lane < 4 && hi == wi) {
        ++h;
        hv = h < k ? cv[lane][h] : -INFINITY;
        hi = h < k ? ci[lane][h] : 0x7fffffff;
      }
    }
  }
}

__global__ __launch_bounds__(64) void logprobs_stage2_kernel(const float* __restrict__ logits, int V, int ld,
                                                             const int* __restrict__ tokens, int max_tokens,
                                                             const int* __restrict__ step_ptr, int k,
                                                             const float* __restrict__ ws, int nchunks,
                                                             float* __restrict__ lp, int* __restrict__ top_ids) {
  const int lane = threadIdx.x, row = blockIdx.x;
  const int pos = step_ptr[row] - 1;
  if (pos < 0 || pos >= max_tokens) return;
  const float* __restrict__ rec = ws + ((size_t)row * nchunks + lane) * LP_REC;
  const bool mine = lane < nchunks;
  float m = mine ? rec[0] : -INFINITY, s = mine ? rec[1] : 0.f;
  lp_wave_lse(m, s);
  const float lse = m + logf(s);
  float* __restrict__ out = lp + ((size_t)row * max_tokens + pos) * (LP_MAXK + 1);
  if (lane == 0) {
    const int tok = tokens[(size_t)row * max_tokens + pos];
    out[0] = (tok >= 0 && tok < V) ? logits[(size_t)row * ld + tok] - lse : NAN;
  }
  if (k == 0) return;
  __shared__ float hvs[LP_MAXCHUNKS][LP_MAXK];
  __shared__ int his[LP_MAXCHUNKS][LP_MAXK];
  if (mine) {
    for (int r = 0; r < k; ++r) {
      hvs[lane][r] = rec[2 + r];
      his[lane][r] = reinterpret_cast<const int*>(rec)[32 + r];
    }
  }
  int h = 0;
  float hv = mine ? hvs[lane][0] : -INFINITY;
  int hi = mine ? his[lane][0] : 0x7fffffff;
  int* __restrict__ ids = top_ids + ((size_t)row * max_tokens + pos) * LP_MAXK;
  for (int r = 0; r < k; ++r) {
    float wv = hv;
    int wi = hi;
    lp_wave_best(wv, wi);
    if (lane == 0) { out[1 + r] = wv - lse; ids[r] = wi; }
    if (mine && hi == wi) {
      ++h;
      hv = h < k ? hvs[lane][h] : -INFINITY;
      hi = h < k ? his[lane][h] : 0x7fffffff;
    }
  }
}

extern "C" long long vis_logprobs_ws_bytes(int V, int batch) {
  if (V <= 0 || V > LP_MAXCHUNKS * LP_CHUNK || batch < 1 || batch > LP_MAXBATCH) return 0;
  return (long long)batch * ((V + LP_CHUNK - 1) / LP_CHUNK) * LP_REC * 4;
}

extern "C" int vis_logprobs_f32(const void* logits, int V, int ld_logits, const void* tokens, int max_tokens,
                                const void* step_ptr, int top_k, void* lp, void* top_ids, void* ws, long long ws_bytes,
                                int batch, hipStream_t stream) {
  if (!logits || !tokens || !step_ptr || !lp || !top_ids || !ws) return VIS_ERR_ARG;
  if (V <= 0 || V > LP_MAXCHUNKS * LP_CHUNK || ld_logits < V || max_tokens <= 0) return VIS_ERR_ARG;
  if (batch < 1 || batch > LP_MAXBATCH || top_k < 0 || top_k > LP_MAXK || top_k > V) return VIS_ERR_ARG;
  if (ws_bytes < vis_logprobs_ws_bytes(V, batch)) return VIS_ERR_ARG;
  const int nchunks = (V + LP_CHUNK - 1) / LP_CHUNK;
  vis_clear_error();
  if (top_k > 0)
    hipLaunchKernelGGL(logprobs_stage1_kernel<true>, dim3(nchunks, batch), dim3(256), 0, stream, (const float*)logits, V,
                       ld_logits, (const int*)step_ptr, max_tokens, top_k, (float*)ws, nchunks);
  else
    hipLaunchKernelGGL(logprobs_stage1_kernel<false>, dim3(nchunks, batch), dim3(256), 0, stream, (const float*)logits, V,
                       ld_logits, (const int*)step_ptr, max_tokens, 0, (float*)ws, nchunks);
  hipLaunchKernelGGL(logprobs_stage2_kernel, dim3(batch), dim3(64), 0, stream, (const float*)logits, V, ld_logits,
                     (const int*)tokens, max_tokens, (const int*)step_ptr, top_k, (const float*)ws, nchunks, (float*)lp,
                     (int*)top_ids);
  return vis_check_launch();
}
