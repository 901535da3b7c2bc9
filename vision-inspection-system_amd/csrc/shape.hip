// Logit shaping ahead of the pick (vis_shape_f32): logit_bias (OpenAI's), top_k and min_p (transformers' TopKLogitsWarper /
// MinPLogitsWarper) applied to a row of f32 logits.  The pick kernels that follow read the shaped copy; the input row stays
// intact.  For row b with allowed set A (every id, or the ids whose bit is set in allow[b * ld_allow + i / 64]):
//   y[v] = x[v] + bias[v] for the ids of the row's bias list (one f32 add), x[v] for every other id;
//   m = max y over A;  t = the k-th largest y over A when 0 < k < |A|, else nothing is cut by rank;
//   v survives when it is in A, y[v] >= t (ties at t all stay) and not (y[v] - m) < delta   (f32 subtraction and compare);
//   out[v] = y[v] for survivors (bit for bit), -inf for every other id; nkept = the number of survivors.
// delta = ln(min_p) / inv_temp is computed by the host (-inf = off).  Comparisons are float comparisons: -0.0 == +0.0.
// k, delta and the bias list of row b are read from device memory at run time: a captured launch serves any values.
//
// One 1024-thread workgroup per row; every pass reads the input row (just written by the lm_head: L2) and recomputes y, so
// nothing the workgroup stores to global memory is ever read back by it:
//   setup:  the bias list goes to LDS with a V-bit map of the ids that carry one - an element pays one LDS bit test, and the
//           search through the list only where the bit is set;
//   pass 1: max, min and |A|                       (skipped when neither top_k nor min_p is on);
//   pass 2: LDS histogram of bin(y) = floor((m - y) * 2047 / (m - min)) over 2048 bins.  The bin is a monotone function of y
//           (every float operation in it is), so a lower bin holds strictly larger values and the k-th largest lies in the
//           bin where the running count passes k.  Linear bins spread a row of logits over the whole histogram, where the top
//           bits of the float key would put it into a few dozen words of LDS atomics;
//   pass 3: that bin's members go to LDS (<= 1024 of them) and the wanted one is found by direct rank counting.  A bin with
//           more members (a tie run, a constant row) is cut by an exact radix select instead: three histogram passes over
//           the bin's members on the order-preserving 32-bit key, 11 + 11 + 10 bits, with both zeros mapped to one key;
//   final:  writes the row and counts the survivors.
// Passes 2 and 3 run only when 0 < k < |A|.  A row's result depends on that row alone: bit-identical at any batch size and
// slot.  No workgroup waits for another, nothing is carried from launch to launch, a repeated launch rewrites the same bytes.
// Per row the workspace receives a 16-byte record {t, m, |A|, path}: path 0 = no rank cut, 1 = LDS rank count, 2 = radix.
#include "common.hip.h"
#include <math.h>

#define SH_MAXV 262144
#define SH_MAXBATCH 64
#define SH_MAXBIAS 300
#define SH_THREADS 1024
#define SH_WAVES (SH_THREADS / 64)
#define SH_BINS 2048
#define SH_MEMBERS 1024
#define SH_ROW_BYTES 16

// order-preserving key of a float (no NaN), -0.0 and +0.0 on one key
__device__ __forceinline__ unsigned sh_key(float f) {
  const unsigned u = (f == 0.0f) ? 0u : __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sh_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct ShSrc {
  const float* x;                       // the row
  const unsigned long long* allow;      // its allow words or null
  int V;
  bool vec;                             // the row may be read 16 bytes at a time
  const unsigned* bmap;                 // LDS: bit v set = id v is in the bias list
  const int* bid;                       // LDS: the list's ids (-1: skipped)
  const float* bval;
  int nb;
};

// y of ids v0 .. v0 + 3 (v0 a multiple of 4, below V); returns the 4-bit mask of those that exist and are in A
__device__ __forceinline__ unsigned sh_load4(const ShSrc& s, int v0, float* y) {
  unsigned in;
  if (s.vec && v0 + 4 <= s.V) {
    const f32x4 xv = *(const f32x4*)(s.x + v0);
    y[0] = xv[0]; y[1] = xv[1]; y[2] = xv[2]; y[3] = xv[3];
    in = 0xFu;
  } else {
    in = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = v0 + k < s.V;
      y[k] = ok ? s.x[v0 + k] : 0.0f;
      in |= (unsigned)ok << k;
    }
  }
  if (s.allow) in &= (unsigned)(s.allow[v0 >> 6] >> (v0 & 63));
  if (s.nb) {
    unsigned w = (s.bmap[v0 >> 5] >> (v0 & 31)) & 0xFu;
    while (w) {
      const int k = __ffs(w) - 1;
      w &= w - 1;
      for (int j = 0; j < s.nb; ++j)
        if (s.bid[j] == v0 + k) { y[k] = y[k] + s.bval[j]; break; }       // the first entry of an id counts
    }
  }
  return in;
}

__device__ __forceinline__ float sh_block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < SH_WAVES; ++w) r = fmaxf(r, red[w]);
  return r;
}

__device__ __forceinline__ unsigned sh_block_sum(unsigned v, unsigned* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned r = 0;
  for (int w = 0; w < SH_WAVES; ++w) r += red[w];
  return r;
}

// the bin where the running count over hist[0 .. SH_BINS) passes k (1 <= k <= the total), and the count before it
__device__ __forceinline__ void sh_find_bin(const unsigned* hist, unsigned k, unsigned* red, int* s_bin, unsigned* s_before) {
  const int tid = threadIdx.x, lane = tid & 63;
  __syncthreads();                             // the histogram is complete, red is free
  const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
  unsigned incl = h0 + h1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) red[tid >> 6] = incl;
  __syncthreads();
  for (int w = 0; w < (tid >> 6); ++w) incl += red[w];
  const unsigned before = incl - h0 - h1;
  if (before < k && k <= before + h0) { *s_bin = 2 * tid; *s_before = before; }
  else if (before + h0 < k && k <= incl) { *s_bin = 2 * tid + 1; *s_before = before + h0; }
  __syncthreads();
}

__device__ __forceinline__ int sh_bin(float y, float m, float scale) {
  const float d = (m - y) * scale;
  return min(SH_BINS - 1, max(0, (int)d));
}

__global__ __launch_bounds__(SH_THREADS) void shape_kernel(const float* __restrict__ logits, int V, int ld_logits,
                                                           const unsigned long long* __restrict__ allow, int ld_allow,
                                                           const int* __restrict__ kk, const float* __restrict__ deltas,
                                                           const int* __restrict__ nbias, const int* __restrict__ bias_ids,
                                                           const float* __restrict__ bias_vals, float* __restrict__ out,
                                                           int ld_out, int* __restrict__ nkept, unsigned char* __restrict__ ws,
                                                           int vec_in, int vec_out) {
  __shared__ unsigned bmap[SH_MAXV / 32];
  __shared__ unsigned hist[SH_BINS];
  __shared__ float mem[SH_MEMBERS];
  __shared__ int bid[SH_MAXBIAS];
  __shared__ float bval[SH_MAXBIAS];
  __shared__ float red_f[SH_WAVES];
  __shared__ unsigned red_u[SH_WAVES];
  __shared__ int s_bin;
  __shared__ unsigned s_before, s_cnt;
  __shared__ float s_t;

  const int tid = threadIdx.x, row = blockIdx.x;
  const int ngroups = (V + 3) >> 2;
  float* __restrict__ y_out = out + (size_t)row * ld_out;
  const int k = kk[row];
  const float delta = deltas[row];
  const int nb = min(max(nbias[row], 0), SH_MAXBIAS);

  // setup: the bias list and the map of its ids
  if (nb) {
    for (int w = tid; w < (V + 31) >> 5; w += SH_THREADS) bmap[w] = 0;
    __syncthreads();
    if (tid < nb) {
      const int id = bias_ids[(size_t)row * SH_MAXBIAS + tid];
      const bool ok = id >= 0 && id < V;                 // ids outside the vocabulary are skipped
      bid[tid] = ok ? id : -1;
      bval[tid] = bias_vals[(size_t)row * SH_MAXBIAS + tid];
      if (ok) atomicOr(&bmap[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  const ShSrc src = {logits + (size_t)row * ld_logits, allow ? allow + (size_t)row * ld_allow : nullptr, V, vec_in != 0,
                     bmap, bid, bval, nb};
  float y[4];

  const bool minp_on = delta > -INFINITY;
  const bool rank_asked = k > 0 && k < V;
  float m = 0.0f, t = -INFINITY;
  unsigned cntA = 0;
  int path = 0;
  if (minp_on || rank_asked) {
    // pass 1
    float mx = -INFINITY, nmn = -INFINITY;
    unsigned c = 0;
    for (int g = tid; g < ngroups; g += SH_THREADS) {
      const unsigned in = sh_load4(src, g * 4, y);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((in >> e) & 1u) { mx = fmaxf(mx, y[e]); nmn = fmaxf(nmn, -y[e]); ++c; }
    }
    m = sh_block_max(mx, red_f);
    const float mn = -sh_block_max(nmn, red_f);
    cntA = sh_block_sum(c, red_u);

    if (rank_asked && (unsigned)k < cntA) {
      const float range = m - mn;
      const float scale = (range > 0.0f && range < INFINITY) ? (float)(SH_BINS - 1) / range : 0.0f;
      // pass 2
      for (int b = tid; b < SH_BINS; b += SH_THREADS) hist[b] = 0;
      if (tid == 0) s_cnt = 0;
      __syncthreads();
      for (int g = tid; g < ngroups; g += SH_THREADS) {
        const unsigned in = sh_load4(src, g * 4, y);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((in >> e) & 1u) atomicAdd(&hist[sh_bin(y[e], m, scale)], 1u);
      }
      sh_find_bin(hist, (unsigned)k, red_u, &s_bin, &s_before);
      const int bb = s_bin;
      unsigned need = (unsigned)k - s_before;            // the need-th largest member of bin bb, >= 1
      // pass 3
      for (int g = tid; g < ngroups; g += SH_THREADS) {
        const unsigned in = sh_load4(src, g * 4, y);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (((in >> e) & 1u) && sh_bin(y[e], m, scale) == bb) {
            const unsigned pos = atomicAdd(&s_cnt, 1u);
            if (pos < SH_MEMBERS) mem[pos] = y[e];
          }
      }
      __syncthreads();
      const unsigned n = s_cnt;
      if (n <= SH_MEMBERS) {
        path = 1;
        if ((unsigned)tid < n) {
          const float yj = mem[tid];
          unsigned gt = 0, ge = 0;
          for (unsigned i = 0; i < n; ++i) {
            const float yi = mem[i];
            gt += yi > yj;
            ge += yi >= yj;
          }
          if (gt < need && need <= ge) s_t = (yj == 0.0f) ? 0.0f : yj;     // tied members store the same value
        }
        __syncthreads();
        t = s_t;
      } else {
        path = 2;
        // the need-th smallest inverted key among the bin's members, most significant digit first
        unsigned prefix = 0;
#pragma unroll 1
        for (int p = 0; p < 3; ++p) {
          const int shift = p == 0 ? 21 : (p == 1 ? 10 : 0);
          const int bits = p == 2 ? 10 : 11;
          __syncthreads();                               // the previous round's histogram has been read
          for (int b = tid; b < SH_BINS; b += SH_THREADS) hist[b] = 0;
          __syncthreads();
          for (int g = tid; g < ngroups; g += SH_THREADS) {
            const unsigned in = sh_load4(src, g * 4, y);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (((in >> e) & 1u) && sh_bin(y[e], m, scale) == bb) {
                const unsigned ik = ~sh_key(y[e]);
                if (p == 0 || (ik >> (shift + bits)) == prefix) atomicAdd(&hist[(ik >> shift) & ((1u << bits) - 1u)], 1u);
              }
          }
          sh_find_bin(hist, need, red_u, &s_bin, &s_before);
          need -= s_before;
          prefix = (prefix << bits) | (unsigned)s_bin;
        }
        t = sh_unkey(~prefix);
      }
    }
  }

  // final pass
  unsigned kept = 0;
  for (int g = tid; g < ngroups; g += SH_THREADS) {
    const int v0 = g * 4;
    const unsigned in = sh_load4(src, v0, y);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool keep = ((in >> e) & 1u) && y[e] >= t && !(minp_on && (y[e] - m) < delta);
      o[e] = keep ? y[e] : -INFINITY;
      kept += keep;
    }
    if (vec_out && v0 + 4 <= V) {
      const f32x4 ov = {o[0], o[1], o[2], o[3]};
      *(f32x4*)(y_out + v0) = ov;
    } else {
      for (int e = 0; e < 4 && v0 + e < V; ++e) y_out[v0 + e] = o[e];
    }
  }
  kept = sh_block_sum(kept, red_u);
  if (tid == 0) {
    nkept[row] = (int)kept;
    float* rec = (float*)(ws + (size_t)row * SH_ROW_BYTES);
    rec[0] = t;
    rec[1] = m;
    ((int*)rec)[2] = (int)cntA;
    ((int*)rec)[3] = path;
  }
}

extern "C" long long vis_shape_ws_bytes(int V, int batch) {
  if (V <= 0 || V > SH_MAXV || batch < 1 || batch > SH_MAXBATCH) return 0;
  return (long long)batch * SH_ROW_BYTES;
}

extern "C" int vis_shape_f32(const void* logits, int V, int ld_logits, const void* allow, int ld_allow, const void* k,
                             const void* delta, const void* nbias, const void* bias_ids, const void* bias_vals, void* out,
                             int ld_out, void* nkept, void* ws, int batch, hipStream_t stream) {
  if (!logits || !k || !delta || !nbias || !bias_ids || !bias_vals || !out || !nkept || !ws) return VIS_ERR_ARG;
  if (V <= 0 || V > SH_MAXV || batch < 1 || batch > SH_MAXBATCH) return VIS_ERR_ARG;
  if (batch > 1 && (ld_logits < V || ld_out < V)) return VIS_ERR_ARG;
  if (allow && (ld_allow < (V + 63) / 64 || ((uintptr_t)allow & 7))) return VIS_ERR_ARG;
  if (((uintptr_t)logits & 3) || ((uintptr_t)out & 3) || ((uintptr_t)k & 3) || ((uintptr_t)delta & 3) || ((uintptr_t)nbias & 3) ||
      ((uintptr_t)bias_ids & 3) || ((uintptr_t)bias_vals & 3) || ((uintptr_t)nkept & 3) || ((uintptr_t)ws & 3))
    return VIS_ERR_ARG;
  if (logits == out) return VIS_ERR_ARG;                  // the input row stays intact (every pass reads it again)
  if (batch == 1) { ld_logits = V; ld_out = V; }
  const int vec_in = !((uintptr_t)logits & 15) && (batch == 1 || ld_logits % 4 == 0);
  const int vec_out = !((uintptr_t)out & 15) && (batch == 1 || ld_out % 4 == 0);
  vis_clear_error();
  hipLaunchKernelGGL(shape_kernel, dim3(batch), dim3(SH_THREADS), 0, stream, (const float*)logits, V, ld_logits,
                     (const unsigned long long*)allow, ld_allow, (const int*)k, (const float*)delta, (const int*)nbias,
                     (const int*)bias_ids, (const float*)bias_vals, (float*)out, ld_out, (int*)nkept, (unsigned char*)ws,
                     vec_in, vec_out);
  return vis_check_launch();
}
