// Nucleus (top_p) sampling with per-row seeds (vis_sample_f32).  For row b with f32 logits l, allowed set A (every id, or
// the ids whose bit is set in allow[b * ld_allow + i / 64]), inverse temperature t = 1 / T and top_p p:
//   order A by (l desc, i asc) - the argmax tie rule; w_i = exp((l_i - m) t) with m = max over A, Z = sum of w over A;
//   K = the shortest prefix of that order whose mass >= p Z (at least one token; p = 1 keeps A, p = 0 the top token);
//   pick = argmax over K of l_i t + gumbel_noise(seeds[b], step[b], i), the expression and tie rule of vis_argmax_f32, so at
//   p = 1 the pick is vis_argmax_f32's bit for bit when seeds[b] is the seed that kernel derives for row b.
// t = 0 is the greedy pick over A (p ignored, nkeep = 1).  Effects are argmax_stage2's: tokens[step] = pick (when
// step < max_tokens), cur_token = pick, step += 1; a row with nothing allowed stores id 0.
//
// Masses are summed in 2^-40 fixed point (u64), so every sum is an integer sum: exact, independent of the order of the
// additions, hence deterministic and batch-invariant without any float atomic.  Per-element rounding is <= 2^-41 with Z >= 1
// (the top token weighs 1), i.e. the cut is the float64 one up to ~1e-7 Z at V = 152 064.
//
// Launch 1, sample_cut_kernel: one 1024-thread workgroup per row finds the cut key (v*, i*), K = {l > v*} + {l == v*, i <= i*}:
//   pass 1: m = max over A;
//   pass 2: LDS histogram of q_i = round(w_i 2^40) over 2048 bins of d = (m - l) t (width 1/64; q = 0 past d ~ 28.4, so
//           the bins cover every weighted element); a block scan finds the boundary bin and the mass before it;
//   pass 3: the boundary bin's members go to LDS (<= 1024 of them): each member's inclusive prefix mass within the bin by a
//           direct count, and the first member in order whose prefix reaches the target is the cut.
//   A boundary bin with more members (a large tie group, a constant row) is cut by bisection instead: on the value
//   (<= 32 passes over the row), then on the index inside the tie group at that value (<= 18 passes).  Slow, exact.
// Launch 2, sample_stage1_kernel: grid (nb, batch) Gumbel-max over K, per-workgroup (value, index) and |K| partials.
// Launch 3, sample_stage2_kernel: one wave per row merges them, stores the pick and nkeep.
#include "decode_common.hip.h"
#include <math.h>

#define SP_BINS 2048             // d bins of width 1 / 64: d in [0, 32)
#define SP_MEMBERS 1024          // boundary-bin members cut in LDS; more take the bisection path
#define SP_THREADS 1024
#define SP_NB 256                // stage-1 workgroups per row at most (argmax_stage1's grid)
#define SP_MAXBATCH 64
#define SP_ROW_BYTES (16 + SP_NB * 12)    // per row: cut (v*, i*), then bval[256], bidx[256], bcnt[256]

__device__ __forceinline__ bool sp_allowed(const unsigned long long* allow, int i) {
  return ((allow[i >> 6] >> (i & 63)) & 1ull) != 0;
}

// monotone map of a float to u32: a < b <=> key(a) < key(b) (no NaN)
__device__ __forceinline__ unsigned sp_fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_funkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// weight of logit l in 2^-40 fixed point, and its bin (-1: weightless)
__device__ __forceinline__ unsigned long long sp_q(float l, float m, float t, int& bin) {
  const float d = (m - l) * t;
  if (!(d >= 0.f)) { bin = -1; return 0; }        // NaN logits weigh nothing
  const float w = expf(-d);
  const unsigned long long q = (unsigned long long)rintf(w * 1099511627776.0f);
  bin = q ? min(SP_BINS - 1, (int)(d * 64.0f)) : -1;
  return q;
}

__device__ __forceinline__ unsigned long long sp_block_sum(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  unsigned long long s = 0;
  for (int w = 0; w < SP_THREADS / 64; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ unsigned long long sp_block_min(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, o, 64));
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  unsigned long long s = ~0ull;
  for (int w = 0; w < SP_THREADS / 64; ++w) s = min(s, red[w]);
  return s;
}

template <bool MASK>
__global__ __launch_bounds__(SP_THREADS) void sample_cut_kernel(const float* __restrict__ logits, int V, int ld_logits,
                                                                const unsigned long long* __restrict__ allow, int ld_allow,
                                                                float t, float top_p, unsigned char* __restrict__ ws) {
  const int tid = threadIdx.x, row = blockIdx.x;
  logits += (size_t)row * ld_logits;
  if (MASK) allow += (size_t)row * ld_allow;
  float* cut_v = (float*)(ws + (size_t)row * SP_ROW_BYTES);
  int* cut_i = (int*)(cut_v + 1);
  if (t == 0.f || top_p >= 1.f) {              // K = A
    if (tid == 0) { *cut_v = -INFINITY; *cut_i = 0x7fffffff; }
    return;
  }
  __shared__ unsigned long long hist[SP_BINS];
  __shared__ unsigned long long red[SP_THREADS / 64];
  __shared__ float mem_l[SP_MEMBERS];
  __shared__ int mem_i[SP_MEMBERS];
  __shared__ unsigned long long mem_q[SP_MEMBERS];
  __shared__ float s_max[SP_THREADS / 64];
  __shared__ int s_bin, s_cnt;
  __shared__ unsigned long long s_before;
  __shared__ unsigned s_klo, s_khi;

  // pass 1: m
  float m = -INFINITY;
  for (int i = tid; i < V; i += SP_THREADS) {
    if (MASK && !sp_allowed(allow, i)) continue;
    m = fmaxf(m, logits[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
  for (int b = tid; b < SP_BINS; b += SP_THREADS) hist[b] = 0;
  if (tid == 0) { s_cnt = 0; s_klo = 0xffffffffu; s_khi = 0; s_bin = -1; }
  __syncthreads();
  m = s_max[0];
  for (int w = 1; w < SP_THREADS / 64; ++w) m = fmaxf(m, s_max[w]);
  if (m == -INFINITY) {                        // nothing allowed: stage 1 finds nothing, stage 2 stores id 0
    if (tid == 0) { *cut_v = -INFINITY; *cut_i = 0x7fffffff; }
    return;
  }

  // pass 2: histogram of the fixed-point mass
  for (int i = tid; i < V; i += SP_THREADS) {
    if (MASK && !sp_allowed(allow, i)) continue;
    int bin;
    const unsigned long long q = sp_q(logits[i], m, t, bin);
    if (q) atomicAdd(&hist[bin], q);
  }
  __syncthreads();
  // block scan over the bins, two per thread in order
  const unsigned long long h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
  unsigned long long incl = h0 + h1;
  const int lane = tid & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) red[tid >> 6] = incl;
  __syncthreads();
  unsigned long long wave_before = 0, Z = 0;
  for (int w = 0; w < SP_THREADS / 64; ++w) {
    if (w < (tid >> 6)) wave_before += red[w];
    Z += red[w];
  }
  incl += wave_before;
  // target: the smallest prefix mass >= p Z, at least the top token (q = 2^40 > 1)
  unsigned long long target = (unsigned long long)ceil((double)top_p * (double)Z);
  if (target == 0) target = 1;
  if (target > Z) target = Z;
  {
    const unsigned long long before = incl - h0 - h1;
    if (before < target && target <= before + h0) { s_bin = 2 * tid; s_before = before; }
    else if (before + h0 < target && target <= incl) { s_bin = 2 * tid + 1; s_before = before + h0; }
  }
  __syncthreads();
  const int bb = s_bin;
  const unsigned long long R = target - s_before;      // mass still needed inside bin bb (> 0)

  // pass 3: gather the boundary bin's members
  for (int i = tid; i < V; i += SP_THREADS) {
    if (MASK && !sp_allowed(allow, i)) continue;
    const float l = logits[i];
    int bin;
    const unsigned long long q = sp_q(l, m, t, bin);
    if (bin != bb) continue;
    const int pos = atomicAdd(&s_cnt, 1);
    if (pos < SP_MEMBERS) { mem_l[pos] = l; mem_i[pos] = i; mem_q[pos] = q; }
    const unsigned k = sp_fkey(l);
    atomicMin(&s_klo, k);
    atomicMax(&s_khi, k);
  }
  __syncthreads();
  const int n = s_cnt;
  if (n <= SP_MEMBERS) {
    // order key: l descending, then i ascending
    unsigned long long best = ~0ull;
    if (tid < n) {
      const float lj = mem_l[tid];
      const int ij = mem_i[tid];
      unsigned long long S = 0;
      for (int k = 0; k < n; ++k) {
        const float lk = mem_l[k];
        if (lk > lj || (lk == lj && mem_i[k] <= ij)) S += mem_q[k];
      }
      if (S >= R) best = ((unsigned long long)(~sp_fkey(lj)) << 32) | (unsigned)ij;
    }
    best = sp_block_min(best, red);
    if (tid == 0) { *cut_v = sp_funkey(~(unsigned)(best >> 32)); *cut_i = (int)(unsigned)(best & 0xffffffffu); }
    return;
  }

  // bisection: the largest value key u with mass(members, key >= u) >= R is the cut value v*
  unsigned lo = s_klo, hi = s_khi;
  while (lo < hi) {
    const unsigned mid = lo + (hi - lo + 1) / 2;
    unsigned long long s = 0;
    for (int i = tid; i < V; i += SP_THREADS) {
      if (MASK && !sp_allowed(allow, i)) continue;
      const float l = logits[i];
      int bin;
      const unsigned long long q = sp_q(l, m, t, bin);
      if (bin == bb && sp_fkey(l) >= mid) s += q;
    }
    if (sp_block_sum(s, red) >= R) lo = mid; else hi = mid - 1;
  }
  const float vs = sp_funkey(lo);
  // mass of the members above v*, and the weight and count of the tie group at v*
  unsigned long long above = 0, ties = 0;
  int bin_v;
  const unsigned long long qv = sp_q(vs, m, t, bin_v);
  for (int i = tid; i < V; i += SP_THREADS) {
    if (MASK && !sp_allowed(allow, i)) continue;
    const float l = logits[i];
    int bin;
    const unsigned long long q = sp_q(l, m, t, bin);
    if (bin != bb) continue;
    if (l > vs) above += q; else if (l == vs) ties += 1;
  }
  above = sp_block_sum(above, red);
  ties = sp_block_sum(ties, red);
  unsigned long long need = (R - above + qv - 1) / qv;  // ties to keep, >= 1 (the mass above v* is < R)
  if (need > ties) need = ties;
  // the need-th smallest index in the tie group
  int ilo = 0, ihi = V - 1;
  while (ilo < ihi) {
    const int mid = ilo + (ihi - ilo) / 2;
    unsigned long long c = 0;
    for (int i = tid; i <= mid; i += SP_THREADS) {
      if (MASK && !sp_allowed(allow, i)) continue;
      if (logits[i] == vs) c += 1;
    }
    if (sp_block_sum(c, red) >= need) ihi = mid; else ilo = mid + 1;
  }
  if (tid == 0) { *cut_v = vs; *cut_i = ilo; }
}

// Gumbel-max over K (argmax_stage1_body's loop with K's test in front), plus |K| per workgroup
template <bool MASK>
__global__ __launch_bounds__(256) void sample_stage1_kernel(const float* __restrict__ logits, int V, int ld_logits,
                                                            const unsigned long long* __restrict__ allow, int ld_allow,
                                                            float inv_temp, const unsigned* __restrict__ seeds,
                                                            const int* __restrict__ step_ptr, unsigned char* __restrict__ ws) {
  const int tid = threadIdx.x, seq = blockIdx.y;
  logits += (size_t)seq * ld_logits;
  if (MASK) allow += (size_t)seq * ld_allow;
  unsigned char* rw = ws + (size_t)seq * SP_ROW_BYTES;
  const float cv = ((const float*)rw)[0];
  const int ci = ((const int*)rw)[1];
  float* bval = (float*)(rw + 16);
  int* bidx = (int*)(bval + SP_NB);
  int* bcnt = bidx + SP_NB;
  const unsigned seed = seeds[seq];
  const unsigned step = (unsigned)step_ptr[seq];
  float best = -INFINITY;
  int bi = 0x7fffffff, cnt = 0;
  for (int i = blockIdx.x * 256 + tid; i < V; i += gridDim.x * 256) {
    if (MASK && !sp_allowed(allow, i)) continue;
    float v = logits[i];
    if (!(v > cv || (v == cv && i <= ci))) continue;
    ++cnt;
    if (inv_temp > 0.f) v = v * inv_temp + gumbel_noise(seed, step, (unsigned)i);
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    cnt += __shfl_xor(cnt, o, 64);
  }
  __shared__ float sv[4];
  __shared__ int si[4], sc[4];
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; sc[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
      cnt += sc[w];
    }
    bval[blockIdx.x] = best;
    bidx[blockIdx.x] = bi;
    bcnt[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(64) void sample_stage2_kernel(const unsigned char* __restrict__ ws, int nb, float inv_temp,
                                                           int* __restrict__ tokens, int max_tokens, int* __restrict__ cur_token,
                                                           int* __restrict__ step_ptr, int* __restrict__ nkeep) {
  const int lane = threadIdx.x, seq = blockIdx.x;
  const unsigned char* rw = ws + (size_t)seq * SP_ROW_BYTES;
  const float* bval = (const float*)(rw + 16);
  const int* bidx = (const int*)(bval + SP_NB);
  const int* bcnt = bidx + SP_NB;
  tokens += (size_t)seq * max_tokens;
  float best = -INFINITY;
  int bi = 0x7fffffff, cnt = 0;
  for (int i = lane; i < nb; i += 64) {
    const float v = bval[i];
    const int ix = bidx[i];
    if (v > best || (v == best && ix < bi)) { best = v; bi = ix; }
    cnt += bcnt[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) {
    if (bi == 0x7fffffff) bi = 0;
    const int st = step_ptr[seq];
    if (st < max_tokens) tokens[st] = bi;
    cur_token[seq] = bi;
    step_ptr[seq] = st + 1;
    if (nkeep) nkeep[seq] = (inv_temp > 0.f) ? cnt : min(cnt, 1);
  }
}

extern "C" long long vis_sample_ws_bytes(int V, int batch) {
  if (V <= 0 || batch <= 0 || batch > SP_MAXBATCH) return 0;
  return (long long)batch * SP_ROW_BYTES;
}

extern "C" int vis_sample_f32(const void* logits, int V, int ld_logits, const void* allow, int ld_allow, float inv_temp,
                              float top_p, const void* seeds, void* tokens, int max_tokens, void* cur_token, void* step_ptr,
                              int batch, void* ws, void* nkeep, hipStream_t stream) {
  if (!logits || !seeds || !tokens || !cur_token || !step_ptr || !ws || V <= 0) return VIS_ERR_ARG;
  if (batch <= 0 || batch > SP_MAXBATCH || (batch > 1 && ld_logits < V)) return VIS_ERR_ARG;
  if (!(top_p >= 0.f && top_p <= 1.f) || !(inv_temp >= 0.f)) return VIS_ERR_ARG;
  if (allow && (ld_allow < (V + 63) / 64 || (((uintptr_t)allow) & 7))) return VIS_ERR_ARG;
  if (batch == 1) ld_logits = V;
  const int nb = min(SP_NB, (V + 255) / 256);
  const unsigned long long* a = (const unsigned long long*)allow;
  vis_clear_error();
  if (a) {
    hipLaunchKernelGGL(sample_cut_kernel<true>, dim3(batch), dim3(SP_THREADS), 0, stream, (const float*)logits, V, ld_logits,
                       a, ld_allow, inv_temp, top_p, (unsigned char*)ws);
    hipLaunchKernelGGL(sample_stage1_kernel<true>, dim3(nb, batch), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                       a, ld_allow, inv_temp, (const unsigned*)seeds, (const int*)step_ptr, (unsigned char*)ws);
  } else {
    hipLaunchKernelGGL(sample_cut_kernel<false>, dim3(batch), dim3(SP_THREADS), 0, stream, (const float*)logits, V,
                       ld_logits, a, 0, inv_temp, top_p, (unsigned char*)ws);
    hipLaunchKernelGGL(sample_stage1_kernel<false>, dim3(nb, batch), dim3(256), 0, stream, (const float*)logits, V,
                       ld_logits, a, 0, inv_temp, (const unsigned*)seeds, (const int*)step_ptr, (unsigned char*)ws);
  }
  hipLaunchKernelGGL(sample_stage2_kernel, dim3(batch), dim3(64), 0, stream, (const unsigned char*)ws, nb, inv_temp,
                     (int*)tokens, max_tokens, (int*)cur_token, (int*)step_ptr, (int*)nkeep);
  return vis_check_launch();
}
