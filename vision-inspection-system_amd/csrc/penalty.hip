// Logit penalties (vis_penalty_prompt, vis_penalize_f32): repetition penalty (transformers' RepetitionPenaltyLogitsProcessor)
// and OpenAI's frequency / presence penalties, applied to a row of raw f32 logits ahead of the pick.
//
// State of one row (one in-flight sequence), PN_HEAD_BYTES + 2 * roundup(V, 8) bytes, zeroed = fresh:
//   int32 head[4] = {pos, anchored, ticket, -}     pos: the token positions [.., pos) are folded into the counts
//   uint16 word[roundup(V, 8)]                      bit 15: the id is in the prompt; bits 0..14: times generated (saturating)
// A 16-bit word instead of 32: the kernel is a stream of x (4 B) + word (2 B) in and y (4 B) out, 10 bytes per id instead
// of 12; a count saturated at 32767 is beyond any context this library serves.
//
// vis_penalize_f32, one launch per pick, grid (chunks of V, batch), 256 threads, four ids per lane and iteration (one
// dwordx4 load of x, one dwordx2 load of the words, one dwordx4 store of y).  Every workgroup reads pos and step: the tokens
// picked since the state was advanced are positions max(pos, 0) .. step - 1 of the row's token buffer (none on the first
// launch after a reset, which anchors pos at step; one in steady state).  The lane that owns id v counts v's occurrences
// among them, adds that to its word, writes the word back (only when it changed) and uses the new value - one owner per
// id, so no atomics and no second launch.  The last workgroup of a row to finish (a ticket in the head) stores pos = step:
// by then every workgroup of the row has read the old pos.  A launch repeated at the same step (graph warm-up before
// capture) finds pos == step, folds nothing and writes the same y.
//
//   seen = prompt bit or c > 0
//   y = x                               if not seen or r == 1
//   y = x < 0 ? x * r : x / r           otherwise
//   y = y - (f * c + q)                 if c > 0
// (r, f, q) of row b = params[3 b ..] in device memory, read at run time: a captured launch serves any values.  A row's y
// depends on its own x, words and parameters only: bit-identical at any batch size and slot.  The neutral triple (1, 0, 0)
// and unseen ids copy x bit for bit.
#include "common.hip.h"

#define PN_MAXV 262144
#define PN_MAXBATCH 64
#define PN_HEAD_BYTES 16
#define PN_PROMPT 0x8000u
#define PN_CMAX 0x7FFFu
enum { PH_POS, PH_ANCHOR, PH_TICKET };

static inline long long pn_row_bytes(int V) { return PN_HEAD_BYTES + 2ll * ((V + 7) / 8 * 8); }

__global__ __launch_bounds__(256) void penalty_prompt_kernel(unsigned* __restrict__ words32, int V, const int* __restrict__ ids,
                                                             int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int id = ids[i];
    if (id >= 0 && id < V) atomicOr(&words32[id >> 1], PN_PROMPT << (16 * (id & 1)));   // many lanes, one id: same bit
  }
}

__device__ __forceinline__ float pn_value(float x, unsigned w, float r, float f, float q) {
  const unsigned c = w & PN_CMAX;
  float y = x;
  if (w != 0 && r != 1.0f) y = x < 0.0f ? x * r : x / r;
  // f c + q in one rounding (fma), then one subtraction: with the multiply / divide above at most three roundings, two of them
  // of a part of the result - within 2^-23 of (|x| max(r, 1 / r) + |f| c + |q|)
  if (c != 0 && (f != 0.0f || q != 0.0f)) y = y - fmaf(f, (float)c, q);
  return y;
}

// word of id `id` after folding toks[p0 .. p1); `changed` is set when it differs from w
__device__ __forceinline__ unsigned pn_fold(unsigned w, int id, const int* __restrict__ toks, int p0, int p1, bool& changed) {
  unsigned add = 0;
  for (int p = p0; p < p1; ++p) add += toks[p] == id;
  if (add == 0) return w;
  changed = true;
  return (w & PN_PROMPT) | min((w & PN_CMAX) + add, PN_CMAX);
}

template <bool VEC>
__global__ __launch_bounds__(256) void penalize_kernel(const float* __restrict__ logits, int V, int ld_logits,
                                                       unsigned char* __restrict__ state, long long row_bytes,
                                                       const float* __restrict__ params, const int* __restrict__ tokens,
                                                       int max_tokens, const int* __restrict__ step_ptr,
                                                       float* __restrict__ out, int ld_out) {
  const int row = blockIdx.y, tid = threadIdx.x;
  unsigned char* __restrict__ st = state + (size_t)row * row_bytes;
  int* head = (int*)st;
  unsigned short* __restrict__ words = (unsigned short*)(st + PN_HEAD_BYTES);
  const int step = step_ptr[row];
  const int p1 = min(step, max_tokens);
  const int p0 = head[PH_ANCHOR] ? max(head[PH_POS], 0) : p1;
  const int* __restrict__ toks = tokens + (size_t)row * max_tokens;
  const float r = params[3 * row], f = params[3 * row + 1], q = params[3 * row + 2];
  const float* __restrict__ x = logits + (size_t)row * ld_logits;
  float* __restrict__ y = out + (size_t)row * ld_out;

  const int ngroups = (V + 3) >> 2;
  for (int g = blockIdx.x * 256 + tid; g < ngroups; g += gridDim.x * 256) {
    const int v0 = g * 4;
    if (VEC && v0 + 4 <= V) {
      const f32x4 xv = *(const f32x4*)(x + v0);
      const u32x2 wv = *(const u32x2*)(words + v0);
      unsigned w[4] = {wv[0] & 0xFFFFu, wv[0] >> 16, wv[1] & 0xFFFFu, wv[1] >> 16};
      bool changed = false;
      f32x4 yv;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = pn_fold(w[k], v0 + k, toks, p0, p1, changed);
        yv[k] = pn_value(xv[k], w[k], r, f, q);
      }
      if (changed) {
        u32x2 nw = {w[0] | (w[1] << 16), w[2] | (w[3] << 16)};
        *(u32x2*)(words + v0) = nw;
      }
      *(f32x4*)(y + v0) = yv;
    } else {
      for (int v = v0; v < min(v0 + 4, V); ++v) {
        bool changed = false;
        const unsigned w = pn_fold(words[v], v, toks, p0, p1, changed);
        if (changed) words[v] = (unsigned short)w;
        y[v] = pn_value(x[v], w, r, f, q);
      }
    }
  }

  // Every thread of this workgroup has read the old pos (the barrier); the row's last workgroup advances it.  The ticket is
  // a relaxed atomic and no fence surrounds it: nothing written here is read by this launch (the next one sees it across the
  // kernel boundary), and a device-scope fence per workgroup would write the L2 back 8192 times at 64 rows.
  __syncthreads();
  if (tid == 0) {
    if (atomicAdd(&head[PH_TICKET], 1) == (int)gridDim.x - 1) {
      head[PH_POS] = step;
      head[PH_ANCHOR] = 1;
      head[PH_TICKET] = 0;
    }
  }
}

extern "C" long long vis_penalty_state_bytes(int V, int batch) {
  if (V <= 0 || V > PN_MAXV || batch < 1 || batch > PN_MAXBATCH) return 0;
  return pn_row_bytes(V) * batch;
}

extern "C" int vis_penalty_prompt(void* state_row, int V, const void* ids, int n, hipStream_t stream) {
  if (!state_row || !ids || V <= 0 || V > PN_MAXV || n < 0 || ((uintptr_t)state_row & 15) || ((uintptr_t)ids & 3))
    return VIS_ERR_ARG;
  if (n == 0) return VIS_OK;
  vis_clear_error();
  hipLaunchKernelGGL(penalty_prompt_kernel, dim3(min((n + 255) / 256, 64)), dim3(256), 0, stream,
                     (unsigned*)((unsigned char*)state_row + PN_HEAD_BYTES), V, (const int*)ids, n);
  return vis_check_launch();
}

extern "C" int vis_penalize_f32(const void* logits, int V, int ld_logits, void* state, const void* params, const void* tokens,
                                int max_tokens, const void* step_ptr, void* out, int ld_out, int batch, hipStream_t stream) {
  if (!logits || !state || !params || !tokens || !step_ptr || !out) return VIS_ERR_ARG;
  if (V <= 0 || V > PN_MAXV || batch < 1 || batch > PN_MAXBATCH || max_tokens <= 0) return VIS_ERR_ARG;
  if (batch > 1 && (ld_logits < V || ld_out < V)) return VIS_ERR_ARG;
  if (((uintptr_t)state & 15) || ((uintptr_t)logits & 3) || ((uintptr_t)out & 3) || ((uintptr_t)params & 3)) return VIS_ERR_ARG;
  if (logits == out) return VIS_ERR_ARG;                  // the raw row stays intact (logprobs read it after the pick)
  const bool vec = !((uintptr_t)logits & 15) && !((uintptr_t)out & 15) && (batch == 1 || (ld_logits % 4 == 0 && ld_out % 4 == 0));
  // 1024 ids per workgroup and iteration; past ~8 workgroups per CU over the batch the rows are grid-strided
  int blocks = (V + 1023) / 1024;
  const int cap = max(1, 8192 / batch);
  if (blocks > cap) blocks = cap;
  vis_clear_error();
  if (vec)
    hipLaunchKernelGGL(penalize_kernel<true>, dim3(blocks, batch), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                       (unsigned char*)state, pn_row_bytes(V), (const float*)params, (const int*)tokens, max_tokens,
                       (const int*)step_ptr, (float*)out, ld_out);
  else
    hipLaunchKernelGGL(penalize_kernel<false>, dim3(blocks, batch), dim3(256), 0, stream, (const float*)logits, V, ld_logits,
                       (unsigned char*)state, pn_row_bytes(V), (const float*)params, (const int*)tokens, max_tokens,
                       (const int*)step_ptr, (float*)out, ld_out);
  return vis_check_launch();
}
