// Token bans ahead of the pick (vis_ban_f32): the three request switches that depend on the SEQUENCE of tokens rather than on
// single ids - no_repeat_ngram_size (transformers' NoRepeatNGramLogitsProcessor), bad_words (transformers'
// NoBadWordsLogitsProcessor, vLLM's bad_words) and min_tokens (vLLM's) - applied to a row of f32 logits.  The pick kernels
// that follow read the copy; the input row stays intact.  ban.py holds the numpy restatement the tests compare against.
//
// History of row b: h = prompt[b][0 .. plen[b]) followed by tokens[b][gen0[b] .. step[b]), length L; the generated part has
// G = step[b] - gen0[b] ids (the prompt pass's pick included once it is stored).  An id is banned when
//   n-gram, n = ngram[b] >= 1:  for some i with i + n - 1 < L: h[i .. i+n-2] == h[L-n+1 .. L-1] and id == h[i+n-1]
//                               (n = 1: every id of h; L < n: nothing);
//   bad word w of m ids:        id == w[m-1] and (m == 1 or (L >= m-1 and h[L-m+1 .. L-1] == w[0 .. m-2])) - a match may
//                               straddle the prompt / generated boundary;
//   min_tokens:                 G < min_tokens[b] and id is one of the EOS ids.
// out[b][v] = -inf for banned v in [0, V), logits[b][v] bit for bit for every other v.  Ids outside [0, V) in the history
// take part in the comparisons (mllama's image token has the id V) and are never written.
//
// ngram, min_tokens, plen, gen0 and step are read from device memory per row, the words' ids and the EOS ids from device
// tables: a batch may mix values and a captured launch serves any of them.  The NUMBER of words, their lengths and the
// number of EOS ids are launch arguments (the host checks them): they are part of what a captured launch is.
//
// Grid (chunks of V, batch), 256 threads.  A workgroup owns the ids [lo, hi) of its row: it copies them (four ids per lane
// and iteration, dwordx4 where the rows allow it), waits for its stores and passes a workgroup barrier, then scans the whole
// history with its lanes - at most the context length, so neither a sort nor a hash - and stores -inf to the banned ids
// that fall into [lo, hi).  Every address of out is thus written by one workgroup only, copy first, ban second.  The scan
// is repeated by each workgroup of the row: it reads a few KB that stay in the cache, the copy moves 8 bytes per id.
// Nothing is carried from launch to launch; a repeated launch rewrites the same bytes.
#include "common.hip.h"
#include <math.h>

#define BN_MAXV 262144
#define BN_MAXBATCH 64
#define BN_MAXWORDS 16
#define BN_MAXWORDLEN 8
#define BN_MAXEOS 8
#define BN_THREADS 256

struct BanWords {
  int n;                                  // words in use
  unsigned char len[BN_MAXWORDS];         // ids of word w (1..8)
};

__global__ __launch_bounds__(BN_THREADS) void ban_kernel(const float* __restrict__ logits, int V, int ld_logits,
                                                         const int* __restrict__ prompt, int ld_prompt,
                                                         const int* __restrict__ plen, const int* __restrict__ tokens,
                                                         int max_tokens, const int* __restrict__ gen0,
                                                         const int* __restrict__ step_ptr, const int* __restrict__ ngram,
                                                         const int* __restrict__ min_tokens, const int* __restrict__ words,
                                                         BanWords bw, const int* __restrict__ eos_ids, int n_eos,
                                                         float* __restrict__ out, int ld_out, int vec) {
  const int row = blockIdx.y, tid = threadIdx.x;
  const float* __restrict__ x = logits + (size_t)row * ld_logits;
  float* __restrict__ y = out + (size_t)row * ld_out;

  // the ids this workgroup owns: groups [g0, g1) of four
  const int ngroups = (V + 3) >> 2;
  const int per = (ngroups + (int)gridDim.x - 1) / (int)gridDim.x;
  const int g0 = min((int)blockIdx.x * per, ngroups), g1 = min(g0 + per, ngroups);
  const int lo = g0 * 4, hi = min(g1 * 4, V);

  for (int g = g0 + tid; g < g1; g += BN_THREADS) {
    const int v0 = g * 4;
    if (vec && v0 + 4 <= V) {
      *(f32x4*)(y + v0) = *(const f32x4*)(x + v0);
    } else {
      for (int v = v0; v < min(v0 + 4, V); ++v) y[v] = x[v];
    }
  }
  // no copy store may land after a ban store to the same address: the stores of this wave have completed, then the barrier
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (lo >= hi) return;

  const int P = min(max(plen[row], 0), ld_prompt);
  const int end = min(max(step_ptr[row], 0), max_tokens);
  const int s0 = min(max(gen0[row], 0), end);
  const int G = end - s0, L = P + G;
  const int* __restrict__ pr = prompt + (size_t)row * ld_prompt;
  const int* __restrict__ gn = tokens + (size_t)row * max_tokens + s0;
#define BN_H(i) ((i) < P ? pr[(i)] : gn[(i) - P])
#define BN_BAN(id)                                                   \
  do {                                                               \
    const int id_ = (id);                                            \
    if (id_ >= lo && id_ < hi) y[id_] = -INFINITY;                   \
  } while (0)

  // n-gram: position i starts a copy of the last n - 1 ids -> what followed it is banned
  const int n = ngram[row];
  if (n >= 1 && L >= n) {
    const int tail = L - n + 1;                     // h[tail .. L) are the last n - 1 ids
    for (int i = tid; i + n - 1 < L; i += BN_THREADS) {
      bool match = true;
      for (int j = 0; j < n - 1 && match; ++j) match = BN_H(i + j) == BN_H(tail + j);
      if (match) BN_BAN(BN_H(i + n - 1));
    }
  }
  // bad words: one lane per word
  if (tid < bw.n) {
    const int m = bw.len[tid];
    const int* __restrict__ w = words + tid * BN_MAXWORDLEN;
    bool match = L >= m - 1;
    for (int j = 0; j < m - 1 && match; ++j) match = BN_H(L - m + 1 + j) == w[j];
    if (match) BN_BAN(w[m - 1]);
  }
  // min_tokens: no EOS yet
  if (tid < n_eos && G < min_tokens[row]) BN_BAN(eos_ids[tid]);
#undef BN_H
#undef BN_BAN
}

extern "C" int vis_ban_f32(const void* logits, int V, int ld_logits, const void* prompt_ids, int ld_prompt,
                           const void* prompt_len, const void* tokens, int max_tokens, const void* gen_start,
                           const void* step_ptr, const void* ngram, const void* min_tokens, const void* words,
                           const int* word_len, int n_words, const void* eos_ids, int n_eos, void* out, int ld_out, int batch,
                           hipStream_t stream) {
  if (!logits || !prompt_ids || !prompt_len || !tokens || !gen_start || !step_ptr || !ngram || !min_tokens || !words ||
      !eos_ids || !out)
    return VIS_ERR_ARG;
  if (V <= 0 || V > BN_MAXV || batch < 1 || batch > BN_MAXBATCH || max_tokens <= 0 || ld_prompt <= 0) return VIS_ERR_ARG;
  if (ld_logits < V || ld_out < V) return VIS_ERR_ARG;
  if (n_words < 0 || n_words > BN_MAXWORDS || n_eos < 0 || n_eos > BN_MAXEOS || (n_words > 0 && !word_len)) return VIS_ERR_ARG;
  BanWords bw = {};
  bw.n = n_words;
  for (int w = 0; w < n_words; ++w) {
    if (word_len[w] < 1 || word_len[w] > BN_MAXWORDLEN) return VIS_ERR_ARG;
    bw.len[w] = (unsigned char)word_len[w];
  }
  if (((uintptr_t)logits & 3) || ((uintptr_t)out & 3) || ((uintptr_t)prompt_ids & 3) || ((uintptr_t)prompt_len & 3) ||
      ((uintptr_t)tokens & 3) || ((uintptr_t)gen_start & 3) || ((uintptr_t)step_ptr & 3) || ((uintptr_t)ngram & 3) ||
      ((uintptr_t)min_tokens & 3) || ((uintptr_t)words & 3) || ((uintptr_t)eos_ids & 3))
    return VIS_ERR_ARG;
  if (logits == out) return VIS_ERR_ARG;                  // the input row stays intact (logprobs read the raw rows)
  const int vec = !((uintptr_t)logits & 15) && !((uintptr_t)out & 15) && (batch == 1 || (ld_logits % 4 == 0 && ld_out % 4 == 0));
  // 1024 ids per workgroup and iteration; past ~8 workgroups per CU over the batch a workgroup owns a longer run of ids (each
  // workgroup scans the row's history once, so fewer, longer workgroups at large batches)
  int blocks = (V + 1023) / 1024;
  const int cap = max(1, 2048 / batch);
  if (blocks > cap) blocks = cap;
  vis_clear_error();
  hipLaunchKernelGGL(ban_kernel, dim3(blocks, batch), dim3(BN_THREADS), 0, stream, (const float*)logits, V, ld_logits,
                     (const int*)prompt_ids, ld_prompt, (const int*)prompt_len, (const int*)tokens, max_tokens,
                     (const int*)gen_start, (const int*)step_ptr, (const int*)ngram, (const int*)min_tokens,
                     (const int*)words, bw, (const int*)eos_ids, n_eos, (float*)out, ld_out, vec);
  return vis_check_launch();
}
