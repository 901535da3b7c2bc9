// Schema-constrained decoding (vis_schema_mask): vis_json_mask's contract with a compiled DFA in place of the hard-wired
// grammar.  json_schema.py compiles a JSON Schema to the tables and is the reference of the tests (allowed / advance).
//
// The grammar is data: trans [n_states][n_classes] u16 (SM_DEAD = no transition), byte_class [256] u8, state_flags
// [n_states] u8, and a header {n_states, n_classes, start, 0} the kernel READS - table sizes are not kernel arguments, so a
// decode graph captured under one schema serves the next one after the host has overwritten the fixed-capacity buffers.
// A byte costs one lookup, s = trans[s * n_classes + byte_class[b]], and one test: s >= n_states is both "dead" and the
// bound of the next lookup.  A header outside the buffers' capacity, or a state outside the header, puts the row in the
// error state instead of indexing anything.
//
// State: int32 [batch][SM_STATE_INTS], json_mask.hip's layout - two slots of SM_SLOT_INTS words chosen by the parity of the
// step (read slot step & 1, write slot (step + 1) & 1: a repeated launch at the same step repeats the same result) and the
// count / ticket words.  Slot words: DFA state, error bit, position, anchored; an all-zero slot is a fresh sequence in the
// header's start state.
//
// One launch per pick, grid (blocks, batch), 512 threads.  byte_class is staged in LDS, and trans too when it fits
// SM_LDS_TRANS_BYTES (two workgroups per CU then still fit the 160 KiB); a larger table is read through L2.  A wave per
// 64-token word, one lane per token, __ballot forms the word.  In a state flagged PLAIN (a string body) tokens flagged
// PLAIN are accepted without a walk.  The count / ticket rule for "nothing allowed -> EOS ids + error bit" is json_mask's.
#include "common.hip.h"

#define SM_MAX_STATES 4096       // json_schema.SCHEMA_MAX_STATES
#define SM_MAX_CLASSES 256       // json_schema.SCHEMA_MAX_CLASSES
#define SM_DEAD 65535            // json_schema.DEAD
#define SM_SLOT_INTS 12
#define SM_STATE_INTS 32
#define SM_COUNT 24
#define SM_TICKET 25
#define SM_HEADER_INTS 4
#define SM_FLAG_EOS 1            // token flags (json_grammar.FLAG_*)
#define SM_FLAG_PLAIN 2
#define SM_STATE_ACCEPT 1        // state flags (json_schema.STATE_*)
#define SM_STATE_PLAIN 2
#define SM_MAXBATCH 64
#define SM_MAXV 262144
#define SM_THREADS 512
#define SM_WAVES (SM_THREADS / 64)
#define SM_LDS_TRANS_BYTES (72 * 1024)

// slot words (json_schema.STATE .. ANCHOR)
enum { SW_STATE, SW_ERR, SW_POS, SW_ANCHOR };

// walk data[a .. e) (e > a) from state s; the byte table is read as aligned dwords (it carries 4 bytes of padding).
// Returns the end state, or a value >= n_states at the first rejected byte.
template <typename T>
__device__ __forceinline__ unsigned sm_walk(unsigned s, const unsigned* __restrict__ data32, int a, int e, T trans,
                                            const unsigned char* cls, unsigned n_states, unsigned n_classes) {
  unsigned word = data32[a >> 2];
  for (int j = a; j < e; ++j) {
    if ((j & 3) == 0 && j != a) word = data32[j >> 2];
    s = trans[s * n_classes + cls[(word >> (8 * (j & 3))) & 0xFFu]];
    if (s >= n_states) return SM_DEAD;
  }
  return s;
}

template <typename T>
__device__ __forceinline__ void sm_row(int* __restrict__ st, const int* __restrict__ toks, int max_tokens, int step,
                                       const int* __restrict__ off, const unsigned* __restrict__ data32,
                                       const unsigned char* __restrict__ flags, const int* __restrict__ eos_ids, int n_eos,
                                       int V, unsigned long long* __restrict__ out, T trans, const unsigned char* cls,
                                       const unsigned char* __restrict__ state_flags, unsigned n_states, unsigned n_classes,
                                       unsigned start, bool bad_header) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* __restrict__ rd = st + (step & 1) * SM_SLOT_INTS;
  unsigned s = rd[SW_ANCHOR] ? (unsigned)rd[SW_STATE] : start;
  int err = rd[SW_ERR] | (int)bad_header;
  if (s >= n_states) { s = 0; err = 1; }
  const int pos = rd[SW_ANCHOR] ? rd[SW_POS] : step;
  const int end = min(step, max_tokens);
  // json_schema.advance: fold the tokens picked since the slot was written; a rejected one sets the error bit only
  for (int p = max(pos, 0); p < end && !err; ++p) {
    const int tok = toks[p];
    if (tok < 0 || tok >= V) { err = 1; break; }
    if (flags[tok] & SM_FLAG_EOS) {
      if (!(state_flags[s] & SM_STATE_ACCEPT)) err = 1;
      continue;
    }
    const int a = off[tok], e = off[tok + 1];
    const unsigned n = a < e ? sm_walk(s, data32, a, e, trans, cls, n_states, n_classes) : SM_DEAD;
    if (n >= n_states) err = 1;
    else s = n;
  }
  int* __restrict__ wr = st + ((step + 1) & 1) * SM_SLOT_INTS;
  if (blockIdx.x == 0 && tid == 0) {
    wr[SW_STATE] = (int)s; wr[SW_ERR] = err; wr[SW_POS] = step; wr[SW_ANCHOR] = 1;
  }

  const int nwords = (V + 63) >> 6;
  const unsigned sf = err ? 0u : state_flags[s];
  const bool plain_ok = sf & SM_STATE_PLAIN, done = sf & SM_STATE_ACCEPT;
  int cnt = 0;
  for (int w = blockIdx.x * SM_WAVES + wave; w < nwords; w += gridDim.x * SM_WAVES) {
    const int t = w * 64 + lane;
    bool ok = false;
    if (t < V && !err) {
      const unsigned f = flags[t];
      if (f & SM_FLAG_EOS) ok = done;
      else if (plain_ok && (f & SM_FLAG_PLAIN)) ok = true;
      else {
        const int a = off[t], e = off[t + 1];
        if (a < e) ok = sm_walk(s, data32, a, e, trans, cls, n_states, n_classes) < n_states;
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) {
      out[w] = m;
      cnt += __popcll(m);
    }
  }

  __shared__ int wg_cnt, wg_last;
  if (tid == 0) wg_cnt = 0;
  __syncthreads();
  if (lane == 0 && cnt) atomicAdd(&wg_cnt, cnt);
  __syncthreads();
  if (tid == 0) {
    if (wg_cnt) atomicAdd(&st[SM_COUNT], wg_cnt);
    __threadfence();                                     // this workgroup's words (and workgroup 0's state) before its ticket
    wg_last = atomicAdd(&st[SM_TICKET], 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!wg_last || tid != 0) return;
  __threadfence();
  if (atomicAdd(&st[SM_COUNT], 0) == 0) {                // no token allowed: EOS instead, and the request is marked failed
    for (int i = 0; i < n_eos; ++i) {
      const int id = eos_ids[i];
      if (id >= 0 && id < V) atomicOr(&out[id >> 6], 1ull << (id & 63));
    }
    wr[SW_ERR] = 1;
  }
  st[SM_COUNT] = 0;                                      // every workgroup has counted: reset for the next launch
  st[SM_TICKET] = 0;
}

__global__ __launch_bounds__(SM_THREADS) void schema_mask_kernel(
    int* __restrict__ state, const int* __restrict__ tokens, int max_tokens, const int* __restrict__ step_ptr,
    const int* __restrict__ off, const unsigned* __restrict__ data32, const unsigned char* __restrict__ flags,
    const int* __restrict__ eos_ids, int n_eos, int V, unsigned long long* __restrict__ allow, int ld_allow,
    const int* __restrict__ header, const unsigned short* __restrict__ trans, const unsigned char* __restrict__ byte_class,
    const unsigned char* __restrict__ state_flags, int cap_states, int cap_classes) {
  extern __shared__ __attribute__((aligned(16))) char sm_lds[];
  __shared__ unsigned char cls[256];
  const int tid = threadIdx.x, row = blockIdx.y;
  unsigned n_states = (unsigned)header[0], n_classes = (unsigned)header[1], start = (unsigned)header[2];
  const bool bad_header = n_states < 1 || n_states > (unsigned)cap_states || n_classes < 1 ||
                          n_classes > (unsigned)cap_classes || start >= n_states;
  if (bad_header) { n_states = 1; n_classes = 1; start = 0; }     // nothing is walked: the row is in the error state
  if (tid < 256) {
    const unsigned c = byte_class[tid];
    cls[tid] = (unsigned char)(c < n_classes ? c : n_classes - 1);   // a class outside the header cannot index past a row
  }
  const unsigned bytes = n_states * n_classes * 2;
  const bool in_lds = bytes <= SM_LDS_TRANS_BYTES;
  if (in_lds) {
    const u32x4* __restrict__ src = (const u32x4*)trans;            // 16-byte aligned, capacity a multiple of 16 bytes
    u32x4* dst = (u32x4*)sm_lds;
    for (unsigned i = tid; i < (bytes + 15) / 16; i += SM_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  int* __restrict__ st = state + (size_t)row * SM_STATE_INTS;
  const int* __restrict__ toks = tokens + (size_t)row * max_tokens;
  unsigned long long* __restrict__ out = allow + (size_t)row * ld_allow;
  if (in_lds)
    sm_row(st, toks, max_tokens, step_ptr[row], off, data32, flags, eos_ids, n_eos, V, out, (const unsigned short*)sm_lds,
           cls, state_flags, n_states, n_classes, start, bad_header);
  else
    sm_row(st, toks, max_tokens, step_ptr[row], off, data32, flags, eos_ids, n_eos, V, out, trans, cls, state_flags,
           n_states, n_classes, start, bad_header);
}

extern "C" int vis_schema_mask(void* state, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                               const void* tok_bytes, const void* tok_flags, const void* eos_ids, int n_eos, int V,
                               void* allow, int ld_allow, const void* header, const void* trans, const void* byte_class,
                               const void* state_flags, int cap_states, int cap_classes, int batch, hipStream_t stream) {
  if (!state || !tokens || !step_ptr || !tok_off || !tok_bytes || !tok_flags || !eos_ids || !allow) return VIS_ERR_ARG;
  if (!header || !trans || !byte_class || !state_flags) return VIS_ERR_ARG;
  if (V <= 0 || V > SM_MAXV || max_tokens <= 0 || n_eos < 1 || n_eos > 64 || batch < 1 || batch > SM_MAXBATCH)
    return VIS_ERR_ARG;
  if (cap_states < 1 || cap_states > SM_MAX_STATES || cap_classes < 1 || cap_classes > SM_MAX_CLASSES) return VIS_ERR_ARG;
  if (((size_t)cap_states * cap_classes * 2) % 16) return VIS_ERR_ARG;
  if (ld_allow < (V + 63) / 64 || ((uintptr_t)allow & 7) || ((uintptr_t)tok_bytes & 3) || ((uintptr_t)state & 3) ||
      ((uintptr_t)header & 3) || ((uintptr_t)trans & 15))
    return VIS_ERR_ARG;
  const int nwords = (V + 63) / 64;
  // a word per wave until the grid holds two workgroups per CU over the batch, then several words per wave: every
  // workgroup stages the table once, so few large workgroups beat many small ones
  int blocks = (nwords + SM_WAVES - 1) / SM_WAVES;
  const int cap = max(1, 512 / batch);
  if (blocks > cap) blocks = cap;
  static const bool attr_ok = hipFuncSetAttribute((const void*)schema_mask_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  SM_LDS_TRANS_BYTES) == hipSuccess;
  if (!attr_ok) return VIS_ERR_LAUNCH;
  vis_clear_error();
  hipLaunchKernelGGL(schema_mask_kernel, dim3(blocks, batch), dim3(SM_THREADS), SM_LDS_TRANS_BYTES, stream, (int*)state,
                     (const int*)tokens, max_tokens, (const int*)step_ptr, (const int*)tok_off, (const unsigned*)tok_bytes,
                     (const unsigned char*)tok_flags, (const int*)eos_ids, n_eos, V, (unsigned long long*)allow, ld_allow,
                     (const int*)header, (const unsigned short*)trans, (const unsigned char*)byte_class,
                     (const unsigned char*)state_flags, cap_states, cap_classes);
  return vis_check_launch();
}
