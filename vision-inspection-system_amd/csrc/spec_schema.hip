// The speculative step under a JSON Schema (spec.py "grammar"; DecodeStage._decode_step_spec): the two launches that know the
// compiled DFA of json_schema.py.  (The third piece, vis_spec_accept_masked, is spec.hip's accept with masked picks.)
//
//  * vis_schema_mask_rows: the allow rows of the R = 1..4 rows of ONE sequence's step.  Row 0 is vis_schema_mask's row at
//    *step_ptr: the same fold of the tokens picked since the record's position, the same "nothing allowed -> EOS ids".  Row
//    r >= 1 is the row of the state behind draft 0 .. draft r-1, walked in registers from row 0's state - the state the plain
//    loop would be in had it picked those drafts, which is the only case in which row r's pick is ever used.  From the first
//    r with r > *n_draft, or whose draft is out of range, an EOS id or rejected by the walk, the rows are all-zero: the draft
//    in front of them cannot be the masked pick, so the accept step never reaches them.
//    Record: int32 [SR_INTS].  Words 0..3 are one slot in json_schema's slot layout (DFA state, error bit, position,
//    anchored; anchored 0 = the header's start state - the position counts either way, so an all-zero record is a sequence
//    whose reply starts at token 0).  *step_ptr advances by 1..R between launches, so there is no parity pair: every
//    workgroup reads the slot, and the workgroup that arrives LAST at the launch's ticket - after every workgroup has read -
//    writes it.  A launch repeated at the same step therefore finds position == step, folds nothing and repeats its rows.
//    Only picked tokens ever enter the fold; drafts are never stored.  Words 8.. / 12..: the per-row count and ticket of
//    the "nothing allowed" rule, word 16 the launch's ticket; all are zero between launches.
//    Grid (blocks, rows), 512 threads; every workgroup derives its row's state itself (at most 3 short walks).  The
//    staging of byte_class / trans in LDS, the header and capacity clamps and the word loop are vis_schema_mask's.
//  * vis_spec_draft_schema: the drafter that reads the schema (schema_draft.propose is its definition).  It folds the
//    tokens behind the record's position into the DFA state with the same fold - reading the record only - and follows
//    jump_tok / jump_next (schema_draft.build: per state the longest token that spells a prefix of the bytes the schema
//    forces there, and the state behind it) up to k times.  With no draft it leaves draft / *n_draft alone: what the
//    drafter in front of it wrote stands.  One workgroup.
//
// Every value read from device memory (the header, the record, *step_ptr, the draft count, drafts, jump entries) is checked
// against its range before it forms an address.
#include "schema_common.hip.h"

#define SR_INTS 32
#define SR_COUNT 8
#define SR_TICKET 12
#define SR_DONE 16
#define SR_MAXROWS 4             // SP_MAXROWS of decode_common.hip.h
#define SR_MAXPATH 3

struct SrHeader {
  unsigned n_states, n_classes, start;
  bool bad;
};

__device__ __forceinline__ SrHeader sr_header(const int* __restrict__ header, int cap_states, int cap_classes) {
  SrHeader h;
  h.n_states = (unsigned)header[0]; h.n_classes = (unsigned)header[1]; h.start = (unsigned)header[2];
  h.bad = h.n_states < 1 || h.n_states > (unsigned)cap_states || h.n_classes < 1 || h.n_classes > (unsigned)cap_classes ||
          h.start >= h.n_states;
  if (h.bad) { h.n_states = 1; h.n_classes = 1; h.start = 0; }     // nothing is walked: the sequence is in the error state
  return h;
}

// json_schema.advance over tokens[pos .. end) from the record's slot: (state, error bit) behind them
template <typename T>
__device__ __forceinline__ void sr_fold(const int* __restrict__ rec, const int* __restrict__ toks, int end,
                                        const int* __restrict__ off, const unsigned* __restrict__ data32,
                                        const unsigned char* __restrict__ flags, int V, T trans, const unsigned char* cls,
                                        const unsigned char* __restrict__ state_flags, const SrHeader& h, unsigned& s_out,
                                        int& err_out) {
  unsigned s = rec[SW_ANCHOR] ? (unsigned)rec[SW_STATE] : h.start;
  int err = (rec[SW_ERR] != 0) | (int)h.bad;
  if (s >= h.n_states) { s = 0; err = 1; }
  for (int p = max(rec[SW_POS], 0); p < end && !err; ++p) {
    const int tok = toks[p];
    if (tok < 0 || tok >= V) { err = 1; break; }
    if (flags[tok] & SM_FLAG_EOS) {
      if (!(state_flags[s] & SM_STATE_ACCEPT)) err = 1;
      continue;
    }
    const int a = off[tok], e = off[tok + 1];
    const unsigned n = a < e ? sm_walk(s, data32, a, e, trans, cls, h.n_states, h.n_classes) : SM_DEAD;
    if (n >= h.n_states) err = 1;
    else s = n;
  }
  s_out = s;
  err_out = err;
}

template <typename T>
__device__ __forceinline__ void smr_row(int* __restrict__ rec, const int* __restrict__ toks, int max_tokens, int step,
                                        const int* __restrict__ draft, int d, const int* __restrict__ off,
                                        const unsigned* __restrict__ data32, const unsigned char* __restrict__ flags,
                                        const int* __restrict__ eos_ids, int n_eos, int V,
                                        unsigned long long* __restrict__ out, T trans, const unsigned char* cls,
                                        const unsigned char* __restrict__ state_flags, const SrHeader& h) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y;
  unsigned s0;
  int err0;
  sr_fold(rec, toks, min(step, max_tokens), off, data32, flags, V, trans, cls, state_flags, h, s0, err0);
  // the row's own state: row 0's walked through the drafts in front of the row (uniform over the workgroup)
  unsigned s = s0;
  bool live = true;
  for (int j = 0; j < row && live; ++j) {
    const int t = j < d ? draft[j] : -1;
    if (err0 || t < 0 || t >= V || (flags[t] & SM_FLAG_EOS)) { live = false; break; }
    const int a = off[t], e = off[t + 1];
    const unsigned n = a < e ? sm_walk(s, data32, a, e, trans, cls, h.n_states, h.n_classes) : SM_DEAD;
    if (n >= h.n_states) live = false;
    else s = n;
  }
  const int err = row == 0 ? err0 : 0;

  const int nwords = (V + 63) >> 6;
  const unsigned sf = (err || !live) ? 0u : state_flags[s];
  const bool plain_ok = sf & SM_STATE_PLAIN, done = sf & SM_STATE_ACCEPT;
  int cnt = 0;
  for (int w = blockIdx.x * SM_WAVES + wave; w < nwords; w += gridDim.x * SM_WAVES) {
    const int t = w * 64 + lane;
    bool ok = false;
    if (t < V && !err && live) {
      const unsigned f = flags[t];
      if (f & SM_FLAG_EOS) ok = done;
      else if (plain_ok && (f & SM_FLAG_PLAIN)) ok = true;
      else {
        const int a = off[t], e = off[t + 1];
        if (a < e) ok = sm_walk(s, data32, a, e, trans, cls, h.n_states, h.n_classes) < h.n_states;
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) {
      out[w] = m;
      cnt += __popcll(m);
    }
  }

  __shared__ int wg_cnt;
  if (tid == 0) wg_cnt = 0;
  __syncthreads();
  if (lane == 0 && cnt) atomicAdd(&wg_cnt, cnt);
  __syncthreads();
  if (tid != 0) return;
  if (live) {                                            // a row behind a rejected draft stays all-zero: no EOS rule
    if (wg_cnt) atomicAdd(&rec[SR_COUNT + row], wg_cnt);
    __threadfence();                                     // this workgroup's words before its ticket
    if (atomicAdd(&rec[SR_TICKET + row], 1) == (int)gridDim.x - 1) {
      __threadfence();
      if (atomicAdd(&rec[SR_COUNT + row], 0) == 0) {     // no token allowed: the EOS ids instead
        for (int i = 0; i < n_eos; ++i) {
          const int id = eos_ids[i];
          if (id >= 0 && id < V) atomicOr(&out[id >> 6], 1ull << (id & 63));
        }
      }
      rec[SR_COUNT + row] = 0;                           // every workgroup of the row has counted
      rec[SR_TICKET + row] = 0;
    }
  }
  __threadfence();
  if (atomicAdd(&rec[SR_DONE], 1) == (int)(gridDim.x * gridDim.y) - 1) {
    // the last workgroup of the launch: every workgroup has read the slot, so it may move to this step
    rec[SW_STATE] = (int)s0; rec[SW_ERR] = err0; rec[SW_POS] = step; rec[SW_ANCHOR] = 1;
    rec[SR_DONE] = 0;
  }
}

__global__ __launch_bounds__(SM_THREADS) void schema_mask_rows_kernel(
    int* __restrict__ rec, const int* __restrict__ tokens, int max_tokens, const int* __restrict__ step_ptr,
    const int* __restrict__ draft, const int* __restrict__ n_draft, const int* __restrict__ off,
    const unsigned* __restrict__ data32, const unsigned char* __restrict__ flags, const int* __restrict__ eos_ids, int n_eos,
    int V, unsigned long long* __restrict__ allow, int ld_allow, const int* __restrict__ header,
    const unsigned short* __restrict__ trans, const unsigned char* __restrict__ byte_class,
    const unsigned char* __restrict__ state_flags, int cap_states, int cap_classes) {
  extern __shared__ __attribute__((aligned(16))) char sm_lds[];
  __shared__ unsigned char cls[256];
  const int tid = threadIdx.x;
  const SrHeader h = sr_header(header, cap_states, cap_classes);
  if (tid < 256) {
    const unsigned c = byte_class[tid];
    cls[tid] = (unsigned char)(c < h.n_classes ? c : h.n_classes - 1);   // a class outside the header cannot index past a row
  }
  const unsigned bytes = h.n_states * h.n_classes * 2;
  const bool in_lds = bytes <= SM_LDS_TRANS_BYTES;
  if (in_lds) {
    const u32x4* __restrict__ src = (const u32x4*)trans;            // 16-byte aligned, capacity a multiple of 16 bytes
    u32x4* dst = (u32x4*)sm_lds;
    for (unsigned i = tid; i < (bytes + 15) / 16; i += SM_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const int d = min(max(*n_draft, 0), (int)gridDim.y - 1);
  unsigned long long* __restrict__ out = allow + (size_t)blockIdx.y * ld_allow;
  if (in_lds)
    smr_row(rec, tokens, max_tokens, *step_ptr, draft, d, off, data32, flags, eos_ids, n_eos, V, out,
            (const unsigned short*)sm_lds, cls, state_flags, h);
  else
    smr_row(rec, tokens, max_tokens, *step_ptr, draft, d, off, data32, flags, eos_ids, n_eos, V, out, trans, cls, state_flags,
            h);
}

extern "C" int vis_schema_mask_rows(void* record, const void* tokens, int max_tokens, const void* step_ptr, const void* draft,
                                    const void* n_draft, int rows, const void* tok_off, const void* tok_bytes,
                                    const void* tok_flags, const void* eos_ids, int n_eos, int V, void* allow, int ld_allow,
                                    const void* header, const void* trans, const void* byte_class, const void* state_flags,
                                    int cap_states, int cap_classes, hipStream_t stream) {
  if (!record || !tokens || !step_ptr || !draft || !n_draft || !tok_off || !tok_bytes || !tok_flags || !eos_ids || !allow)
    return VIS_ERR_ARG;
  if (!header || !trans || !byte_class || !state_flags) return VIS_ERR_ARG;
  if (V <= 0 || V > SM_MAXV || max_tokens <= 0 || n_eos < 1 || n_eos > 64 || rows < 1 || rows > SR_MAXROWS) return VIS_ERR_ARG;
  if (cap_states < 1 || cap_states > SM_MAX_STATES || cap_classes < 1 || cap_classes > SM_MAX_CLASSES) return VIS_ERR_ARG;
  if (((size_t)cap_states * cap_classes * 2) % 16) return VIS_ERR_ARG;
  if (ld_allow < (V + 63) / 64 || ((uintptr_t)allow & 7) || ((uintptr_t)tok_bytes & 3) || ((uintptr_t)record & 3) ||
      ((uintptr_t)header & 3) || ((uintptr_t)trans & 15) || (((uintptr_t)draft | (uintptr_t)n_draft | (uintptr_t)step_ptr) & 3))
    return VIS_ERR_ARG;
  const int nwords = (V + 63) / 64;
  int blocks = (nwords + SM_WAVES - 1) / SM_WAVES;       // vis_schema_mask's grid rule with the rows in the batch's place
  const int cap = max(1, 512 / rows);
  if (blocks > cap) blocks = cap;
  static const bool attr_ok = hipFuncSetAttribute((const void*)schema_mask_rows_kernel,
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_TRANS_BYTES) == hipSuccess;
  if (!attr_ok) return VIS_ERR_LAUNCH;
  vis_clear_error();
  hipLaunchKernelGGL(schema_mask_rows_kernel, dim3(blocks, rows), dim3(SM_THREADS), SM_LDS_TRANS_BYTES, stream, (int*)record,
                     (const int*)tokens, max_tokens, (const int*)step_ptr, (const int*)draft, (const int*)n_draft,
                     (const int*)tok_off, (const unsigned*)tok_bytes, (const unsigned char*)tok_flags, (const int*)eos_ids, n_eos,
                     V, (unsigned long long*)allow, ld_allow, (const int*)header, (const unsigned short*)trans,
                     (const unsigned char*)byte_class, (const unsigned char*)state_flags, cap_states, cap_classes);
  return vis_check_launch();
}

// ------------------------------------------------------------------------------------------------ vis_spec_draft_schema
__global__ __launch_bounds__(256) void spec_draft_schema_kernel(
    const int* __restrict__ rec, const int* __restrict__ tokens, int max_tokens, const int* __restrict__ step_ptr,
    const int* __restrict__ off, const unsigned* __restrict__ data32, const unsigned char* __restrict__ flags, int V,
    const int* __restrict__ header, const unsigned short* __restrict__ trans, const unsigned char* __restrict__ byte_class,
    const unsigned char* __restrict__ state_flags, int cap_states, int cap_classes, const int* __restrict__ jump_tok,
    const int* __restrict__ jump_next, int k, int* __restrict__ draft, int* __restrict__ n_draft) {
  __shared__ unsigned char cls[256];
  const SrHeader h = sr_header(header, cap_states, cap_classes);
  {
    const unsigned c = byte_class[threadIdx.x];
    cls[threadIdx.x] = (unsigned char)(c < h.n_classes ? c : h.n_classes - 1);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;                          // a few dozen dependent table reads: one lane
  unsigned s;
  int err;
  sr_fold(rec, tokens, min(max(*step_ptr, 0), max_tokens), off, data32, flags, V, trans, cls, state_flags, h, s, err);
  if (err) return;
  int buf[SR_MAXPATH], n = 0;
  for (; n < k; ++n) {                                   // s < n_states <= cap_states, the tables' length
    const int t = jump_tok[s], nx = jump_next[s];
    if (t < 0 || t >= V || nx < 0 || (unsigned)nx >= h.n_states) break;
    buf[n] = t;
    s = (unsigned)nx;
  }
  if (n == 0) return;                                    // what the drafter in front wrote stands
  for (int i = 0; i < n; ++i) draft[i] = buf[i];
  *n_draft = n;
}

extern "C" int vis_spec_draft_schema(const void* record, const void* tokens, int max_tokens, const void* step_ptr,
                                     const void* tok_off, const void* tok_bytes, const void* tok_flags, int V,
                                     const void* header, const void* trans, const void* byte_class, const void* state_flags,
                                     int cap_states, int cap_classes, const void* jump_tok, const void* jump_next, int k,
                                     void* draft, void* n_draft, hipStream_t stream) {
  if (!record || !tokens || !step_ptr || !tok_off || !tok_bytes || !tok_flags || !header || !trans || !byte_class || !state_flags ||
      !jump_tok || !jump_next || !draft || !n_draft)
    return VIS_ERR_ARG;
  if (V <= 0 || V > SM_MAXV || max_tokens <= 0 || k < 1 || k > SR_MAXPATH) return VIS_ERR_ARG;
  if (cap_states < 1 || cap_states > SM_MAX_STATES || cap_classes < 1 || cap_classes > SM_MAX_CLASSES) return VIS_ERR_ARG;
  if (((uintptr_t)record | (uintptr_t)tokens | (uintptr_t)step_ptr | (uintptr_t)tok_off | (uintptr_t)tok_bytes | (uintptr_t)header |
       (uintptr_t)jump_tok | (uintptr_t)jump_next | (uintptr_t)draft | (uintptr_t)n_draft) & 3)
    return VIS_ERR_ARG;
  if ((uintptr_t)trans & 1) return VIS_ERR_ARG;
  vis_clear_error();
  hipLaunchKernelGGL(spec_draft_schema_kernel, dim3(1), dim3(256), 0, stream, (const int*)record, (const int*)tokens, max_tokens,
                     (const int*)step_ptr, (const int*)tok_off, (const unsigned*)tok_bytes, (const unsigned char*)tok_flags, V,
                     (const int*)header, (const unsigned short*)trans, (const unsigned char*)byte_class,
                     (const unsigned char*)state_flags, cap_states, cap_classes, (const int*)jump_tok, (const int*)jump_next, k,
                     (int*)draft, (int*)n_draft);
  return vis_check_launch();
}
