// JSON mode (vis_json_mask): per-sequence grammar state and the allowed-token bitmask of the next pick.
//
// The grammar is json_grammar.py's, transliterated: jg_step below is json_grammar.step byte for byte (the Python module is
// the reference of the tests).  A token is allowed when the grammar accepts its whole byte string from the row's state;
// EOS ids only in the DONE state (after the top-level '}'); tokens without bytes never.
//
// One launch per pick, grid (blocks, batch), 256 threads.  State: int32 [batch][JG_STATE_INTS] - two slots of JG_SLOT_INTS
// words and the launch's counters.  The slot read is the one of the step's parity, (step & 1); every workgroup folds the
// tokens picked since that slot was written (positions pos .. step - 1 of the token buffer: one in steady state, none at
// the prompt pass) into registers, and workgroup 0 writes the folded state to the other slot, ((step + 1) & 1) - the slot
// the next launch reads once the pick has advanced the step.  Reads and the write never touch the same slot, so no
// workgroup can see a half-written state; a launch repeated at the same step (graph warm-up) reads and writes the same
// slots again with the same result.
//
// Mask: a wave per 64-token word, one lane per token; a lane walks its token's bytes from the state (aligned dword loads
// of the CSR byte table) and stops at the first rejected byte - most tokens stop at their first byte outside strings.
// Inside a string (no UTF-8 sequence open) tokens flagged PLAIN (printable ASCII without '"' and '\') are accepted without
// a walk.  __ballot forms the word.  Every workgroup adds its count of allowed tokens to the row's counter; the last
// workgroup to finish (ticket) sees the total, and if it is zero (a vocabulary that lacks a byte the grammar needs) it
// allows the EOS ids and sets the error bit of the new state, then zeroes the counters for the next launch.
#include "common.hip.h"

#define JG_MAX_DEPTH 32          // json_grammar.MAX_DEPTH
#define JG_MAX_WS 16             // json_grammar.MAX_WS
#define JG_SLOT_INTS 12
#define JG_STATE_INTS 32
#define JG_COUNT 24
#define JG_TICKET 25
#define JG_FLAG_EOS 1
#define JG_FLAG_PLAIN 2
#define JM_MAXBATCH 64
#define JM_MAXV 262144

enum {
  JG_START, JG_OBJ_FIRST, JG_OBJ_KEY, JG_COLON, JG_VALUE, JG_ARR_FIRST, JG_AFTER, JG_STR, JG_ESC, JG_HEX, JG_LIT_T,
  JG_LIT_F, JG_LIT_N, JG_N_MINUS, JG_N_ZERO, JG_N_INT, JG_N_DOT, JG_N_FRAC, JG_N_EXP, JG_N_EXP_SIGN, JG_N_EXP_DIG, JG_DONE
};
// slot words (json_grammar.LEX .. ANCHOR)
enum { JW_LEX, JW_DEPTH, JW_STACK, JW_WS, JW_UTF, JW_AUX, JW_KEY, JW_ERR, JW_POS, JW_ANCHOR };

struct JState {
  int lex, depth;
  unsigned stack;
  int ws, utf, aux, key, err;
};

__device__ __forceinline__ bool jg_push(JState& s, bool arr) {
  if (s.depth >= JG_MAX_DEPTH) return false;
  if (arr) s.stack |= 1u << s.depth;
  else s.stack &= ~(1u << s.depth);
  s.depth += 1;
  s.lex = arr ? JG_ARR_FIRST : JG_OBJ_FIRST;
  return true;
}

__device__ __forceinline__ void jg_pop(JState& s) {
  s.depth -= 1;
  s.lex = s.depth == 0 ? JG_DONE : JG_AFTER;
}

__device__ __forceinline__ bool jg_value_start(JState& s, unsigned b) {
  if (b == '{') return jg_push(s, false);
  if (b == '[') return jg_push(s, true);
  if (b == '"') { s.lex = JG_STR; s.key = 0; s.utf = 0; return true; }
  if (b == '-') s.lex = JG_N_MINUS;
  else if (b == '0') s.lex = JG_N_ZERO;
  else if (b >= '1' && b <= '9') s.lex = JG_N_INT;
  else if (b == 't') { s.lex = JG_LIT_T; s.aux = 1; }
  else if (b == 'f') { s.lex = JG_LIT_F; s.aux = 1; }
  else if (b == 'n') { s.lex = JG_LIT_N; s.aux = 1; }
  else return false;
  return true;
}

// expected byte i of a literal ("true", "false", "null"); 0 past its end
__device__ __forceinline__ unsigned jg_lit_byte(int lex, int i) {
  const unsigned long long w = lex == JG_LIT_T ? 0x65757274ull : lex == JG_LIT_F ? 0x65736c6166ull : 0x6c6c756eull;
  return (unsigned)(w >> (8 * i)) & 0xFFu;
}
__device__ __forceinline__ int jg_lit_len(int lex) { return lex == JG_LIT_F ? 5 : 4; }

// json_grammar.step
__device__ bool jg_step(JState& s, unsigned b) {
  if (s.err) return false;
  int lex = s.lex;
  if (lex == JG_STR) {
    const int pend = s.utf & 0xFF;
    if (pend) {
      if (b < (unsigned)((s.utf >> 8) & 0xFF) || b > (unsigned)((s.utf >> 16) & 0xFF)) return false;
      s.utf = pend > 1 ? ((pend - 1) | (0x80 << 8) | (0xBF << 16)) : 0;
      return true;
    }
    if (b == '"') { s.lex = s.key ? JG_COLON : JG_AFTER; s.key = 0; return true; }
    if (b == '\\') { s.lex = JG_ESC; return true; }
    if (b < 0x20) return false;
    if (b < 0x80) return true;
    if (b >= 0xC2 && b <= 0xDF) s.utf = 1 | (0x80 << 8) | (0xBF << 16);
    else if (b == 0xE0) s.utf = 2 | (0xA0 << 8) | (0xBF << 16);
    else if ((b >= 0xE1 && b <= 0xEC) || b == 0xEE || b == 0xEF) s.utf = 2 | (0x80 << 8) | (0xBF << 16);
    else if (b == 0xED) s.utf = 2 | (0x80 << 8) | (0x9F << 16);
    else if (b == 0xF0) s.utf = 3 | (0x90 << 8) | (0xBF << 16);
    else if (b >= 0xF1 && b <= 0xF3) s.utf = 3 | (0x80 << 8) | (0xBF << 16);
    else if (b == 0xF4) s.utf = 3 | (0x80 << 8) | (0x8F << 16);
    else return false;
    return true;
  }
  if (lex == JG_ESC) {
    if (b == '"' || b == '\\' || b == '/' || b == 'b' || b == 'f' || b == 'n' || b == 'r' || b == 't') {
      s.lex = JG_STR;
      return true;
    }
    if (b == 'u') { s.lex = JG_HEX; s.aux = 0; return true; }
    return false;
  }
  if (lex == JG_HEX) {
    if (!((b >= '0' && b <= '9') || (b >= 'A' && b <= 'F') || (b >= 'a' && b <= 'f'))) return false;
    s.aux += 1;
    if (s.aux == 4) { s.lex = JG_STR; s.aux = 0; }
    return true;
  }
  if (lex == JG_LIT_T || lex == JG_LIT_F || lex == JG_LIT_N) {
    if (b != jg_lit_byte(lex, s.aux)) return false;
    s.aux += 1;
    if (s.aux == jg_lit_len(lex)) { s.lex = JG_AFTER; s.aux = 0; }
    return true;
  }
  const bool digit = b >= '0' && b <= '9';
  if (lex == JG_N_MINUS) {
    if (b == '0') s.lex = JG_N_ZERO;
    else if (digit) s.lex = JG_N_INT;
    else return false;
    return true;
  }
  if (lex == JG_N_DOT) {
    if (!digit) return false;
    s.lex = JG_N_FRAC;
    return true;
  }
  if (lex == JG_N_EXP) {
    if (b == '+' || b == '-') s.lex = JG_N_EXP_SIGN;
    else if (digit) s.lex = JG_N_EXP_DIG;
    else return false;
    return true;
  }
  if (lex == JG_N_EXP_SIGN) {
    if (!digit) return false;
    s.lex = JG_N_EXP_DIG;
    return true;
  }
  if (lex == JG_N_ZERO || lex == JG_N_INT || lex == JG_N_FRAC || lex == JG_N_EXP_DIG) {
    if (digit && lex != JG_N_ZERO) return true;
    if (b == '.' && (lex == JG_N_ZERO || lex == JG_N_INT)) { s.lex = JG_N_DOT; return true; }
    if ((b == 'e' || b == 'E') && lex != JG_N_EXP_DIG) { s.lex = JG_N_EXP; return true; }
    if (digit) return false;                 // a digit after a leading zero
    s.lex = lex = JG_AFTER;                   // the number ends here: the byte is read as what follows a value
  }
  if (lex == JG_DONE) return false;
  // structural states
  if (b == ' ' || b == '\t' || b == '\n' || b == '\r') {
    s.ws += 1;
    return s.ws <= JG_MAX_WS;
  }
  s.ws = 0;
  if (lex == JG_START) return b == '{' && jg_push(s, false);
  if (lex == JG_OBJ_FIRST || lex == JG_OBJ_KEY) {
    if (b == '"') { s.lex = JG_STR; s.key = 1; s.utf = 0; return true; }
    if (b == '}' && lex == JG_OBJ_FIRST) { jg_pop(s); return true; }
    return false;
  }
  if (lex == JG_COLON) {
    if (b != ':') return false;
    s.lex = JG_VALUE;
    return true;
  }
  if (lex == JG_VALUE || lex == JG_ARR_FIRST) {
    if (b == ']' && lex == JG_ARR_FIRST) { jg_pop(s); return true; }
    return jg_value_start(s, b);
  }
  // JG_AFTER
  const bool arr = (s.stack >> (s.depth - 1)) & 1u;
  if (b == ',') { s.lex = arr ? JG_VALUE : JG_OBJ_KEY; return true; }
  if ((b == ']' && arr) || (b == '}' && !arr)) { jg_pop(s); return true; }
  return false;
}

// walk data[a .. e) (e > a) from s; the table is read as aligned dwords (it carries 4 bytes of padding)
__device__ __forceinline__ bool jg_walk(JState& s, const unsigned* __restrict__ data32, int a, int e) {
  unsigned word = data32[a >> 2];
  for (int j = a; j < e; ++j) {
    if ((j & 3) == 0 && j != a) word = data32[j >> 2];
    if (!jg_step(s, (word >> (8 * (j & 3))) & 0xFFu)) return false;
  }
  return true;
}

// json_grammar.advance: fold one picked token; a rejected one sets the error bit and leaves the rest as it was
__device__ __forceinline__ void jg_fold(JState& s, int tok, const int* __restrict__ off, const unsigned* __restrict__ data32,
                                       const unsigned char* __restrict__ flags, int V) {
  if (s.err) return;
  if (tok < 0 || tok >= V) { s.err = 1; return; }
  if (flags[tok] & JG_FLAG_EOS) {
    if (s.lex != JG_DONE) s.err = 1;
    return;
  }
  const int a = off[tok], e = off[tok + 1];
  JState l = s;
  if (a < e && jg_walk(l, data32, a, e)) s = l;
  else s.err = 1;
}

__global__ __launch_bounds__(256) void json_mask_kernel(int* __restrict__ state, const int* __restrict__ tokens,
                                                        int max_tokens, const int* __restrict__ step_ptr,
                                                        const int* __restrict__ off, const unsigned* __restrict__ data32,
                                                        const unsigned char* __restrict__ flags,
                                                        const int* __restrict__ eos_ids, int n_eos, int V,
                                                        unsigned long long* __restrict__ allow, int ld_allow) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y;
  int* __restrict__ st = state + (size_t)row * JG_STATE_INTS;
  const int step = step_ptr[row];
  const int* __restrict__ rd = st + (step & 1) * JG_SLOT_INTS;
  JState s;
  s.lex = rd[JW_LEX]; s.depth = rd[JW_DEPTH]; s.stack = (unsigned)rd[JW_STACK]; s.ws = rd[JW_WS]; s.utf = rd[JW_UTF];
  s.aux = rd[JW_AUX]; s.key = rd[JW_KEY]; s.err = rd[JW_ERR];
  const int pos = rd[JW_ANCHOR] ? rd[JW_POS] : step;
  const int end = min(step, max_tokens);
  const int* __restrict__ toks = tokens + (size_t)row * max_tokens;
  for (int p = max(pos, 0); p < end; ++p) jg_fold(s, toks[p], off, data32, flags, V);
  int* __restrict__ wr = st + ((step + 1) & 1) * JG_SLOT_INTS;
  if (blockIdx.x == 0 && tid == 0) {
    wr[JW_LEX] = s.lex; wr[JW_DEPTH] = s.depth; wr[JW_STACK] = (int)s.stack; wr[JW_WS] = s.ws; wr[JW_UTF] = s.utf;
    wr[JW_AUX] = s.aux; wr[JW_KEY] = s.key; wr[JW_ERR] = s.err; wr[JW_POS] = step; wr[JW_ANCHOR] = 1;
  }

  const int nwords = (V + 63) >> 6;
  const bool plain_ok = s.lex == JG_STR && (s.utf & 0xFF) == 0 && !s.err;
  const bool done = s.lex == JG_DONE;
  unsigned long long* __restrict__ out = allow + (size_t)row * ld_allow;
  int cnt = 0;
  for (int w = blockIdx.x * 4 + wave; w < nwords; w += gridDim.x * 4) {
    const int t = w * 64 + lane;
    bool ok = false;
    if (t < V && !s.err) {
      const unsigned f = flags[t];
      if (f & JG_FLAG_EOS) ok = done;
      else if (plain_ok && (f & JG_FLAG_PLAIN)) ok = true;
      else if (!done) {
        const int a = off[t], e = off[t + 1];
        if (a < e) {
          JState l = s;
          ok = jg_walk(l, data32, a, e);
        }
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
    if (wg_cnt) atomicAdd(&st[JG_COUNT], wg_cnt);
    __threadfence();                                     // this workgroup's words (and workgroup 0's state) before its ticket
    wg_last = atomicAdd(&st[JG_TICKET], 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!wg_last || tid != 0) return;
  __threadfence();
  if (atomicAdd(&st[JG_COUNT], 0) == 0) {                // no token allowed: EOS instead, and the request is marked failed
    for (int i = 0; i < n_eos; ++i) {
      const int id = eos_ids[i];
      if (id >= 0 && id < V) atomicOr(&out[id >> 6], 1ull << (id & 63));
    }
    wr[JW_ERR] = 1;
  }
  st[JG_COUNT] = 0;                                      // every workgroup has counted: reset for the next launch
  st[JG_TICKET] = 0;
}

extern "C" int vis_json_mask(void* state, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                             const void* tok_bytes, const void* tok_flags, const void* eos_ids, int n_eos, int V,
                             void* allow, int ld_allow, int batch, hipStream_t stream) {
  if (!state || !tokens || !step_ptr || !tok_off || !tok_bytes || !tok_flags || !eos_ids || !allow) return VIS_ERR_ARG;
  if (V <= 0 || V > JM_MAXV || max_tokens <= 0 || n_eos < 1 || n_eos > 64 || batch < 1 || batch > JM_MAXBATCH)
    return VIS_ERR_ARG;
  if (ld_allow < (V + 63) / 64 || ((uintptr_t)allow & 7) || ((uintptr_t)tok_bytes & 3) || ((uintptr_t)state & 3))
    return VIS_ERR_ARG;
  const int nwords = (V + 63) / 64;
  // four words per workgroup until the grid holds ~2 waves per SIMD over the batch, then several words per wave
  int blocks = (nwords + 3) / 4;
  const int cap = max(1, 2048 / batch);
  if (blocks > cap) blocks = cap;
  vis_clear_error();
  hipLaunchKernelGGL(json_mask_kernel, dim3(blocks, batch), dim3(256), 0, stream, (int*)state, (const int*)tokens,
                     max_tokens, (const int*)step_ptr, (const int*)tok_off, (const unsigned*)tok_bytes,
                     (const unsigned char*)tok_flags, (const int*)eos_ids, n_eos, V, (unsigned long long*)allow, ld_allow);
  return vis_check_launch();
}
