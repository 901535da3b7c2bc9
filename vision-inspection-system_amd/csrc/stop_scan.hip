// Stop sequences and how a reply ended (vis_stop_scan): one launch after each pick folds the bytes of the tokens picked since
// the row's last launch through the Aho-Corasick automaton of the request's stop strings and keeps one sticky record per row.
// stop.py compiles the tables and is the reference of the tests (scan).
//
// The automaton is data, as vis_schema_mask's: trans [n_states][n_classes] u16 packed at the front of a buffer of fixed
// capacity, byte_class [256] u8, hits [cap_states][2] u8 = (length of the longest stop string that is a suffix at the state,
// its index), and a header {n_states, n_classes, 0, 0} the kernel READS - a decode graph captured under one stop set serves
// the next one after the host has overwritten the buffers.  Failure links are resolved into trans, so a byte costs one
// lookup, s = trans[s * n_classes + byte_class[b]]; bit 15 of an entry says that its target state ends a stop string, so hits
// is read once per reply, not once per byte.  A header outside the capacities switches the walk off (EOS is still seen); a
// state or class outside the header is clamped, never used as an index.
//
// Record: int32 [batch][SS_STATE_INTS] - DFA state, position (the next token of the row to fold), bytes so far, reason
// (0 open, 1 EOS, 2 stop), tokens kept (EOS: exclusive; stop: through the token that completed the match), cut (byte offset
// where the match starts; EOS: bytes so far), which stop string, anchored.  All zero = a fresh sequence: its first launch
// folds the one token just picked (position step - 1) and anchors the record.  A launch repeated at the same step finds
// position == step and changes nothing; a row with reason != 0 is never written again.
//
// The work per row is a dependent walk of a handful of bytes: one wave per row, lane 0 walks, the record is read and written
// as two 16-byte vectors.
#include "common.hip.h"

#define SS_MAX_STATES 257        // stop.MAX_STATES: 4 strings x 64 bytes + the start state
#define SS_MAX_CLASSES 256       // stop.MAX_CLASSES
#define SS_HIT 0x8000u           // stop.HIT
#define SS_STATE_INTS 8
#define SS_FLAG_EOS 1            // token flags (json_grammar.FLAG_EOS)
#define SS_MAXBATCH 64
#define SS_MAXV 262144

typedef int i32x4 __attribute__((ext_vector_type(4)));

// record words (stop.STATE .. ANCHOR)
enum { SS_STATE, SS_POS, SS_BYTES, SS_REASON, SS_NTOK, SS_CUT, SS_WHICH, SS_ANCHOR };

__global__ __launch_bounds__(64) void stop_scan_kernel(
    int* __restrict__ state, const int* __restrict__ tokens, int max_tokens, const int* __restrict__ step_ptr,
    const int* __restrict__ off, const unsigned* __restrict__ data32, const unsigned char* __restrict__ flags, int V,
    const int* __restrict__ header, const unsigned short* __restrict__ trans, const unsigned char* __restrict__ byte_class,
    const unsigned char* __restrict__ hits, int cap_states, int cap_classes, int eos_on) {
  if (threadIdx.x != 0) return;
  const int row = blockIdx.x;
  i32x4* __restrict__ rec = (i32x4*)(state + (size_t)row * SS_STATE_INTS);
  const i32x4 lo = rec[0], hi = rec[1];
  if (lo[SS_REASON] != 0) return;                                    // sticky
  const int step = step_ptr[row];
  unsigned n_states = (unsigned)header[0], n_classes = (unsigned)header[1];
  const bool walk = n_states >= 1 && n_states <= (unsigned)cap_states && n_classes >= 1 && n_classes <= (unsigned)cap_classes;
  const int anchored = hi[SS_ANCHOR - 4];
  unsigned s = anchored ? (unsigned)lo[SS_STATE] : 0u;
  if (!walk || s >= n_states) s = 0;
  int pos = anchored ? lo[SS_POS] : step - 1;
  int nbytes = anchored ? lo[SS_BYTES] : 0, ntok = anchored ? hi[SS_NTOK - 4] : 0;
  int reason = 0, cut = 0, which = 0;
  const int end = min(step, max_tokens);
  const int* __restrict__ toks = tokens + (size_t)row * max_tokens;
  if (pos < 0) pos = 0;
  if (anchored && pos >= end) return;                                // the same step again: nothing to fold, nothing to write
  for (; pos < end && !reason; ++pos) {
    const int tok = toks[pos];
    const bool inside = tok >= 0 && tok < V;
    if (inside && eos_on && (flags[tok] & SS_FLAG_EOS)) {
      reason = 1; cut = nbytes;
      break;
    }
    ++ntok;
    if (!inside || !walk) continue;
    const int a = off[tok], e = off[tok + 1];
    if (a >= e) continue;
    unsigned word = data32[a >> 2];
    for (int j = a; j < e; ++j) {
      if ((j & 3) == 0 && j != a) word = data32[j >> 2];
      unsigned c = byte_class[(word >> (8 * (j & 3))) & 0xFFu];
      if (c >= n_classes) c = n_classes - 1;
      const unsigned t = trans[s * n_classes + c];
      s = t & 0x7FFFu;
      if (s >= n_states) s = 0;
      ++nbytes;
      if (t & SS_HIT) {
        const int len = hits[2 * s];
        reason = 2; which = hits[2 * s + 1]; cut = max(nbytes - len, 0);
        break;
      }
    }
  }
  i32x4 o0, o1;
  o0[SS_STATE] = (int)s; o0[SS_POS] = pos; o0[SS_BYTES] = nbytes; o0[SS_REASON] = reason;
  o1[SS_NTOK - 4] = ntok; o1[SS_CUT - 4] = cut; o1[SS_WHICH - 4] = which; o1[SS_ANCHOR - 4] = 1;
  rec[0] = o0;
  rec[1] = o1;
}

extern "C" int vis_stop_scan(void* state, const void* tokens, int max_tokens, const void* step_ptr, const void* tok_off,
                             const void* tok_bytes, const void* tok_flags, int V, const void* header, const void* trans,
                             const void* byte_class, const void* hits, int cap_states, int cap_classes, int eos_on, int batch,
                             hipStream_t stream) {
  if (!state || !tokens || !step_ptr || !tok_off || !tok_bytes || !tok_flags) return VIS_ERR_ARG;
  if (!header || !trans || !byte_class || !hits) return VIS_ERR_ARG;
  if (V <= 0 || V > SS_MAXV || max_tokens <= 0 || batch < 1 || batch > SS_MAXBATCH || (eos_on != 0 && eos_on != 1))
    return VIS_ERR_ARG;
  if (cap_states < 1 || cap_states > SS_MAX_STATES || cap_classes < 1 || cap_classes > SS_MAX_CLASSES) return VIS_ERR_ARG;
  if (((uintptr_t)state & 15) || ((uintptr_t)tok_bytes & 3) || ((uintptr_t)header & 3) || ((uintptr_t)trans & 1) ||
      ((uintptr_t)tokens & 3) || ((uintptr_t)step_ptr & 3) || ((uintptr_t)tok_off & 3))
    return VIS_ERR_ARG;
  vis_clear_error();
  hipLaunchKernelGGL(stop_scan_kernel, dim3(batch), dim3(64), 0, stream, (int*)state, (const int*)tokens, max_tokens,
                     (const int*)step_ptr, (const int*)tok_off, (const unsigned*)tok_bytes, (const unsigned char*)tok_flags, V,
                     (const int*)header, (const unsigned short*)trans, (const unsigned char*)byte_class,
                     (const unsigned char*)hits, cap_states, cap_classes, eos_on);
  return vis_check_launch();
}
