// The constants and the byte walk of schema_mask.hip (vis_schema_mask) for the schema kernels outside that file
// (spec_schema.hip: the speculative step under a schema).  schema_mask.hip keeps its own copy - the tests read its defines
// there; tests/test_schema_draft.py holds the two against each other, define by define and the walk line by line.
#pragma once
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
