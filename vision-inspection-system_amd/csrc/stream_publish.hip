// Token-by-token publication of a reply while the decode loop runs (vis_stream_publish), and the host memory it writes
// (vis_host_coherent_alloc / vis_host_free).  One launch after each pick, BEHIND vis_stop_scan: it counts no bytes and finds
// no EOS itself - state, bytes so far, reason and cut come from the row's stop-scan record, so the stop scan is on whenever
// streaming is (with the request's stop strings, or with an automaton of the start state alone).  stream.py is the reference
// of the tests (publish_ref) and the reader side.
//
// What it writes is HOST memory the GPU stores to coherently (hipHostMalloc, coherent + mapped): per row an append-only array
// of 16-byte records indexed like the token row - the token picked at position p has record p - plus one `count` word and
// one `start` word.  Record = {token id, safe_bytes, status, cut}, ONE 16-byte vector store:
//   safe_bytes  bytes of the reply's byte stream that can no longer be taken back: for an open row bytes so far minus
//               depth[state], the length of the longest suffix of the text that is a prefix of a stop string; on EOS the
//               bytes in front of the EOS token; on a stop match the offset where the match starts (= cut)
//   status      0 open, 1 EOS, 2 stop (the stop scan's reason)
// start[row] is stored with the row's first record (the position of the first generated token), count[row] = step after the
// record, as a system-scope release store: a host that reads count == c with a plain aligned load may read the records
// [start, c).  Nothing published is ever rewritten, so the host needs no seqlock and a slow reader loses nothing.
//
// Two rules keep the arrays consistent.  `pub` (device memory, int32 per row, zero = fresh) mirrors count: a launch repeated
// at the same step finds pub == step and changes nothing (the warm-up of a graph capture, vis_stop_scan's rule).  A row whose
// stop-scan record has ended is published once, at the step that ended it (EOS: pos == step - 1, stop: pos == step); from
// then on its count is frozen, which is how the reader learns that it is done.  A position at or beyond `capacity` or
// `max_tokens` is never written.
//
// One wave per row, lane 0 works: a dozen dependent loads and three stores.
#include "common.hip.h"
#include <string.h>

#define SP_STATE_INTS 8          // SS_STATE_INTS of stop_scan.hip
#define SP_MAX_STATES 257        // SS_MAX_STATES
#define SP_MAXBATCH 64
#define SP_RECORD_INTS 4

typedef int sp_i32x4 __attribute__((ext_vector_type(4)));

// words of the stop-scan record (stop_scan.hip)
enum { SP_STATE, SP_POS, SP_BYTES, SP_REASON, SP_NTOK, SP_CUT, SP_WHICH, SP_ANCHOR };

__global__ __launch_bounds__(64) void stream_publish_kernel(
    const int* __restrict__ stop_state, const int* __restrict__ tokens, int max_tokens, const int* __restrict__ step_ptr,
    const unsigned char* __restrict__ depth, int n_states, int* __restrict__ pub, int* __restrict__ records, int capacity,
    int* __restrict__ count, int* __restrict__ start) {
  if (threadIdx.x != 0) return;
  const int row = blockIdx.x;
  const int step = step_ptr[row];
  if (step < 1 || step > max_tokens || step > capacity) return;      // position step - 1 lies outside the arrays
  const int seen = pub[row];
  if (seen >= step) return;                                          // the same step again
  const sp_i32x4* __restrict__ rec = (const sp_i32x4*)(stop_state + (size_t)row * SP_STATE_INTS);
  const sp_i32x4 lo = rec[0], hi = rec[1];
  if (!hi[SP_ANCHOR - 4]) return;                                    // no stop scan has run for this row yet
  const int reason = lo[SP_REASON], pos = lo[SP_POS];
  // an ended row is published at the step that ended it and never again; an open row has folded every token up to step
  if (pos != (reason == 1 ? step - 1 : step)) return;
  int safe;
  if (reason == 0) {
    const int s = lo[SP_STATE];
    const int d = (s >= 0 && s < n_states) ? (int)depth[s] : 0;
    safe = max(lo[SP_BYTES] - d, 0);
  } else {
    safe = hi[SP_CUT - 4];
  }
  sp_i32x4 o;
  o[0] = tokens[(size_t)row * max_tokens + (step - 1)];
  o[1] = safe;
  o[2] = reason;
  o[3] = reason ? hi[SP_CUT - 4] : 0;
  if (seen == 0) start[row] = step - 1;
  *(sp_i32x4*)(records + ((size_t)row * capacity + (step - 1)) * SP_RECORD_INTS) = o;
  __hip_atomic_store(count + row, step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  pub[row] = step;
}

extern "C" int vis_stream_publish(const void* stop_state, const void* tokens, int max_tokens, const void* step_ptr,
                                  const void* depth, int n_states, void* pub, void* records, int capacity, void* count,
                                  void* start, int batch, hipStream_t stream) {
  if (!stop_state || !tokens || !step_ptr || !depth || !pub || !records || !count || !start) return VIS_ERR_ARG;
  if (max_tokens <= 0 || capacity < max_tokens || batch < 1 || batch > SP_MAXBATCH) return VIS_ERR_ARG;
  if (n_states < 1 || n_states > SP_MAX_STATES) return VIS_ERR_ARG;
  if (((uintptr_t)stop_state & 15) || ((uintptr_t)records & 15) || ((uintptr_t)tokens & 3) || ((uintptr_t)step_ptr & 3) ||
      ((uintptr_t)pub & 3) || ((uintptr_t)count & 3) || ((uintptr_t)start & 3))
    return VIS_ERR_ARG;
  vis_clear_error();
  hipLaunchKernelGGL(stream_publish_kernel, dim3(batch), dim3(64), 0, stream, (const int*)stop_state, (const int*)tokens,
                     max_tokens, (const int*)step_ptr, (const unsigned char*)depth, n_states, (int*)pub, (int*)records,
                     capacity, (int*)count, (int*)start);
  return vis_check_launch();
}

// Host memory for vis_stream_publish: page-locked, mapped into the device's address space and COHERENT (fine-grained: a
// store of a running kernel becomes visible to the host without waiting for the kernel to end).  Zero-filled.  *host_ptr is
// the address the host reads, *dev_ptr the one a kernel is given.
extern "C" int vis_host_coherent_alloc(void** host_ptr, void** dev_ptr, long long bytes) {
  if (!host_ptr || !dev_ptr || bytes <= 0 || bytes > (1ll << 32)) return VIS_ERR_ARG;
  void* p = nullptr;
  void* d = nullptr;
  if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess || !p) return VIS_ERR_LAUNCH;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess || !d) {
    (void)hipHostFree(p);
    return VIS_ERR_LAUNCH;
  }
  ::memset(p, 0, (size_t)bytes);
  *host_ptr = p;
  *dev_ptr = d;
  return VIS_OK;
}

extern "C" int vis_host_free(void* host_ptr) {
  if (!host_ptr) return VIS_ERR_ARG;
  return hipHostFree(host_ptr) == hipSuccess ? VIS_OK : VIS_ERR_LAUNCH;
}
