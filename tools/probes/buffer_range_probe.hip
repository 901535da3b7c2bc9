// Probe: which part of a buffer LDS-DMA load's address does the descriptor's range check see?
// The prefill attention kernels (csrc/attn_prefill.hip) fetch K tiles through att_tile_dma16 (csrc/attn_tile_dma.hip.h) with the
// per-lane offset in a VGPR and the tile's position in the instruction's SCALAR offset, under a descriptor of
// num_records = k_tokens * row bytes.  On the ragged last tile base + scalar + vector passes num_records although the vector
// offset alone does not.  This program calls that same helper on a buffer it owns and prints what arrives in LDS.
//
// One device allocation; of its first ALLOC bytes - the only ones a load can reach - the first num_records bytes hold data (word i = DATA0 + i), everything behind them
// POISON (a non-zero word that is no NaN as bf16).  One wave loads 64 pieces of 16 bytes, lane l from
// base + soffset + voffset0 + 16 l, into an LDS image pre-set to UNTOUCHED, and copies the image out.  Per row size (160 and 256
// bytes, the two kernels'; 10 rows) four launches:
//   a  scalar offset in range, vector offsets in range                        -> data
//   b  scalar offset 0, vector offsets straddle num_records                   -> data, then zeros (the documented check)
//   c  scalar offset past num_records, vector offsets small
//   d  scalar offset in range, vector offsets in range, the SUM straddles num_records (the kernels' ragged last tile)
// Safety: before every launch the host asserts soffset + largest voffset + 16 + SLACK <= ALLOC, so every address a launch can
// form lies inside the allocation whatever the hardware checks.  Nothing here can fault.
// Output: per case the class of every piece (zeros / poison / data / untouched / mixed) as runs, one CASE line with counts
// (read by tests/test_buffer_range_gpu.py), then the verdict `soffset range-checked: yes|no`.  Exit 0 unless a HIP call failed
// (2) or the pieces past the range are neither all zeros nor all poison (1).
// Build: make -C vision-inspection-system_amd/csrc   (-> csrc/buffer_range_probe; recorded run: profiles/buffer_range_probe.txt)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "../../vision-inspection-system_amd/csrc/attn_tile_dma.hip.h"

typedef uint32_t pr_u32x4 __attribute__((ext_vector_type(4)));

static constexpr uint32_t POISON = 0x5a5a5a5au, UNTOUCHED = 0x0e0e0e0eu, DATA0 = 0x11110000u;
static constexpr uint32_t ALLOC = 65536, SLACK = 4096, PIECES = 64, ROWS = 10;

__global__ __launch_bounds__(64) void probe_kernel(const void* base, int num_records, uint32_t voffset0, int soffset, uint32_t* out) {
  __shared__ __attribute__((aligned(16))) char lds[PIECES * 16];
  const int lane = threadIdx.x;
  *(pr_u32x4*)(lds + lane * 16) = (pr_u32x4){UNTOUCHED, UNTOUCHED, UNTOUCHED, UNTOUCHED};
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, num_records, 0x00020000);
  att_tile_dma16(rs, (att_lds_void*)lds, voffset0 + (uint32_t)lane * 16, soffset);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  *(pr_u32x4*)(out + lane * 4) = *(const pr_u32x4*)(lds + lane * 16);
}

#define HIP_OK(call)                                                                        \
  do {                                                                                      \
    const hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                                 \
      printf("HIP error: %s at %s:%d - stopping\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      fflush(stdout);                                                                       \
      exit(2);                                                                              \
    }                                                                                       \
  } while (0)

enum Cls { ZEROS, POISONED, DATA, UNTOUCHED_, MIXED, NCLS };
static const char* const CLS_NAME[NCLS] = {"zeros", "poison", "data", "untouched", "mixed"};

static Cls classify(const uint32_t* w, uint32_t addr) {
  bool z = true, p = true, d = true, u = true;
  for (int j = 0; j < 4; ++j) {
    z &= w[j] == 0;
    p &= w[j] == POISON;
    u &= w[j] == UNTOUCHED;
    d &= w[j] == DATA0 + addr / 4 + j;
  }
  return z ? ZEROS : p ? POISONED : d ? DATA : u ? UNTOUCHED_ : MIXED;
}

struct Tally { int past[NCLS] = {0, 0, 0, 0, 0}; };

// One launch.  `in` / `past`: pieces wholly below / at or past num_records; the counts of the latter are added to *tally.
static void run_case(const char* name, uint32_t row_bytes, uint32_t voffset0, uint32_t soffset, char* dbuf,
                     uint32_t* dout, Tally* tally) {
  const uint32_t num_records = ROWS * row_bytes;
  const uint32_t bound = soffset + voffset0 + (PIECES - 1) * 16 + 16;   // one past the last byte any lane can address
  if (bound + SLACK > ALLOC || num_records + SLACK > ALLOC) {
    printf("case %s: address bound %u + slack %u exceeds the allocation of %u bytes - not launched\n", name, bound, SLACK, ALLOC);
    exit(3);
  }
  std::vector<uint32_t> host(ALLOC / 4, POISON);
  for (uint32_t i = 0; i < num_records / 4; ++i) host[i] = DATA0 + i;
  HIP_OK(hipMemcpy(dbuf, host.data(), ALLOC, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dout, 0xcc, PIECES * 16));
  hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, 0, dbuf, (int)num_records, voffset0, (int)soffset, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  uint32_t img[PIECES * 4];
  HIP_OK(hipMemcpy(img, dout, sizeof img, hipMemcpyDeviceToHost));

  printf("case %s%u: row bytes %u, num_records %u, soffset %u, voffset %u..%u, largest address formed %u of %u\n", name, row_bytes,
         row_bytes, num_records, soffset, voffset0, voffset0 + (PIECES - 1) * 16, bound, ALLOC);
  Cls cls[PIECES];
  int n_in = 0, in_data = 0, n_past = 0, past[NCLS] = {0, 0, 0, 0, 0};
  for (uint32_t l = 0; l < PIECES; ++l) {
    const uint32_t addr = soffset + voffset0 + l * 16;
    cls[l] = classify(img + 4 * l, addr);
    if (addr + 16 <= num_records) { ++n_in; in_data += cls[l] == DATA; }
    else { ++n_past; ++past[cls[l]]; if (tally) ++tally->past[cls[l]]; }
  }
  printf("  pieces:");
  for (uint32_t l = 0; l < PIECES;) {
    uint32_t e = l;
    while (e + 1 < PIECES && cls[e + 1] == cls[l]) ++e;
    printf(" %u-%u %s%s", l, e, CLS_NAME[cls[l]], e + 1 < PIECES ? "," : "\n");
    l = e + 1;
  }
  printf("CASE %s%u in=%d in_data=%d past=%d past_zeros=%d past_poison=%d past_other=%d\n", name, row_bytes, n_in, in_data, n_past,
         past[ZEROS], past[POISONED], n_past - past[ZEROS] - past[POISONED]);
  fflush(stdout);
}

int main() {
  char* dbuf = nullptr;
  HIP_OK(hipMalloc(&dbuf, ALLOC + PIECES * 16));               // the loads' ALLOC bytes, then the 1 KiB the kernel copies its LDS image to
  uint32_t* dout = (uint32_t*)(dbuf + ALLOC);
  printf("buffer LDS-DMA range-check probe: one allocation of %u bytes, data word i = 0x%08x + i below num_records, poison 0x%08x behind, "
         "LDS preset 0x%08x; %u pieces of 16 bytes per launch\n", ALLOC, DATA0, POISON, UNTOUCHED, PIECES);
  Tally scalar_past;
  for (uint32_t rb : {160u, 256u}) {
    const uint32_t n = ROWS * rb;
    run_case("a", rb, 0, 2 * rb, dbuf, dout, nullptr);
    run_case("b", rb, n - PIECES * 8, 0, dbuf, dout, nullptr);
    run_case("c", rb, 0, n + rb, dbuf, dout, &scalar_past);
    run_case("d", rb, 0, 8 * rb, dbuf, dout, &scalar_past);
  }
  HIP_OK(hipFree(dbuf));
  int total = 0;
  for (int c = 0; c < NCLS; ++c) total += scalar_past.past[c];
  if (scalar_past.past[ZEROS] == total) { printf("soffset range-checked: yes\n"); return 0; }
  if (scalar_past.past[POISONED] == total) { printf("soffset range-checked: no\n"); return 0; }
  printf("soffset range-checked: inconclusive (cases c and d, pieces past num_records: %d zeros, %d poison, %d other of %d)\n",
         scalar_past.past[ZEROS], scalar_past.past[POISONED], total - scalar_past.past[ZEROS] - scalar_past.past[POISONED], total);
  return 1;
}
