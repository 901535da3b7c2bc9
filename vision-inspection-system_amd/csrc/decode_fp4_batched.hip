// vis_gemm_decode_mxfp4: the batched decode projection (5..64 in-flight sequences) on OCP Microscaling FP4 weights.
//   sum_slot part[slot][m][n] = sum_k deq(Wq, Ws)[n][k] * bf16(x[m][k]),  f32 accumulation on the bf16 MFMA
// The structure is gemm_decode_stream_kernel's (gemm_bf16.hip): persistent workgroups, one per CU, each owning one
// contiguous range of the (128-column tile, K-step) sequence ("stream-K"), a ring of LDS-DMA stages with counted vmcnt
// waits and ONE barrier per step, all accumulator sets stored after the last K-step.  The weights arrive at a quarter
// of the bytes: v_cvt_scalef32_pk_bf16_fp4 turns a byte of codes times its block scale into an EXACT bf16 pair
// (decode_fp4.hip), so the arithmetic is the bf16 projection's on hip.dequantize_mxfp4(Wq, Ws).
// Algorithmic bytes per launch: N*K/2 (codes) + N*K/32 (scales) + B*K*2 (x) + the partial slabs.
//
// K-step = 256 elements: a tile row of codes is one full 128-byte line (8 MX blocks, 8 scale bytes).  K % 64 == 0 only,
// so the last step of a tile row may hold 2, 4 or 6 valid blocks: its loads are clamped to valid addresses of the
// same row and the consumer replaces codes of the blocks past K by 0 (= +0.0) and their scale by 1.
//
// One stage in LDS (MB = 16-row blocks of x, 1 / 2 / 4 for B <= 16 / 32 / 64):
//   x      [16 MB][512 B]   32 chunks of 16 B per row; chunk q of row r sits at position q ^ key(r),
//                           key(r) = (r & 15) ^ (((r >> 2) ^ (r >> 3)) & 1) << 2
//   codes  [128][128 B]     8 chunks (= MX blocks) per row; block c of row r sits at position c ^ (r & 7)
//   scales [128][16 B]      the four ALIGNED dwords that cover the row's 8 scale bytes of this step (a row of scales
//                           starts at any byte: lds = K/32 = 22 for K = 704), byte b of the step at offset mis + b,
//                           mis = (Ws + row * lds) & 3; dwords past the covered ones repeat the last one
// All three are filled by LDS-DMA (2 MB + 4 + 2 instructions per thread and stage), destination linear in the lane, the
// swizzle applied to the SOURCE chunk, as in the bf16 kernel.
//
// MFMA mapping.  v_mfma_f32_16x16x32_bf16(Wfrag, xfrag): lane (l15, h) supplies k-slots 8h..8h+7 of row l15.  A lane
// reads ONE 16-byte chunk of codes = one whole MX block (block 4g + h of the step, g = 0 / 1 the 128-element half) with
// one scale, and dword t of it feeds MFMA t = 0..3 of that half; k-slot 8h + e of MFMA t is element 128g + 32h + 8t + e,
// so the x fragment of lane (m, h) is x chunk 16g + 4h + t.  The permutation is the same for every B and row: the
// K order and the stream-K cut depend on (N, K) alone, MB changes the slab height only.
//
// Bank conflicts (ds_read_b128 is served in four groups of 16 lanes; a group holds all 16 values of l15, rows
// {0-3, 12-15} with one h and rows {4-11} with h ^ 1; 64 banks x 4 B = sixteen 16-byte slots per bank row):
//   codes: row stride 128 B -> slot = 8 (r & 1) + ((4g + h) ^ (r & 7)).  Two rows of one parity collide only if
//          h1 ^ h2 == (r1 ^ r2) & 7; within a group h1 ^ h2 is 0 (then r1 == r2 + 8, which are never both in the
//          same half of the group) or 1 (then the parities differ): conflict-free.
//   x:     row stride 512 B -> slot = position & 15 = (4h + t) ^ key(r).  The third term of key() flips bit 0 of h for
//          exactly the rows {4-11}, which undoes the group's h ^ 1: slot = (4 h0 + t) ^ (r & 15), 16 distinct values.
//   scales: ds_read_u8 of 64 lanes, rows at 16 B: rows r and r + 8 of a 32-lane group share banks (2-way) on 4 of the
//          4 + 4 + 8 MB reads of a step; the four lanes of a row read one dword (broadcast).
#include "decode_common.hip.h"

#define F4G_BN 128           // columns per tile
#define F4G_KS 256           // elements per K-step
#define F4G_MAX_WG 256       // one per CU
#define F4G_MAX_SLOTS 16
#define F4G_W_BYTES (F4G_BN * 128)
#define F4G_S_BYTES (F4G_BN * 16)

struct F4GemmArgs {
  const bf16_t* A;    // [M][lda]
  const uint8_t* Wq;  // [N][ldq]
  const uint8_t* Ws;  // [N][lds]
  float* part;        // [nslots][16 MB][N] or null
  void* C;            // direct output (part == null)
  int M, N, K, lda, ldq, lds, ldc;
  int nk_all, total, spb, nslots, out_f32;
};

template <int MB> struct F4Cfg {
  static constexpr int XI = 2 * MB;                                  // x LDS-DMA instructions per thread per stage
  static constexpr int PER = XI + 4 + 2;                             // all LDS-DMA instructions per thread per stage
  static constexpr int X_BYTES = 16 * MB * 512;
  static constexpr int STAGE_BYTES = X_BYTES + F4G_W_BYTES + F4G_S_BYTES;   // 26 / 34 / 50 KiB
  static constexpr int DEPTH = (MB == 1) ? 5 : (MB == 2) ? 4 : 3;
  static constexpr int LDS_BYTES = DEPTH * STAGE_BYTES;              // 130 / 136 / 150 KiB
  static_assert((DEPTH - 2) * PER <= 63, "vmcnt is a 6-bit counter");
};

// wait until all but the `younger` (0..DEPTH-2) most recent stages of this wave have landed
template <int PER>
__device__ __forceinline__ void f4g_wait_stages(int younger) {
  switch (younger) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PER) : "memory"); break;
  }
}

__device__ __forceinline__ int f4g_xkey(int r) { return (r & 15) ^ ((((r >> 2) ^ (r >> 3)) & 1) << 2); }

// eight codes (one dword) times the block scale as an exact bf16x8: byte b = elements 2b (low nibble), 2b + 1
__device__ __forceinline__ bf16x8 f4g_cvt8(uint32_t w, float scale) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  const bf16x4 lo = __builtin_shufflevector(p0, p1, 0, 1, 2, 3), hi = __builtin_shufflevector(p2, p3, 0, 1, 2, 3);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int MB>
__global__ __launch_bounds__(256, 1) void gemm_decode_mxfp4_kernel(F4GemmArgs p) {
  typedef F4Cfg<MB> Cfg;
  constexpr int XI = Cfg::XI, DEPTH = Cfg::DEPTH, STAGE_BYTES = Cfg::STAGE_BYTES, X_BYTES = Cfg::X_BYTES;
  constexpr int S_OFF = X_BYTES + F4G_W_BYTES;
  extern __shared__ __attribute__((aligned(16))) char lds4[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wn = tid >> 6;  // wave = 32-column slice
  const int l15 = lane & 15, h = lane >> 4;
  const int s0 = blockIdx.x * p.spb;
  const int nsteps = min(s0 + p.spb, p.total) - s0;
  if (nsteps <= 0) return;  // whole workgroup
  const int nblk = p.K >> 5;  // MX blocks per row

  int p_tile = s0 / p.nk_all, p_kt = s0 - p_tile * p.nk_all;  // producer cursor
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);

  auto stage = [&](int slot) {  // next step of this workgroup's range -> ring slot
    char* base = lds4 + slot * STAGE_BYTES;
    const int n0 = p_tile * F4G_BN;
    const int vb = min(8, nblk - p_kt * 8);  // valid blocks of this step: 8, or 2 / 4 / 6 in a ragged last step
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int c = i * 256 + tid;
      const int row = c >> 5;
      const int q = min((c & 31) ^ f4g_xkey(row), 4 * vb - 1);
      const char* src = (const char*)p.A + (size_t)min(row, p.M - 1) * p.lda * 2 + (size_t)p_kt * 512 + q * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(base + i * 4096 + wave_u * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = i * 256 + tid;
      const int row = c >> 3;
      const int ch = min((c & 7) ^ (row & 7), vb - 1);
      const uint8_t* src = p.Wq + (size_t)min(n0 + row, p.N - 1) * p.ldq + (size_t)p_kt * 128 + ch * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(base + X_BYTES + i * 4096 + wave_u * 1024),
                                       16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i * 256 + tid;
      const int row = c >> 2;
      const uint8_t* a = p.Ws + (size_t)min(n0 + row, p.N - 1) * p.lds + (size_t)p_kt * 8;
      const int mis = (int)((uintptr_t)a & 3);
      const int d = min(c & 3, (mis + vb - 1) >> 2);  // every dword read holds at least one scale byte of this row
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a - mis + 4 * d),
                                       (__attribute__((address_space(3))) void*)(base + S_OFF + i * 1024 + wave_u * 256), 4,
                                       0, 0);
    }
    if (++p_kt == p.nk_all) {
      p_kt = 0;
      ++p_tile;
    }
  };

  const int sw = lane & 7;
  const int xk = f4g_xkey(l15);

  int c_tile = s0 / p.nk_all, c_kt = s0 - c_tile * p.nk_all;  // consumer cursor
  const int pre = min(DEPTH - 1, nsteps);
  for (int s = 0; s < pre; ++s) stage(s);
  int slot = 0, fill = pre % DEPTH;  // slot consumed this step / slot refilled this step
  int st = 0;

  // one K-step (tile, kt) of the ring into `acc`
  auto step = [&](f32x4 (&acc)[MB][2], int tile, int kt) {
    f4g_wait_stages<Cfg::PER>(min(DEPTH - 2, nsteps - 1 - st));
    __builtin_amdgcn_s_barrier();  // stage st visible to all waves; every wave is past compute(st-1)
    if (st + DEPTH - 1 < nsteps) {
      stage(fill);
      fill = (fill + 1 == DEPTH) ? 0 : fill + 1;
    }
    const char* base = lds4 + slot * STAGE_BYTES;
    const int vb = min(8, nblk - kt * 8);
    int srow[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wn * 32 + j * 16 + l15;
      const uintptr_t a = (uintptr_t)p.Ws + (size_t)min(tile * F4G_BN + r, p.N - 1) * p.lds;
      srow[j] = S_OFF + r * 16 + (int)(a & 3);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (4 * g >= vb) break;  // workgroup-uniform: the whole half lies past K
      const bool ok = (4 * g + h) < vb;
      bf16x8 xa[MB][4];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          xa[mb][t] = *(const bf16x8*)(base + (mb * 16 + l15) * 512 + (((16 * g + 4 * h + t) ^ xk) << 4));
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        u32x4 w = *(const u32x4*)(base + X_BYTES + (wn * 32 + j * 16 + l15) * 128 + (((4 * g + h) ^ sw) << 4));
        const uint32_t sb = *(const uint8_t*)(base + srow[j] + 4 * g + h);
        float sc = __builtin_bit_cast(float, sb << 23);  // 2^(byte - 127)
        if (!ok) {  // block past K: the clamped load repeated a valid block of the row
          w = (u32x4){0u, 0u, 0u, 0u};
          sc = 1.0f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bf16x8 wf = f4g_cvt8(w[t], sc);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
            acc[mb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xa[mb][t], acc[mb][j], 0, 0, 0);
        }
      }
    }
    slot = (slot + 1 == DEPTH) ? 0 : slot + 1;
    ++st;
  };

  // flush of one tile segment: lane holds D[n = n0 + 32 wn + 16 j + 4 h + r][m = 16 mb + l15]
  auto flush = [&](f32x4 (&acc)[MB][2], int tile, bool tile_done) {
    const int nb = tile * F4G_BN + wn * 32 + 4 * h;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = mb * 16 + l15;
      if (m >= p.M) continue;
      if (p.part) {
        const int seg = blockIdx.x - (tile * p.nk_all) / p.spb;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = nb + j * 16;
          if (n >= p.N) continue;
          *(f32x4*)(p.part + ((size_t)seg * (16 * MB) + m) * p.N + n) = acc[mb][j];
          if (tile_done)
            for (int z = seg + 1; z < p.nslots; ++z)
              *(f32x4*)(p.part + ((size_t)z * (16 * MB) + m) * p.N + n) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = nb + j * 16;
          if (n >= p.N) continue;
          const f32x4 v = acc[mb][j];
          if (p.out_f32) {
            *(f32x4*)((float*)p.C + (size_t)m * p.ldc + n) = v;
          } else {
            u32x2 o;
            o[0] = pack2bf(v[0], v[1]);
            o[1] = pack2bf(v[2], v[3]);
            *(u32x2*)((bf16_t*)p.C + (size_t)m * p.ldc + n) = o;
          }
        }
      }
    }
  };

  // As in gemm_decode_stream_kernel: every tile a range touches gets its OWN accumulator set and ALL sets are stored
  // after the last K-step (a store issued while the ring runs sits in the same in-order vmcnt queue as the ring's
  // LDS-DMA loads, and the counted waits of the following steps would wait for it too).  Ranges that touch more than
  // NSEG tiles flush the oldest set on the spot.  (Four sets at MB = 4: six do not fit the 512 registers beside the
  // sixteen x fragments of a half step.)
  constexpr int NSEG = (MB == 4) ? 4 : 8;
  f32x4 accs[NSEG][MB][2];
  int seg_tile[NSEG];
  bool seg_done[NSEG];
  int nseg = 0;
#pragma unroll
  for (int sg = 0; sg < NSEG; ++sg) {
    seg_tile[sg] = 0;
    seg_done[sg] = false;
    if (st < nsteps) {  // workgroup-uniform
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        accs[sg][mb][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
        accs[sg][mb][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      for (;;) {
        const int n_here = min(nsteps - st, p.nk_all - c_kt);
        for (int i = 0; i < n_here; ++i) step(accs[sg], c_tile, c_kt + i);
        c_kt += n_here;
        const bool done = (c_kt == p.nk_all);
        seg_tile[sg] = c_tile;
        seg_done[sg] = done;
        if (done) { c_kt = 0; ++c_tile; }
        if (sg + 1 < NSEG || st >= nsteps) break;
        // last set and steps left: this tile is stored now and the set reused
        flush(accs[sg], seg_tile[sg], seg_done[sg]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          accs[sg][mb][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
          accs[sg][mb][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
      nseg = sg + 1;
    }
  }
#pragma unroll
  for (int sg = 0; sg < NSEG; ++sg)
    if (sg < nseg) flush(accs[sg], seg_tile[sg], seg_done[sg]);
}

// geometry of the stream-K cut for (N, K): steps per workgroup and the number of partial slots a tile can need
static void f4g_geometry(int N, int K, bool direct, int* spb, int* nslots, int* nwg) {
  const int tiles = (N + F4G_BN - 1) / F4G_BN, nk = (K + F4G_KS - 1) / F4G_KS;
  const long total = (long)tiles * nk;
  int wg = F4G_MAX_WG;
  for (;;) {
    long per;
    if (direct) {
      const long tpw = (tiles + wg - 1) / wg;  // whole tiles per workgroup
      per = tpw * nk;
    } else {
      per = (total + wg - 1) / wg;
      if (per < 4) per = total < 4 ? total : 4;  // never cut finer than 4 K-steps
    }
    int slots = 1;
    if (!direct)
      for (int t = 0; t < tiles; ++t) {
        const int s = (int)(((long)(t + 1) * nk - 1) / per - ((long)t * nk) / per) + 1;
        if (s > slots) slots = s;
      }
    if (slots <= F4G_MAX_SLOTS || wg == 1) {
      *spb = (int)per;
      *nslots = slots;
      *nwg = (int)((total + per - 1) / per);
      return;
    }
    wg = wg / 2;  // fewer, longer ranges -> fewer segments per tile
  }
}

extern "C" int vis_gemm_decode_mxfp4_ksplit(int N, int K) {
  if (N <= 0 || K < 64) return 0;
  int spb, slots, nwg;
  f4g_geometry(N, K, false, &spb, &slots, &nwg);
  return slots;
}

extern "C" int vis_gemm_decode_mxfp4(const void* A, const void* Wq, const void* Ws, void* part, void* C, int B, int N,
                                     int K, int lda, int ldq, int lds, int ldc, int ksplit, int out_f32,
                                     hipStream_t stream) {
  if (!A || !Wq || !Ws || (!part && !C) || B < 5 || B > 64 || N <= 0 || K <= 0) return VIS_ERR_ARG;
  if (K % 64 != 0 || N % 4 != 0 || lda % 8 != 0 || lda < K || ldq % 16 != 0 || ldq < K / 2 || lds < K / 32 ||
      (C && ldc % 4 != 0) || (!part && ldc < N))
    return VIS_ERR_ARG;
  if (((uintptr_t)A | (uintptr_t)Wq | (uintptr_t)part | (uintptr_t)C) & 15) return VIS_ERR_ARG;
  int spb, need, nwg;
  f4g_geometry(N, K, part == nullptr, &spb, &need, &nwg);
  if (part) {
    if (ksplit <= 0) ksplit = need;
    if (ksplit < need || ksplit > F4G_MAX_SLOTS) return VIS_ERR_ARG;
  } else {
    ksplit = 1;
  }
  static const bool attr_ok = [] {
    return hipFuncSetAttribute((const void*)gemm_decode_mxfp4_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               F4Cfg<1>::LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute((const void*)gemm_decode_mxfp4_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               F4Cfg<2>::LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute((const void*)gemm_decode_mxfp4_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               F4Cfg<4>::LDS_BYTES) == hipSuccess;
  }();
  if (!attr_ok) return VIS_ERR_LAUNCH;
  F4GemmArgs p;
  p.A = (const bf16_t*)A; p.Wq = (const uint8_t*)Wq; p.Ws = (const uint8_t*)Ws; p.part = (float*)part; p.C = C;
  p.M = B; p.N = N; p.K = K; p.lda = lda; p.ldq = ldq; p.lds = lds; p.ldc = ldc;
  p.nk_all = (K + F4G_KS - 1) / F4G_KS;
  p.total = ((N + F4G_BN - 1) / F4G_BN) * p.nk_all;
  p.spb = spb; p.nslots = ksplit; p.out_f32 = out_f32;
  vis_clear_error();
  if (B > 32) hipLaunchKernelGGL((gemm_decode_mxfp4_kernel<4>), dim3(nwg), dim3(256), F4Cfg<4>::LDS_BYTES, stream, p);
  else if (B > 16) hipLaunchKernelGGL((gemm_decode_mxfp4_kernel<2>), dim3(nwg), dim3(256), F4Cfg<2>::LDS_BYTES, stream, p);
  else hipLaunchKernelGGL((gemm_decode_mxfp4_kernel<1>), dim3(nwg), dim3(256), F4Cfg<1>::LDS_BYTES, stream, p);
  return vis_check_launch();
}
