// One 16-byte-per-lane piece of a K / V^T tile, global memory -> LDS, by buffer LDS-DMA (buffer_load_dwordx4 ... offen lds).
// Shared by attn_vit32_kernel and attn_prefill_pair_kernel (attn_prefill.hip) and by tools/probes/buffer_range_probe.hip,
// which measures what this very load form delivers when an address passes the descriptor's num_records.
//
// A lane reads base(rs) + lane_off + tile_off: lane_off (a loop constant of the kernels) is the instruction's vector offset,
// tile_off (the tile's position, wave-uniform) its scalar offset - no per-tile vector arithmetic.  Measured on the MI355X
// (profiles/buffer_range_probe.txt): the range check applies to the SUM of the two offsets - a piece at or past num_records
// arrives in LDS as zeros whether the vector or the scalar part carried it there - although LLVM's description of the raw
// buffer intrinsics and the ISA text exclude the scalar offset from the check.  tests/test_buffer_range_gpu.py holds that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __attribute__((address_space(3))) void att_lds_void;

__device__ __forceinline__ void att_tile_dma16(__amdgpu_buffer_rsrc_t rs, att_lds_void* dst, uint32_t lane_off, int tile_off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, lane_off, tile_off, 0, 0);
}
