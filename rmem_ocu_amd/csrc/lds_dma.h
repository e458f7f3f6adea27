// What the compute kernels that stage through LDS-DMA share (gemm_conv.hip, bottleneck.hip, bneck_block.hip, stem.hip,
// conv3x3_direct.hip, idbank.hip, rowchain.hip): the address-space pointer types, the buffer descriptor and its 16-byte load into
// LDS, the offset beyond every buffer and the size limit that goes with it, and the XOR swizzle of a 64-element tile row.  Helpers
// only: no kernel lives here.  (The strip kernels among them share more: strip_conv.h.)
//
// attention.hip keeps a private copy of the descriptor block (with make_rsrc(const void*, int)): bench.py ties the committed
// counter summary of that kernel to the sha256 of its source, so any edit there marks the roofline traffic stale until the
// counters are collected again.  The names and semantics here are the same, so the next change to that kernel can drop its copy
// and include this header instead.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(1))) const void* gptr_t;   // global_load_lds source
typedef __attribute__((address_space(3))) void* lptr_t;         // LDS-DMA destination

// Buffer-descriptor LDS-DMA (buffer_load_dwordx4 ... offen lds): no VGPR staging and no ds_write.  The descriptor type and these
// builtins exist only in the device pass of hipcc; the host pass just needs the names to parse, hence the empty twins.
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void buf_load_lds16(rsrc_t r, lptr_t dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 16, voff, soff, 0, 0);
}
#else
struct rsrc_t {};
__device__ inline rsrc_t make_rsrc(const void*, long) { return {}; }
__device__ inline void buf_load_lds16(rsrc_t, lptr_t, int, int) {}
#endif

// Byte offset beyond every buffer (descriptors span less than 2 GB).  The hardware range check of a buffer access turns it into
// a zero fill on loads -- a lane whose tap is padding, or whose row is past the last one, passes it instead of branching -- and
// into a dropped store on stores.
constexpr int OOB = (int)0x80000000;
// ... which entry points enforce: the bytes a descriptor spans, slack for a kernel's overshoot included, stay below this
constexpr long kRsrcLimit = (1L << 31) - (1L << 22);

// Element index of (row, 16-byte chunk) in a [rows][64] e16 panel.  Rows are 128 B (8 chunks of 16 B); physical chunk =
// chunk ^ ((row >> 1) & 7): the 16 lanes of every ds_read_b128 lane group (rows r..r+3, r+12..r+15 at chunk c and rows
// r+4..r+11 at chunk c+1) then land on 16 distinct 16-byte slots of the 256-byte bank row.  LDS-DMA fills a panel linearly,
// so a writer applies the swizzle to the per-lane SOURCE address and the reader to the fragment address.  Every kernel that
// writes or reads such a panel must use this one formula: the weight panels of gemm_conv.hip, bottleneck.hip and idbank.hip,
// and the A panels of the chain kernels (bottleneck.hip, rowchain.hip), where one phase writes what the next one reads.
__device__ __forceinline__ int swz(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 1) & 7)) << 3); }

}  // namespace
