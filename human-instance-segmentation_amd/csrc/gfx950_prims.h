// The gfx950 primitives every LDS-DMA kernel file shares: buffer resources, the LDS-DMA load, counted waits, the
// transposing LDS read, the LDS swizzles and the XCD-major workgroup remap.  Each is defined here once; a kernel
// file includes this header (through conv_common.h / wgrad_common.h) and does not redefine any of it (DESIGN.md
// "Shared gfx950 primitives").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hiseg {

// ---- vector (MFMA operand / accumulator, buffer load) and LDS address-space types
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) char lds_char;

// ---- buffer resources
// Raw (stride 0) buffer over [p, p + bytes): an offset >= bytes is out of range, its load returns zeros (through
// LDS-DMA: writes zeros to LDS) and its store is dropped.
constexpr int kBufRsrcFlags = 0x00020000;     // word 3 of the descriptor: BUF_DATA_FORMAT_32, raw addressing
constexpr unsigned kOobOffset = 0x80000000u;  // >= num_records of any resource (at most 2^31 - 1 bytes)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, kBufRsrcFlags);
}

// ---- LDS-DMA
// One 16-B-per-lane LDS-DMA (1 KiB per wave instruction): lane l's 16 bytes at rsrc + voff land at LDS byte
// lds_addr + 16 l.  Written as inline asm so that hipcc's waitcnt pass does not see it: the compiler would
// otherwise drain vmcnt(0) before the first ds_read after every issue (LDS-DMA writes alias the LDS the MFMAs read),
// which serialises the ring.  Completion is tracked by the callers' explicit counted vm_wait
// (cdna_hip_programming.md §5.7 item 1).  M0 (the LDS base of the instruction) is written inside the same statement,
// so the compiler can neither schedule another M0 user between the two nor reuse a stale M0; lds_addr must be
// wave-uniform and goes through readfirstlane, so the "s" operand holds whether or not the compiler proved that.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned lds_addr, unsigned voff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :: "s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff), "s"(rsrc) : "memory");
}

// Wait until at most N of the wave's vector-memory operations (LDS-DMAs included) are still in flight.
template <int N>
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// ---- transposing LDS read (ds_read_b64_tr_b16, cdna_hip_programming.md T10): per 16-lane group a 4-row x 16-column
// block of 16-bit elements arrives column-major; two reads give one 16x16x32 MFMA operand
__device__ __forceinline__ i16x4 lds_read_tr16(const lds_char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p);
}
__device__ __forceinline__ i16x4 lds_read_tr16(unsigned byte_addr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(uintptr_t)byte_addr);
}

// ---- LDS swizzles: chunk c (16 B) of row r sits at slot c ^ f(r).  The DMA writes lane-linearly, so a loader
// applies f on the SOURCE address and a reader on the LDS address; kernel families that must agree bit for bit
// (conv_resblock keeps conv_hwc's layout) agree because they call the same function.
// 64-B halo rows read from any starting row (the 3x3 taps shift the fragment's 16 rows by 0..2)
__device__ __forceinline__ int halo_row_swz(int r) { return ((r >> 2) & 1) << 1; }
// 64-B weight rows read as fragments of rows r .. r + 15 with 16 | r
__device__ __forceinline__ int weight_row_swz(int r) { return (-(r >> 2)) & 3; }
// 256-B image rows (16 chunks) read by lds_read_tr16 (T10 (b)): the chunk term, and the byte offset of chunk ch of
// row `row`
__device__ __forceinline__ int tr_image_chunk_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ unsigned tr_image_swz(int row, int ch) {
  return 256u * (unsigned)row + 16u * (unsigned)(ch ^ tr_image_chunk_swz(row));
}

// ---- XCD-major bijective workgroup remap.  The hardware deals consecutive workgroup ids round-robin over the 8
// XCDs; this maps dispatch id `block` of `nblocks` so that XCD x (the ids = x mod 8) owns one contiguous run of
// remapped ids, the runs ascending in x and their lengths differing by at most one (the first nblocks % 8 XCDs get
// the longer runs).  Workgroups whose remapped ids are close -- the tiles a kernel orders fastest -- then run on one
// XCD at about the same time and share its L2.  tests/test_xcd_remap.py proves the bijection on the host.
__host__ __device__ __forceinline__ int xcd_major(int block, int nblocks) {
  const int q8 = nblocks >> 3, r8 = nblocks & 7, xcd = block & 7, loc = block >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
}

}  // namespace hiseg
