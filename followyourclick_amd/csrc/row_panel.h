// What the register-resident row-panel kernels share (ff_block.hip, temporal_block_rr.hip, panel_linear.hip, and the LDS-tile
// temporal_block.hip that dispatches into the second): the asm-issued LDS-DMA statements, the MFMA overloads and the fragment
// read, the cross-lane reductions that are safe next to those DMAs, and the host side of a launch with more than 64 KB of dynamic
// LDS (lds_attr.h, which the GEMM family shares).  The rules below have this one home; a kernel of the family takes them from here instead of copying them.
// (The two-pass LayerNorm statistics on the operand registers stay written out in ff_block.hip and temporal_block_rr.hip:
// as a function here, hipcc orders the operands of their ~160 additions the other way round.  Same sums, other code.)
#pragma once
#include "fyc_common.h"
#include "lds_attr.h"      // rp::LdsAttr: the dynamic-LDS attribute, once per device

namespace rp {

constexpr int PIECE = 1024;                    // one MFMA operand for all 64 lanes (16 B / lane): the unit of the packed weight streams

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- device: global -> LDS DMA from inline asm -----------------------------------------------------------------------------------
// NOT the builtin: while a builtin LDS-DMA is outstanding hipcc turns every counted lgkmcnt wait of the fragment reads into
// lgkmcnt(0) (it models the DMA as a FLAT access that may touch LDS), so each k-step paid the full LDS round trip.  The compiler
// does not count these loads: the barriers of these kernels carry their own s_waitcnt vmcnt.  M0 is saved and restored inside
// every statement: it is compiler-reserved, and an "m0" clobber is only a warning, so a statement must leave it as it found it
// (tests/test_build_checks.py checks that on the generated code).  The s_nop 0 is the wait state between the M0 write and its use.

// 1 KiB (one piece): wave-uniform base + 32-bit lane offset
__device__ __forceinline__ void dma16(const char* gbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(gbase), "s"(lds_dst) : "memory");
}
// Four consecutive pieces (4 KiB of the stream -> 4 KiB of the ring) by one wave: ONE M0 write, the instruction's immediate
// offset moves the global and the LDS address together.
__device__ __forceinline__ void dma16x4(const char* gbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, %2\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(gbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void dma16v(const void* gsrc, unsigned lds_dst) {                        // one piece, per-lane source address
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void dma_landed_barrier() {       // all of this wave's DMA pieces have landed, then the workgroup meets
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// ---- device: matrix instructions and the fragment read ---------------------------------------------------------------------------
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
// piece `piece` of the stage at sl (= stage base + lane * 16): the lane-linear image is a conflict-free ds_read_b128
template <typename Frag> __device__ __forceinline__ Frag frag(const char* sl, int piece) { return *reinterpret_cast<const Frag*>(sl + piece * PIECE); }

// ---- device: cross-lane reductions next to asm-issued DMAs -------------------------------------------------------------------------
// gfx950's v_permlane32_swap / v_permlane16_swap, plain VALU.  NOT __shfl_xor: that is ds_bpermute_b32, an LDS-queue instruction,
// and hipcc (which cannot see the asm DMAs above) waits for it with a COUNTED lgkmcnt between the fragment reads of the stages it
// sinks this code into - with LDS-DMA writes in flight the result was consumed early in ~12 % of the row blocks of ff_block.hip
// (row statistics off by ~1e-3: tools/ff_stress.py found the kernel's output changing from launch to launch;
// profiles/r03_ff_block_race.txt).  No LDS-queue instruction other than fragment reads
// and staging writes may sit between asm-issued DMAs.
__device__ __forceinline__ float halves_sum(float v) { return swap32_sum(v); }             // over the two lane halves of a wave, every lane gets it (fyc_common.h: the two results of the swap must stay opaque to hipcc)
__device__ __forceinline__ float rows_sum(float v) { return swap32_sum(swap16_sum(v)); }   // over the four 16-lane rows of a wave (fyc_common.h: opaque swap results, as for the maxima)
__device__ __forceinline__ float rows_max(float v) { return swap32_max(swap16_max(v)); }   // (fyc_common.h: the plain fmaxf form is miscompiled)

// ---- host ------------------------------------------------------------------------------------------------------------------------
// Does a kernel that needs `bytes` of LDS fit this process's device (one GPU per process)?  The LDS per CU is queried once per
// process; when no device answered (0) the answer is yes and the launch reports what is wrong.  A device / partition mode with
// less LDS makes the *_supported entry points say no, and the caller keeps the unfused schedule.
inline bool lds_fits(int64_t bytes) {
  static const int64_t cap = [] {
    int64_t caps[8];
    return fyc_device_caps(caps) == 0 ? caps[1] : (int64_t)0;
  }();
  return !(cap > 0 && cap < bytes);
}

// every pointer is 16-byte aligned (null counts as aligned: optional operands)
template <typename... P>
inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...); }

}  // namespace rp
