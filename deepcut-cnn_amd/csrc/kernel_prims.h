// kernel_prims.h — the device primitives every kernel source shares (conv_gemm.h, wino_f32.hip, wino_f16.hip, stream1x1.hip, stream1x1_f32.hip,
// stem_f16.hip): vector types, buffer descriptors, the magic-number division, and the inline-asm memory, wait, barrier and lane
// primitives.  Each exists once here: a fix to one of them (wait states in front of an inline-asm request, say) is one edit.
#pragma once
#include <hip/hip_runtime.h>

namespace dc {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// Buffer addressing (V# descriptors): address = base + voffset(VGPR) + soffset(SGPR); an access whose
// voffset is >= num_records returns 0 / is dropped.  This keeps the K loop almost free of VALU work —
// which matters because on gfx950 the fp32 MFMA shares the SIMD's fp32 datapath: every VALU
// instruction issued between MFMAs is paid IN ADDITION to them (tools/probes/mfma_probe.hip:
// 143 TF/s bare, 91 TF/s with 8 VALU per MFMA, one or two waves per SIMD alike).
//   * per-thread voffsets are loop invariant, the per-tile displacement (tap, channel block) is uniform
//     and travels in soffset (SALU);
//   * zero padding = out-of-range voffset (one v_cndmask per load from a precomputed tap-validity mask).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dc_rsrc(const void* p, unsigned bytes = 0x7fffffff) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
template <typename V = f32x4>
__device__ __forceinline__ V dc_bload4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
constexpr unsigned kOOB = 0x80000000u;  // > any tensor size: hardware returns 0
// n / d for 0 <= n < 2^31 with host-computed magic {mul, shift} (dc_magic, kernels.h): 2 VALU instead of the ~25 of a runtime division
__device__ __forceinline__ int dc_fastdiv(int n, const unsigned (&mg)[2]) {
  return (mg[1] >> 31) ? n : (int)(__umulhi((unsigned)n, mg[0]) >> (mg[1] & 31));  // bit 31 of the shift word: d == 1
}

// LDS-DMA (`buffer_load_dwordx4 ... lds`): 64 lanes x 16 bytes travel from global memory straight into LDS, no VGPRs and
// no ds_write.  The LDS destination is M0 + 16*lane (lane-linear, 1 KiB per wave instruction); the SOURCE address is per
// lane (V# base + voffset + soffset), so a swizzled LDS image is made by permuting which 16-byte chunk each lane
// fetches.  An out-of-range voffset stores zeros (the zero padding of the gather keeps working unchanged).
// Written as inline asm on purpose: through the builtin the compiler knows that LDS is written behind its back and
// makes every later ds_read wait for vmcnt(0) — the pipelines keep 1-2 tiles in flight across their barriers and
// count vmcnt themselves.  (M0 is written in the same statement that reads it; the compiler does not use M0 on these paths.)
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ i32x4 dc_rsrc_words(const void* p) {
  const unsigned long long a = (unsigned long long)p;
  return i32x4{(int)(unsigned)a, (int)((a >> 32) & 0xffffu), 0x7fffffff, 0x00020000};
}
// The descriptor of what lies behind byte `off` of a view: the base moved by off (wave uniform, sign extended: SALU), `bytes` records.
// This is how a uniform, step-dependent displacement comes UNDER the range check with a loop-invariant voffset and no VALU work: for a
// raw buffer (stride 0, not swizzled) the check compares inst_offset + voffset with num_records; soffset is added to the address but
// takes no part in the check ("sgpr_offset is not a part of the offset term", buffer addressing / range checking in the CDNA3 ISA
// guide), so a displacement in soffset would leave the end of the operand unguarded.  bytes = 0: every access is dropped.
__device__ __forceinline__ i32x4 dc_rsrc_behind(i32x4 base, int off, int bytes) {
  const unsigned long long a = (((unsigned long long)(unsigned)base[1] << 32) | (unsigned)base[0]) + (unsigned long long)(long long)off;
  return i32x4{(int)(unsigned)a, (int)(unsigned)(a >> 32), bytes, base[3]};
}
// voff on the lanes whose bit is set in a wave-uniform mask, an out-of-range offset on the others: ONE VALU instruction, the mask is
// SALU work (plain asm: a pure function of its inputs)
__device__ __forceinline__ unsigned dc_lanes_or_oob(unsigned long long mask, unsigned voff) {
  unsigned v;
  asm("v_cndmask_b32_e64 %0, -1, %1, %2" : "=v"(v) : "v"(voff), "s"(mask));
  return v;
}
// (wave-uniform values that the compiler keeps in vector registers — it does behind the wave-uniform branches of a step loop — come back
//  to scalar ones here: an "s" operand is not converted by the compiler, the assembler rejects the instruction)
__device__ __forceinline__ unsigned dc_uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ i32x4 dc_uni4(i32x4 r) {
  return i32x4{__builtin_amdgcn_readfirstlane(r[0]), __builtin_amdgcn_readfirstlane(r[1]), __builtin_amdgcn_readfirstlane(r[2]), __builtin_amdgcn_readfirstlane(r[3])};
}
__device__ __forceinline__ void dc_dma16(i32x4 rs, unsigned lds, unsigned voff, unsigned soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds), "v"(voff), "s"(rs), "s"(soff)
               : "memory", "m0");
}
// the same with soffset 0 (an immediate: no SGPR holds it) and the LDS address made scalar here (dc_uni)
__device__ __forceinline__ void dc_dma16(i32x4 rs, unsigned lds_, unsigned voff) {
  const unsigned lds = dc_uni(lds_);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds), "v"(voff), "s"(rs) : "memory", "m0");
}
// ... and the descriptor made scalar here as well (dc_uni4: a descriptor the compiler may hold in vector registers).  A form of its
// own, like dc_store16_untracked_uni: dc_uni4 written around the caller's argument runs before the other operands are computed and
// schedules the step loop of stream1x1.hip differently
__device__ __forceinline__ void dc_dma16_uni(i32x4 rs, unsigned lds, unsigned voff) { dc_dma16(dc_uni4(rs), lds, voff); }
// a 4-byte buffer load the compiler does not track (no s_waitcnt of its own): the caller's counted vmcnt covers it
__device__ __forceinline__ float dc_load_f32_untracked(i32x4 rs, unsigned voff) {
  float v;
  // s_nop: the hazard recogniser does not look inside inline asm, and "VALU writes SGPR -> VMEM reads that SGPR" needs 5
  // wait states (a descriptor restored from an SGPR spill by v_readlane right in front of this statement read stale
  // registers in the round-3 walking-tile experiment: wild addresses).  tools/check_asm_hazards.py scans for the pattern.
  asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, 0 offen" : "=v"(v) : "v"(voff), "s"(rs) : "memory");
  return v;
}
// a 16-byte buffer store the compiler does not track (no s_waitcnt of its own): the caller's counted vmcnt covers it
// (the s_nop behind it: a store of more than 8 bytes reads its data registers over several cycles, and the hazard recogniser, which does not
//  look inside inline asm, let a v_or overwrite the first of them in the next cycle — one wrong dword per vector on some lanes)
__device__ __forceinline__ void dc_store16_untracked(i32x4 rs, unsigned voff, u32x4 v) {
  asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rs) : "memory");
}
__device__ __forceinline__ void dc_store16_untracked_uni(i32x4 rs, unsigned voff, u32x4 v) { dc_store16_untracked(dc_uni4(rs), voff, v); }
template <int N>
__device__ __forceinline__ void dc_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// own LDS traffic retired, then the workgroup barrier (a raw s_barrier: __syncthreads() would drain vmcnt too)
__device__ __forceinline__ void dc_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// lanes 32..63 of lo[e] <-> lanes 0..31 of hi[e], e = 0..3 (inline asm: this compiler's builtin returns the first result
// twice; one s_nop for the four: the VALU instructions that produced the operands need two wait states before a permlane)
__device__ __forceinline__ void dc_permlane32_swap4(float (&lo)[4], float (&hi)[4]) {
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %4\n\tv_permlane32_swap_b32 %1, %5\n\tv_permlane32_swap_b32 %2, %6\n\tv_permlane32_swap_b32 %3, %7"
      : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]));
}
// the same for e = 0..1
__device__ __forceinline__ void dc_permlane32_swap2(unsigned (&lo)[2], unsigned (&hi)[2]) {
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3" : "+v"(lo[0]), "+v"(lo[1]), "+v"(hi[0]), "+v"(hi[1]));
}
// float32 + the low / high half of a packed float16 pair, exactly rounded once (v_fma_mix_f32 h * 1.0 + f): the conversion folded into
// the add.  Plain (non-volatile) asm: pure functions of their inputs.
__device__ __forceinline__ float dc_add_half_lo(unsigned h2, float f) {
  float d;
  asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(h2), "v"(f));
  return d;
}
__device__ __forceinline__ float dc_add_half_hi(unsigned h2, float f) {
  float d;
  asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(h2), "v"(f));
  return d;
}

}  // namespace dc
