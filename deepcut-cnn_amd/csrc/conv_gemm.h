// conv_gemm.h — the gather-GEMM kernel of the DeeperCut forward path (device code only; conv_gemm_f32.hip, conv_gemm_f16.hip and
// conv_gemm_bf16.hip instantiate it for one element type each, conv_gemm.cpp launches it).
//
// conv_gemm_kernel is the hot kernel: an im2col-free gather-GEMM over channels-last (NHWC)
// activations using the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32, LDS-staged
// activation / filter tiles (double buffered, padded rows -> conflict-free ds_read_b128 operand
// fetches), and a fused epilogue (folded BatchNorm+Scale / bias, residual add, ReLU, sigmoid).
// It replaces, for this path, im2col_gpu + caffe_gpu_gemm (+ col2im_gpu for the deconvolution
// heads) and the per-layer BatchNorm/Scale/ReLU/Eltwise/Crop/Sigmoid kernels of the reference
// (src/caffe/layers/*.cu, src/caffe/util/im2col.cu, math_functions.cu) — see DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernel_prims.h"
#include "kernels.h"

namespace dc {

// ------------------------------------------------------------------------------------------------
// gather-GEMM convolution
// ------------------------------------------------------------------------------------------------

// Kernel arguments are fetched lazily, cache line by cache line, wherever the compiler first needs a field: the gather-GEMM
// touched four lines of its 632-byte block at four different points of its prologue, each first touch a scalar-cache miss
// on the critical path.  DC_KARG_TOUCH requests one dword of each of the first five lines (every field but the multi-class table) at kernel entry (results unused), so
// that the lines arrive together; DC_KARG_HOLD keeps the five scratch SGPRs reserved until a point that the compiler can
// only reach after an `s_waitcnt lgkmcnt(0)` of its own (scalar loads return out of order: a register freed earlier could
// be overwritten by the late dummy load).
#define DC_KARG_TOUCH(n0, n1, n2, n3, n4)                                                                                  \
  unsigned n0, n1, n2, n3, n4;                                                                                             \
  {                                                                                                                        \
    const auto* ka_ = __builtin_amdgcn_kernarg_segment_ptr();                                                              \
    asm volatile("s_load_dword %0, %5, 0x0\n\ts_load_dword %1, %5, 0x40\n\ts_load_dword %2, %5, 0x80\n\ts_load_dword %3, %5, 0xc0\n\t" \
                 "s_load_dword %4, %5, 0x100"                                                                              \
                 : "=&s"(n0), "=&s"(n1), "=&s"(n2), "=&s"(n3), "=&s"(n4)                                                     \
                 : "s"(ka_));                                                                                              \
  }
#define DC_KARG_HOLD(n0, n1, n2, n3, n4) asm volatile("" ::"s"(n0), "s"(n1), "s"(n2), "s"(n3), "s"(n4))
static_assert(sizeof(ConvGemmParams) >= 0x140, "DC_KARG_TOUCH reads five 64-byte lines of the argument block");

// element-type traits of the gather-GEMM: activations / filters are float or _Float16 in HBM and LDS,
// accumulation, the epilogue arithmetic and its constants are always float
template <typename T>
struct Elem;
template <>
struct Elem<float> {
  static constexpr int SPC = 4;  // MFMA steps per 32-byte operand chunk: 4 x v_mfma_f32_32x32x2_f32 (k = 8)
  typedef unsigned raw_t;  // a loaded element before conversion (conversion = first use: the load stays in flight until then)
  static __device__ __forceinline__ raw_t load_raw(__amdgpu_buffer_rsrc_t r, unsigned off) { return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0); }
  static __device__ __forceinline__ float cvt(raw_t v) { return __builtin_bit_cast(float, v); }
  static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
  }
  static __device__ __forceinline__ void store(float v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, 0);
  }
};
template <>
struct Elem<_Float16> {
  static constexpr int SPC = 1;  // 1 x v_mfma_f32_32x32x16_f16 (k = 16) per 32-byte chunk
  typedef unsigned short raw_t;
  static __device__ __forceinline__ raw_t load_raw(__amdgpu_buffer_rsrc_t r, unsigned off) { return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0); }
  static __device__ __forceinline__ float cvt(raw_t v) { return (float)__builtin_bit_cast(_Float16, v); }
  static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return (float)__builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0));
  }
  static __device__ __forceinline__ void store(float v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (_Float16)v), r, off, 0, 0);
  }
};
// bfloat16: float32's exponent range with 8 significant bits.  Widening is a 16-bit shift; a store rounds once, to nearest even
// (v_cvt_pk_bf16_f32; NaN stays NaN)
template <>
struct Elem<__bf16> {
  static constexpr int SPC = 1;  // 1 x v_mfma_f32_32x32x16_bf16 (k = 16) per 32-byte chunk
  typedef unsigned short raw_t;
  static __device__ __forceinline__ raw_t load_raw(__amdgpu_buffer_rsrc_t r, unsigned off) { return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0); }
  static __device__ __forceinline__ float cvt(raw_t v) { return __builtin_bit_cast(float, (unsigned)v << 16); }
  static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t r, unsigned off) { return cvt(load_raw(r, off)); }
  static __device__ __forceinline__ void store(float v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (__bf16)v), r, off, 0, 0);
  }
};
// the 16-bit matrix step of either 16-bit type: 32x32 output fragment += 32x16 (a) x 16x32 (b), float32 accumulation
template <typename T>
__device__ __forceinline__ f32x16 dc_mfma16(f32x4 a, f32x4 b, f32x16 c) {
  if constexpr (std::is_same_v<T, __bf16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// MC: multi-class launch (ConvGemmParams::ncls > 1): the class-dependent scalars come from p.cls[class of this block].
// DMA: 0 = operands staged through a register ring (PF tiles) and ds_write_b128 into two padded LDS stages;
//      D >= 2 = operands fetched by LDS-DMA into a ring of D unpadded, XOR-swizzled LDS stages (tile rows of 128 bytes),
//      D - 1 tiles requested ahead, one raw barrier per tile, vmcnt counted by hand (PF unused).
// SWP: the MFMA operands are swapped (filters as the row operand), so that a lane's accumulators are 16 CHANNELS of one
//      pixel (4 runs of 4 consecutive channels) instead of 16 pixels of one channel: the epilogue then forms 16-byte output
//      vectors in registers (float16: one v_permlane32_swap per register pair) — no LDS transposition, no barriers.
// MP: multi-problem launch (ConvGemmParams::nprob > 0): every per-tensor scalar AND pointer comes from the device-resident
//     table p.multi->prob[problem of this block] — the same layer over the scales of a pyramid / the classes of a deconvolution.
template <typename T, int BM, int BN, int BK, int WR, int WC, int WK, int PF, bool MC = false, int DMA = 0, bool SWP = false, bool MP = false>
// (second launch bound = waves per SIMD the register budget must allow: the 4-wave LDS-DMA tiles are meant to run two
//  workgroups per CU, so their allocation has to stay within 256 registers — with it the compiler also keeps the
//  accumulators in VGPRs instead of AGPRs: no v_accvgpr_read pass in front of the epilogue, 169 instead of 200 registers)
__global__ __launch_bounds__(WR* WC* WK * 64, (DMA && WR * WC * WK == 4) ? 2 : 1) void conv_gemm_kernel(const std::conditional_t<MP, ConvMultiArgs, ConvGemmParams> ka) {
  const ConvGemmParams& p = [&]() -> const ConvGemmParams& {
    if constexpr (MP) return ka.p;
    else return ka;
  }();
  const long long t_entry = (long long)__builtin_amdgcn_s_memrealtime();  // before the first kernel-argument load (DC_DEBUG_TIMING)
  DC_KARG_TOUCH(ka0, ka1, ka2, ka3, ka4);
  constexpr int ES = sizeof(T);          // bytes per element
  constexpr int VEC = 16 / ES;           // elements per 16-byte vector
  constexpr int SPC = Elem<T>::SPC;
  constexpr int NW = WR * WC * WK;       // waves per workgroup (4 or 8)
  constexpr int NT = NW * 64;
  static_assert(NW == 4 || NW == 8 || (NW == 16 && DMA), "4 or 8 waves per workgroup (16 compiles for the LDS-DMA tiles: measured, no gain — EXPERIMENTS.md A)");
  constexpr int LDB = DMA ? BK * ES : BK * ES + 16;  // LDS row, bytes: padded (16-B aligned, bank-spread), or 128 swizzled (DMA)
  static_assert(!DMA || BK * ES == 128 || BK * ES == 256, "the LDS-DMA image has 128- or 256-byte rows (8 / 16 chunks of 16 bytes, XOR-swizzled)");
  static_assert(DMA == 0 || (DMA >= 2 && DMA <= 4), "ring of 2..4 LDS stages");
  constexpr int NSTG = DMA ? DMA : 2;
#ifndef DC_PRO_FULL
#define DC_PRO_FULL 1
#endif
  // LDS-DMA: the prologue requests the first DMA-1 tiles (all their filter pieces before the row decode, their activation pieces
  // after it) and then — LATE — the whole of tile DMA-1, which the steady state (tile `it` requests tile it+DMA-1) would only ask for
  // during tile 0: a first-tile latency earlier, without putting another tile's filter pieces in front of tile 0's activations
  // (requested with the first filter pieces instead, it cost the float32 batch-1 forward 1.4 %).
  // float16 only: the float32 batch-1 launches are one round of workgroups that all start together, and a deeper initial burst
  // delays their first tile more than the earlier tile DMA-1 gives back (one forward at a time 335.8 -> 331.5 images/s).
  constexpr bool LATE = DMA && DC_PRO_FULL && ES == 2;
  constexpr int TM = BM / WR, TN = BN / WC;
  constexpr int FM = TM / 32, FN = TN / 32;
  static_assert(FM >= 1 && FN >= 1 && TM % 32 == 0 && TN % 32 == 0, "wave tile = multiples of 32x32");
  constexpr int C4 = BK / VEC;           // 16-byte vectors per tile row
  constexpr int RPP = NT / C4;           // tile rows covered by one pass of the workgroup's threads
  constexpr int NA = BM / RPP, NBV = BN / RPP;
  static_assert(NA >= 1 && NBV >= 1, "tile too small for the loader");
  constexpr int KCH = BK * ES / 32;      // 32-byte operand chunks per tile row
  static_assert(KCH % WK == 0, "k chunks must split evenly over WK");
  constexpr int NCH = KCH / WK;          // chunks this wave owns per tile
  static_assert(NCH >= 2 && NCH % 2 == 0, "the software pipeline needs an even number (>=2) of chunks per wave");
  constexpr int NST = NCH * SPC;         // MFMA steps per tile per wave
  static_assert(DMA || NST >= 4, "the register-ring pipeline places its work in 4 distinct MFMA steps");
  constexpr int GBAR = SPC > 1 ? NST - 3 : NST - 1;  // step before which the tile's barrier is taken
  constexpr int TILEB = (BM + BN) * LDB;  // bytes per LDS stage
  constexpr int RPW = 16 / WK;           // accumulator registers each split-K wave finalises
  constexpr int WPS = BN + 4;                       // wide-epilogue staging row pitch (floats)
  // DMA: the buffer is sized for the ring, the split-K exchange and the wide epilogue's staging, whichever is largest
  constexpr int EPIB = ES == 2 && !SWP ? BM * WPS * 4 : 0;
  constexpr int SPKB = (WK - 1) * BM * BN * 4;
  constexpr int MAINB = DMA ? (NSTG * TILEB > EPIB ? (NSTG * TILEB > SPKB ? NSTG * TILEB : SPKB) : (EPIB > SPKB ? EPIB : SPKB)) : 2 * TILEB;
  static_assert(SPKB <= MAINB, "split-K partials must fit in the tile buffers");
  constexpr bool EARLY_RESID = !SWP && FM * FN * RPW <= 16;  // shortcut tile prefetched before the K loop
  // Wide epilogue (float16): the C fragment gives a lane ONE channel of 16 different pixels, i.e. 2-byte accesses — 128 vector
  // memory instructions per lane for a 64x64 wave tile with a shortcut, and the CU's address unit, not HBM, bounds the
  // bandwidth-bound layers (K <= 512).  Instead the finished tile (fp32, after the affine) is transposed through the tile
  // buffers in LDS and every thread adds the shortcut to, and stores, 8 consecutive channels of one pixel: 16-byte accesses,
  // 8x fewer instructions; the shortcut vectors are requested before the transposition so that they are in flight meanwhile.
  constexpr int WVEC = BM * (BN / 8) / NT;           // 16-byte output vectors per thread
  constexpr bool WIDE_OK = !SWP && ES == 2 && BM * WPS * 4 <= MAINB && (BM * (BN / 8)) % NT == 0 && WVEC <= 16;

  static_assert(!SWP || (DMA && (16 / WK) % 4 == 0), "SWP: LDS-DMA kernels, every split-K wave finalises whole 4-channel runs");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[MAINB + 4 * BM + (SWP ? 8 * BN : 0)];
  int* rowinfo = reinterpret_cast<int*>(smem + MAINB);
  float* epi_sc = reinterpret_cast<float*>(smem + MAINB + 4 * BM);  // SWP: scale[BN], shift[BN] of the tile's channels
  // per tile row: byte offset of its output pixel, or -1
  static_assert(!(MC && MP), "a multi-problem launch carries its deconvolution classes as problems");

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wk = wave % WK;
  const int wc = (wave / WK) % WC;
  const int wr = wave / (WK * WC);

  // Tile <- block map.  Blocks are observed to land on XCD (blockIdx % 8), each XCD with its own 4 MB L2.
  // The default n-fastest order makes every XCD touch every filter row AND every pixel row; instead the
  // tile grid is cut into 8 rectangles (gx x gy chosen on the host to minimise filters*gy + pixels*gx)
  // and XCD q walks rectangle q, so an L2 only fetches its rectangle's share of both operands.
  // Correctness does not depend on the placement (it is only a locality hint).
  // class-dependent scalars (uniform: SGPRs).  Single-problem launches read them from the parameter block itself.
  int c_Ktot = p.Ktot, c_nty = p.nty, c_ntx = p.ntx, c_dy0 = p.dy0, c_ddy = p.ddy, c_x0 = p.x0, c_ddx = p.ddx, c_xbias = p.x_bias;
  int c_OH = p.OH, c_OW = p.OW, c_M = p.M;
  unsigned c_dohw[2] = {p.div_ohw[0], p.div_ohw[1]}, c_dow[2] = {p.div_ow[0], p.div_ow[1]};
  long c_woff = 0, c_yoff = 0;
  // per-tensor scalars (uniform): the argument block's in a single-problem launch, the problem's in a multi-problem one
  const T* px = reinterpret_cast<const T*>(p.x);
  long c_ximg = p.x_img_stride, c_yimg = p.y_img_stride;
  int c_xrow = p.x_row_stride, c_xrows = p.x_rows, c_xrowlen = p.x_rowlen, c_yrow = p.y_row_stride, c_ypix = p.y_pix_stride;
  void* c_y = p.y;
  const void* c_resid = p.resid;
  int c_densex = p.dense_x, c_densey = p.dense_y;
  int tile_n, tile_m;
  if constexpr (MP) {
    // XCD (qx, qy) owns the n tiles [tn*qx/gx, tn*(qx+1)/gx) and walks, problem after problem, the m tiles
    // [tm_k*qy/gy, tm_k*(qy+1)/gy) of every problem k, n fastest: the layer's filters (shared by all problems) are fetched
    // once per L2 that needs them.  The grid is 8 x the longest XCD list; surplus workgroups exit.
    const ConvMultiTable* tb = &ka.t;  // in the argument block: scalar loads
    const int xq = blockIdx.x & 7, lgx = p.mc_lgx, lgy = 3 - lgx;
    const int qx = xq & ((1 << lgx) - 1), qy = xq >> lgx;
    const int n_lo = (p.tiles_n * qx) >> lgx, n_cnt = ((p.tiles_n * (qx + 1)) >> lgx) - n_lo;
    const int slot = blockIdx.x >> 3;
    const int mrow = n_cnt == (p.tiles_n >> lgx) ? dc_fastdiv(slot, p.div_rw[0]) : dc_fastdiv(slot, p.div_rw[1]);  // slot / n_cnt
    int k = 0, start = 0;
#pragma unroll
    for (int j = 0; j < kMaxProblems; ++j) {
      const int e = tb->end[qy][j];
      const int ge = (e - 1 - mrow) >> 31;  // -1 iff mrow >= e (sign arithmetic: stays on the scalar unit; e <= INT_MAX, mrow >= 0)
      k -= ge;
      start = (e & ge) | (start & ~ge);
    }
    if (k >= p.nprob) return;
    const ConvProblem& q = tb->prob[k];
    c_Ktot = q.Ktot, c_nty = q.nty, c_ntx = q.ntx, c_dy0 = q.dy0, c_ddy = q.ddy, c_x0 = q.x0, c_ddx = q.ddx, c_xbias = q.x_bias;
    c_OH = q.OH, c_OW = q.OW, c_M = q.M;
    c_dohw[0] = q.div_ohw[0], c_dohw[1] = q.div_ohw[1], c_dow[0] = q.div_ow[0], c_dow[1] = q.div_ow[1];
    c_woff = q.w_off;
    px = reinterpret_cast<const T*>(q.x);
    c_ximg = q.x_img_stride, c_yimg = q.y_img_stride;
    c_xrow = q.x_row_stride, c_xrows = q.x_rows, c_xrowlen = q.x_rowlen, c_yrow = q.y_row_stride, c_ypix = q.y_pix_stride;
    c_y = q.y;
    c_resid = q.resid;
    c_densex = q.dense_x, c_densey = q.dense_y;
    tile_m = ((q.tiles_m * qy) >> lgy) + (mrow - start);
    tile_n = n_lo + (slot - mrow * n_cnt);
  } else if constexpr (MC) {
    // Workgroup b runs on XCD (b % 8), each with its own L2.  XCD (qx, qy) of a gx x gy arrangement owns the n tiles
    // [tn*qx/gx, tn*(qx+1)/gx) and, of EVERY class, the m tiles [tm*qy/gy, tm*(qy+1)/gy); it walks its classes heaviest
    // first.  So an L2 fetches 1/gx of the filter images and 1/gy of the pixels instead of everything (the heads'
    // filters alone are 30 MB against 4 MB of L2).  The grid is 8 x the longest XCD list; surplus workgroups exit.
    const int xq = blockIdx.x & 7, lgx = p.mc_lgx, lgy = 3 - lgx;
    const int qx = xq & ((1 << lgx) - 1), qy = xq >> lgx;
    const int n_lo = (p.tiles_n * qx) >> lgx, n_cnt = ((p.tiles_n * (qx + 1)) >> lgx) - n_lo;
    int slot = blockIdx.x >> 3, c = -1, m_lo = 0;
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k)
      if (k < p.ncls && c < 0) {
        const int lo = (p.cls[k].tiles_m * qy) >> lgy;
        const int cnt = (((p.cls[k].tiles_m * (qy + 1)) >> lgy) - lo) * n_cnt;
        if (slot < cnt) c = k, m_lo = lo;
        else slot -= cnt;
      }
    if (c < 0) return;
    const ConvClass& q = p.cls[c];
    c_Ktot = q.Ktot, c_nty = q.nty, c_ntx = q.ntx, c_dy0 = q.dy0, c_ddy = q.ddy, c_x0 = q.x0, c_ddx = q.ddx, c_xbias = q.x_bias;
    c_OH = q.OH, c_OW = q.OW, c_M = q.M;
    c_dohw[0] = q.div_ohw[0], c_dohw[1] = q.div_ohw[1], c_dow[0] = q.div_ow[0], c_dow[1] = q.div_ow[1];
    c_woff = q.w_off, c_yoff = q.y_off;
    const int sr = slot / n_cnt;  // uniform
    tile_m = m_lo + sr;
    tile_n = n_lo + (slot - sr * n_cnt);
  } else if (p.xcd_on) {
    const int q = blockIdx.x & 7, slot = blockIdx.x >> 3;  // XCD, position inside its rectangle
    const int lgx = p.xcd_lgx, lgy = 3 - lgx, qx = q & ((1 << lgx) - 1), qy = q >> lgx;
    const int n_lo = (p.tiles_n * qx) >> lgx, rw = ((p.tiles_n * (qx + 1)) >> lgx) - n_lo;
    const int m_lo = (p.tiles_m * qy) >> lgy, rh = ((p.tiles_m * (qy + 1)) >> lgy) - m_lo;
    if (slot >= rw * rh) return;  // grid is padded to 8 x the largest rectangle
    const int sr = rw == (p.tiles_n >> lgx) ? dc_fastdiv(slot, p.div_rw[0]) : dc_fastdiv(slot, p.div_rw[1]);  // slot / rw, all scalar
    tile_n = n_lo + (slot - sr * rw);
    tile_m = m_lo + sr;
  } else {
    tile_m = dc_fastdiv(blockIdx.x, p.div_tn);
    tile_n = blockIdx.x - tile_m * p.tiles_n;
  }
  const int m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  const int T_ = c_Ktot / BK;
  DC_KARG_HOLD(ka0, ka1, ka2, ka3, ka4);  // the tile map above needed kernel arguments: the dummy loads have landed
  auto stamp = [&](int slot) {
    if (p.dbg && lane == 0) {
      long long* d = p.dbg + ((long)blockIdx.x * NW + wave) * 12;
      d[slot] = (long long)__builtin_readcyclecounter();
      if (slot == 0) d[8] = t_entry, d[10] = (long long)__builtin_amdgcn_s_memrealtime();  // 100 MHz, the same clock on every CU
      if (slot == 7) d[9] = (long long)__builtin_amdgcn_s_memrealtime();
    }
  };
  stamp(0);

  // ---- prologue, ordered so that every exposed memory round trip overlaps another -------------------
  // (1) filter rows need no pixel decode: their first PF tiles go out immediately
  const int lrow = t / C4;
  // byte column of this thread's 16-byte vector.  DMA: lane l of a wave lands at LDS byte 16*l of its 1 KiB piece (8 rows of
  // 128 bytes: row l/8, position l%8 — or 4 rows of 256 bytes), and position p of row r holds source chunk p ^ swz(r),
  // swz(r) = (r >> 1) & 7 for 128-byte rows, r & 15 for 256-byte rows: the 16 lanes a ds_read_b128 serves together (rows
  // {0-3,12-15,20-27} / {4-11,16-19,28-31} of a fragment, same chunk) then hit 16 different 16-byte bank groups, without padding.
  constexpr bool ROW256 = BK * ES == 256;
  const int lcb = DMA ? ((t % C4) ^ (ROW256 ? (lrow & 15) : ((lrow >> 1) & 7))) * 16 : (t % C4) * 16;
  const int lce = lcb / ES;       // same, in elements
  static_assert(!DMA || (C4 == (ROW256 ? 16 : 8) && RPP % (ROW256 ? 16 : 32) == 0), "DMA loader: the swizzle of a row must not depend on the piece set");
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned ldsw = lds0 + (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;  // this wave's piece of every 8*NW-row set
  unsigned bvoff[NBV];
#pragma unroll
  for (int j = 0; j < NBV; ++j) {
    const int n = n0 + lrow + RPP * j;
    bvoff[j] = n < p.Cout ? (unsigned)(n * c_Ktot + lce) * ES : kOOB;  // rows past Cout read as zeros
  }
  const __amdgpu_buffer_rsrc_t wr_ = dc_rsrc(reinterpret_cast<const T*>(p.w) + c_woff, 0x7fffffffu);
  const i32x4 wrs = dc_rsrc_words(reinterpret_cast<const T*>(p.w) + c_woff);
  f32x4 ra[DMA ? 1 : PF][DMA ? 1 : NA], rb[DMA ? 1 : PF][DMA ? 1 : NBV];  // 16-byte containers (4 floats or 8 halves)
  int kg = 0;
  auto gload_b = [&](int slot) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) rb[slot][j] = dc_bload4(wr_, bvoff[j], (unsigned)kg * ES);
    kg += BK;
  };
  // DMA: the filter rows of one K tile into LDS stage `stg` (piece j = rows j*RPP + 8*wave .. +7 of the B block)
  auto dma_b = [&](int stg) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) dc_dma16(wrs, ldsw + stg * TILEB + BM * LDB + j * RPP * LDB, bvoff[j], (unsigned)kg * ES);  // prologue: stage index
    kg += BK;
  };
  if constexpr (DMA) {
#pragma unroll
    for (int k = 0; k < DMA - 1; ++k)
      if (k < T_) dma_b(k);
  } else {
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (k < T_) gload_b(k);
  }

  // (2) epilogue constants (folded BatchNorm/Scale/bias) also travel now
  float sc[FN], sh[FN];
  float epi_c = 0.f;  // SWP: thread t < BN holds scale[n0 + t], BN <= t < 2*BN holds shift[n0 + t - BN]; to LDS before the first barrier
  if constexpr (SWP) {
    static_assert(2 * BN <= NT, "one epilogue constant per thread");
    const bool is_sh = t >= BN;
    const int co = n0 + (is_sh ? t - BN : t);
    epi_c = is_sh ? 0.f : 1.f;
    const i32x4 scr = dc_rsrc_words(p.scale), shr = dc_rsrc_words(p.shift);  // uniform descriptors (SGPRs)
    if (!is_sh) {
      if (p.scale && co < p.Cout) epi_c = dc_load_f32_untracked(scr, (unsigned)co * 4u);
    } else if (t < 2 * BN) {
      if (p.shift && co < p.Cout) epi_c = dc_load_f32_untracked(shr, (unsigned)co * 4u);
    }
  } else {
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const int co = n0 + wc * TN + b * 32 + (lane & 31);
      const bool cok = co < p.Cout;
      sc[b] = (cok && p.scale) ? p.scale[co] : 1.f;
      sh[b] = (cok && p.shift) ? p.shift[co] : 0.f;
    }
  }

  stamp(1);
  // (3) activation rows: every loading thread decodes ITS rows itself (two magic-number divisions and a handful of
  //     multiply-adds each) and requests their first tiles at once.  An earlier form decoded each row once, in one thread,
  //     and shared it through LDS: that put a barrier and an LDS round trip between the kernel arguments and the first
  //     activation load — ~2 k cycles of every workgroup's life.  Loop-invariant voffset + validity bit per tap (zero padding
  //     = out-of-range voffset); bit (ty*ntx + tx) = source row ty inside the image and source element inside its row (the
  //     thread's element column is added: it matters only for the stem's row taps, which span several pixels).
  unsigned avoff[NA], amask[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + lrow + RPP * i;
    avoff[i] = kOOB;
    amask[i] = 0;
    if (!MC && c_densex) {  // 1x1 over a dense tensor: pixel m starts at element m * sx, its one tap is always inside
      if (m < c_M) avoff[i] = (unsigned)(m * p.sx) * ES + lcb, amask[i] = 1u;
    } else if (m < c_M) {
      const int n = dc_fastdiv(m, c_dohw);
      const int rem = m - n * (c_OH * c_OW);
      const int oy = dc_fastdiv(rem, c_dow);
      const int ox = rem - oy * c_OW;
      avoff[i] = (unsigned)(int)(((long)n * c_ximg + (long)(oy * p.sy) * c_xrow + ox * p.sx) * ES) + lcb;
      unsigned rowmask = 0, colmask = 0, full = 0;
      if (DMA && c_nty == 3 && c_ntx == 3) {
        // the 3x3 layers (a third of the float16 time): the same masks, straight-line — the generic loops below cost ~3 k
        // cycles of every workgroup's prologue (dependent compares + branches, two to four rows per thread)
        const int y0 = oy * p.sy + c_dy0, x0 = ox * p.sx + lce + c_x0;
        const unsigned r0 = (unsigned)y0 < (unsigned)c_xrows, r1 = (unsigned)(y0 + c_ddy) < (unsigned)c_xrows, r2 = (unsigned)(y0 + 2 * c_ddy) < (unsigned)c_xrows;
        const unsigned cm = ((unsigned)x0 < (unsigned)c_xrowlen ? 1u : 0u) | ((unsigned)(x0 + c_ddx) < (unsigned)c_xrowlen ? 2u : 0u) |
                            ((unsigned)(x0 + 2 * c_ddx) < (unsigned)c_xrowlen ? 4u : 0u);
        amask[i] = (r0 ? cm : 0u) | (r1 ? cm << 3 : 0u) | (r2 ? cm << 6 : 0u);
        continue;
      }
#pragma nounroll
      for (int ty = 0; ty < c_nty; ++ty) rowmask |= ((unsigned)(oy * p.sy + c_dy0 + ty * c_ddy) < (unsigned)c_xrows ? 1u : 0u) << ty;
#pragma nounroll
      for (int tx = 0; tx < c_ntx; ++tx) colmask |= ((unsigned)(ox * p.sx + lce + c_x0 + tx * c_ddx) < (unsigned)c_xrowlen ? 1u : 0u) << tx;
#pragma nounroll
      for (int ty = 0; ty < c_nty; ++ty)
        if ((rowmask >> ty) & 1u) full |= colmask << (ty * c_ntx);
      amask[i] = full;
    }
  }
  // the source descriptor starts `x_bias` elements BEFORE the tensor so that every tap displacement is a
  // non-negative soffset; masked lanes never touch memory, valid lanes land inside the tensor
  const __amdgpu_buffer_rsrc_t xr = dc_rsrc(px + c_xbias, 0x7fffffffu);
  const i32x4 xrs = dc_rsrc_words(px + c_xbias);
  // tap cursor, all uniform (SALU): (tx, c0, running bit) and the element displacement of the current tap
  int tx = 0, c0 = 0, tbit = 0;
  int row_soff = c_dy0 * c_xrow + c_x0 - c_xbias;  // displacement of tap (ty, 0)
  int tap_soff = row_soff;
  auto gload_a = [&](int slot) {
    const unsigned soff = (unsigned)(tap_soff + c0) * ES;
    const unsigned bit = 1u << tbit;
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[slot][i] = dc_bload4(xr, (amask[i] & bit) ? avoff[i] : kOOB, soff);
    c0 += BK;
    if (c0 >= p.klen) {
      c0 = 0;
      ++tbit;
      ++tx;
      tap_soff += c_ddx;
      if (tx >= c_ntx) {
        tx = 0;
        row_soff += c_ddy * c_xrow;
        tap_soff = row_soff;
      }
    }
  };
  // DMA: the tap cursor hands out (soffset, validity bit) of the next K tile ...
  unsigned d_soff = 0, d_bit = 0, d_kg = 0;
  auto dma_next = [&]() {
    d_soff = (unsigned)(tap_soff + c0) * ES;
    d_bit = 1u << tbit;
    d_kg = (unsigned)kg * ES;
    kg += BK;
    c0 += BK;
    if (c0 >= p.klen) {
      c0 = 0;
      ++tbit;
      ++tx;
      tap_soff += c_ddx;
      if (tx >= c_ntx) {
        tx = 0;
        row_soff += c_ddy * c_xrow;
        tap_soff = row_soff;
      }
    }
  };
  // ... and piece pc of that tile (0..NA-1: activation rows, NA..NA+NBV-1: filter rows) goes to stage `stg`
  auto dma_piece = [&](unsigned so, int pc) {  // so: byte offset of the stage
    if (pc < NA) {
#ifdef DC_ABL  // diagnostic builds (wrong results, timing only): bit 0 = no in-loop DMA, 1 = no in-loop barrier, 2 = no in-loop
               // fragment reads, 4 = activation pieces of 3 of 9 taps only (the bytes an LDS-resident halo would move)
      if ((DC_ABL & 16) && c_nty == 3 && (d_bit & 0x1b6u)) return;
#endif
      dc_dma16(xrs, ldsw + so + pc * RPP * LDB, (amask[pc < NA ? pc : 0] & d_bit) ? avoff[pc < NA ? pc : 0] : kOOB, d_soff);
    }
    else
      dc_dma16(wrs, ldsw + so + BM * LDB + (pc - NA) * RPP * LDB, bvoff[pc >= NA ? pc - NA : 0], d_kg);
  };
  if constexpr (DMA) {
    // the filter pieces of the first DMA-1 tiles are on their way already (dma_b advanced kg): only the activation pieces here
    const int kg_keep = kg;
#pragma unroll
    for (int k = 0; k < DMA - 1; ++k)
      if (k < T_) {
        dma_next();
#pragma unroll
        for (int i = 0; i < NA; ++i) dma_piece(k * TILEB, i);
      }
    kg = kg_keep;
    if (LATE && T_ >= DMA) {  // tile DMA-1, whole (activation and filter pieces), into the last stage
      dma_next();
#pragma unroll
      for (int pc = 0; pc < NA + NBV; ++pc) dma_piece((DMA - 1) * TILEB, pc);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (k < T_) gload_a(k);
  }
  stamp(2);
  // (4) output byte offset of every tile row, for the epilogue (off the critical path: the loads are in flight)
  if (t < BM) {
    const int m = m0 + t;
    int yo = -1;
    if (!MC && c_densey) {
      if (m < c_M) yo = m * c_ypix * ES;
    } else if (m < c_M) {
      const int n = dc_fastdiv(m, c_dohw);
      const int rem = m - n * (c_OH * c_OW);
      const int oy = dc_fastdiv(rem, c_dow);
      const int ox = rem - oy * c_OW;
      yo = (int)(((long)n * c_yimg + (long)oy * c_yrow + (long)ox * c_ypix) * ES);
    }
    rowinfo[t] = yo;
  }
  stamp(3);
  const __amdgpu_buffer_rsrc_t yr = dc_rsrc(reinterpret_cast<T*>(c_y) + c_yoff, 0x7fffffffu);
  const __amdgpu_buffer_rsrc_t rr = dc_rsrc(reinterpret_cast<const T*>(c_resid ? c_resid : c_y) + c_yoff, 0x7fffffffu);

  f32x16 acc[FM][FN];
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  auto lstore = [&](int buf, int slot) {
    unsigned char* As = smem + buf * TILEB;
    unsigned char* Bs = As + BM * LDB;
#pragma unroll
    for (int i = 0; i < NA; ++i)
      *reinterpret_cast<f32x4*>(As + (lrow + RPP * i) * LDB + lcb) = ra[slot][i];
#pragma unroll
    for (int j = 0; j < NBV; ++j)
      *reinterpret_cast<f32x4*>(Bs + (lrow + RPP * j) * LDB + lcb) = rb[slot][j];
  };
  // MFMA operand fragments, two register sets (chunk parity); lane holds 16 bytes of row (lane&31):
  // fp32: k = 4*(lane>>5) .. +3 of the 8-deep chunk; fp16: k = 8*(lane>>5) .. +7 of the 16-deep chunk
  f32x4 av[2][FM], bv[2][FN];
  // DMA image: 16-byte chunk c of row r sits at position c ^ ((r >> 1) & 7); the wave's q-th operand chunk pair is chunk
  // 2*(q*WK + wk) + (lane >> 5), and since q*WK*32 only touches address bits 5..6 it is applied as an XOR on the offset
  const int frag_k = DMA ? (((2 * wk + (lane >> 5)) ^ (ROW256 ? (lane & 15) : ((lane >> 1) & 7))) * 16) : ((lane >> 5) * 16 + wk * 32);
  const int frag_a = (wr * TM + (lane & 31)) * LDB + frag_k;
  const int frag_b = BM * LDB + (wc * TN + (lane & 31)) * LDB + frag_k;
  auto frag_load = [&](int buf, int q, int set) {
    const unsigned char* As = smem + buf * TILEB + (DMA ? (frag_a ^ (q * WK * 32)) : frag_a + q * WK * 32);
    const unsigned char* Bs = smem + buf * TILEB + (DMA ? (frag_b ^ (q * WK * 32)) : frag_b + q * WK * 32);
#pragma unroll
    for (int a = 0; a < FM; ++a) av[set][a] = *reinterpret_cast<const f32x4*>(As + a * 32 * LDB);
#pragma unroll
    for (int b = 0; b < FN; ++b) bv[set][b] = *reinterpret_cast<const f32x4*>(Bs + b * 32 * LDB);
  };

  // ---- K loop: software pipeline -------------------------------------------------------------------
  // A wave issues in order, and on gfx950 the fp32 MFMA shares the SIMD's fp32 datapath with VALU, so
  // (a) VALU work in the loop is paid on top of the MFMAs -> there is almost none (buffer addressing);
  // (b) anything not interleaved BETWEEN MFMAs in program order stalls the matrix pipe -> the loop's
  //     non-MFMA work is placed into specific MFMA steps of the tile and pinned with sched_barrier.
  // Per tile a wave owns NCH 32-byte chunks = NST MFMA steps (4 per chunk in fp32, 1 in fp16):
  //   first step of chunk q: ds_read the fragments of chunk q+1
  //   step 1: ds_write tile it+1 (ring slot loaded PF iterations ago) into the idle LDS stage
  //   step 2/3: issue the global loads of tile it+1+PF into the ring slot just freed
  //   step GBAR: barrier, then ds_read chunk 0 of tile it+1 from the stage just filled — in fp32 its latency
  //            is covered by the 3 remaining MFMA steps of this tile (all fragment reads of the current
  //            stage are issued before the barrier, so the next tile may overwrite it).
  // Tile k lives in ring slot k % PF: filters are streamed from HBM once per forward (263 MB per image
  // sweep the 256 MB Infinity Cache), so a single tile of lookahead does not cover their latency.
  if constexpr (DMA) {
    // tile 0 has landed when at most the later prologue tiles' activation pieces (requested after it) are outstanding
    // (the early tiles' activation pieces after tile 0's, NA each, and the late tile's NA + NBV)
    const int pt = T_ < DMA - 1 ? T_ : DMA - 1;  // early tiles requested
    if (LATE && T_ >= DMA) {
      if (pt >= 3) dc_wait_vm<2 * NA + NA + NBV>();
      else if (pt == 2) dc_wait_vm<NA + NA + NBV>();
      else dc_wait_vm<NA + NBV>();
    } else {
      if (pt >= 3) dc_wait_vm<2 * NA>();
      else if (pt == 2) dc_wait_vm<NA>();
      else dc_wait_vm<0>();
    }
    if constexpr (SWP) {  // the constants were requested before every DMA piece: the wait above covers them
      if (t < 2 * BN) epi_sc[t] = epi_c;
    }
    dc_lds_barrier();  // every wave's pieces of tile 0 are in LDS; the rows' output offsets (and constants) are visible
  } else {
    lstore(0, 0);
    if (PF < T_) {
      gload_a(0);
      gload_b(0);
    }
    __syncthreads();  // tile 0 staged; the rows' output offsets are visible
  }
  frag_load(0, 0, 0);
  // (5) small wave tiles: the shortcut itself is requested now, before the K loop.
  //     MFMA 32x32 C layout: col = lane&31 (channel), row = (r&3)+8*(r>>2)+4*(lane>>5).
  //     With in-workgroup split-K every one of the WK waves finalises RPW of the 16 accumulator registers.
  float rs[EARLY_RESID ? FM * FN * RPW : 1];
  if (EARLY_RESID && c_resid) {
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
      for (int b = 0; b < FN; ++b)
#pragma unroll
        for (int e = 0; e < RPW; ++e) {
          const int r = wk * RPW + e;
          const int yo = rowinfo[wr * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
          const int co = n0 + wc * TN + b * 32 + (lane & 31);
          const unsigned off = (yo >= 0 && co < p.Cout) ? (unsigned)yo + co * ES : kOOB;
          rs[(a * FN + b) * RPW + e] = Elem<T>::load(rr, off);
        }
  }
  stamp(4);
  // shortcut tile through LDS-DMA (swapped-operand epilogue, float16, one wave per output fragment set, a stage holds the tile)
  constexpr bool RD_OK = SWP && ES == 2 && WK == 1 && (BN * ES == 128 || BN * ES == 256) && BM * BN * ES <= TILEB && (BM * BN * ES / 1024) % NW == 0;
  constexpr int RD_PCS = RD_OK ? BM * BN * ES / 1024 / NW : 1;
  bool rd_on = false;
  unsigned rd_off = 0;
  if constexpr (DMA) {
    // ---- K loop, LDS-DMA form.  Tile `it` is computed from stage it % DMA while the pieces of tile it+DMA-1 are requested
    // into the stage tile it-1 was read from (free since the barrier taken inside tile it-1).  Before the last MFMA step of a
    // tile (fp32: the third last) every wave (a) waits until ITS pieces of tile it+1 have landed — vmcnt counts requests, the
    // younger tiles stay in flight —, (b) waits for its own fragment reads, (c) takes the one barrier of the tile: after it
    // tile it+1 is complete in LDS for every reader and stage it % DMA may be overwritten.  The first fragments of tile it+1
    // are fetched right there, under the remaining MFMA step(s).
    constexpr int PPW = NA + NBV;  // pieces (1 KiB wave requests) per wave and tile
    static_assert(2 * PPW <= 60, "vmcnt is a 6-bit counter");
    // The stage offsets are run-time scalars and the loop is NOT unrolled over the ring (one body for the steady state, one
    // for the last DMA-1 tiles, one for the last tile): with an unrolled ring and an early exit in the middle the
    // register allocator parked the 64 accumulators in different register classes on the two sides of the loop header
    // and copied all of them (v_accvgpr_read/write) once per round.
    rd_on = RD_OK && c_resid && p.vec_epi && !MC;
    unsigned sb = 0;                    // byte offset of the stage tile `it` is read from
    unsigned sbp = (DMA - 1) * TILEB;   // ... of the stage tile it+DMA-1 goes to (tile it-1 was read from it)
    auto tile = [&](auto more1_tag, auto moreD_tag, int it) {
      constexpr bool more1 = decltype(more1_tag)::value, moreD = decltype(moreD_tag)::value;
      const unsigned sbn = sb + TILEB == DMA * TILEB ? 0u : sb + TILEB;  // stage of tile it+1
      if (moreD) dma_next();
      // One MFMA step = FM*FN matrix instructions; its other work — the FM+FN fragment reads of the next chunk, the wait +
      // barrier + first reads of the next tile (step GBAR), this step's share of the DMA requests — is cut into FM*FN slices
      // and slice m is issued right AFTER matrix instruction m (pinned by sched_barrier): a wave issues in order and a
      // v_mfma_f32_32x32x16_f16 occupies the pipe for 32 cycles, so ~5 other instructions fit into each MFMA's shadow; issued
      // as one block before the step's MFMAs they left the matrix pipe idle for a third of a one-wave-per-SIMD K loop.
      constexpr int NM = FM * FN, NFR = FM + FN;
      auto frag_one = [&](unsigned so, int q, int set, int i) {  // i-th of the FM+FN 16-byte fragment reads of chunk q
        if (i < FM) av[set][i < FM ? i : 0] = *reinterpret_cast<const f32x4*>(smem + so + (frag_a ^ (q * WK * 32)) + (i < FM ? i : 0) * 32 * LDB);
        else bv[set][i >= FM ? i - FM : 0] = *reinterpret_cast<const f32x4*>(smem + so + (frag_b ^ (q * WK * 32)) + (i >= FM ? i - FM : 0) * 32 * LDB);
      };
#pragma unroll
      for (int g = 0; g < NST; ++g) {
        const int q = g / SPC, st = g % SPC, cur = q & 1;
        const bool rd_next = st == 0 && q + 1 < NCH;   // fragment reads of chunk q+1
        const bool sync = g == GBAR && more1;          // wait + barrier + first reads of tile it+1
        const int pc_lo = (g < GBAR && moreD) ? g * PPW / GBAR : 0, pc_hi = (g < GBAR && moreD) ? (g + 1) * PPW / GBAR : 0;
        const int n_sync = sync ? 1 + NFR : 0, n_rd = rd_next ? NFR : 0, n_items = n_sync + n_rd + (pc_hi - pc_lo);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const int a = m / FN, b = m % FN;
          if constexpr (SPC == 4) {
            if constexpr (SWP) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[cur][b][st], av[cur][a][st], acc[a][b], 0, 0, 0);
            else acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][a][st], bv[cur][b][st], acc[a][b], 0, 0, 0);
          } else {
            if constexpr (SWP) acc[a][b] = dc_mfma16<T>(bv[cur][b], av[cur][a], acc[a][b]);
            else acc[a][b] = dc_mfma16<T>(av[cur][a], bv[cur][b], acc[a][b]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = m * n_items / NM; i < (m + 1) * n_items / NM; ++i) {
            if (i < n_sync) {
              if (i == 0) {
                // tiles that may stay in flight: those after it+1 that exist, but never a prologue tile (the prologue requested
                // all filter pieces before all activation pieces, so "the youngest n tiles" only means something for loop tiles)
                if (moreD && it >= DMA - 1) {
                  dc_wait_vm<(DMA - 2) * PPW>();  // steady state: the DMA-2 tiles after it+1 are loop tiles
                } else {
                  int lastq = it + DMA - 1;  // youngest tile requested so far (this tile's own requests precede this point)
                  if (lastq > T_ - 1) lastq = T_ - 1;
                  const int nearly = T_ < DMA - 1 ? T_ : DMA - 1;  // early prologue tiles 0..nearly-1: what is younger than the
                  int npro = (nearly - 1 < lastq ? nearly - 1 : lastq) - (it + 1);  // activation pieces of one of them is NA pieces per later one
                  if (npro < 0) npro = 0;
                  int nloop = lastq - (it + 1 > nearly - 1 ? it + 1 : nearly - 1);  // whole tiles (the late one, the loop's): PPW each
                  if (nloop < 0) nloop = 0;
                  if (DMA >= 4 && nloop == 2) dc_wait_vm<2 * PPW>();
                  else if (DMA >= 4 && nloop == 1 && npro == 1) dc_wait_vm<NA + PPW>();
                  else if (DMA >= 3 && nloop == 1) dc_wait_vm<PPW>();
                  else if (DMA >= 4 && npro == 2) dc_wait_vm<2 * NA>();
                  else if (DMA >= 3 && npro == 1) dc_wait_vm<NA>();
                  else dc_wait_vm<0>();
                }
#if defined(DC_ABL) && (DC_ABL & 2)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
                dc_lds_barrier();
#endif
              } else {
#if !(defined(DC_ABL) && (DC_ABL & 4))
                frag_one(sbn, 0, 0, i - 1);
#endif
              }
            } else if (i < n_sync + n_rd) {
#if !(defined(DC_ABL) && (DC_ABL & 4))
              frag_one(sb, q + 1, cur ^ 1, i - n_sync);
#endif
            } else {
#if !(defined(DC_ABL) && (DC_ABL & 1))
              dma_piece(sbp, pc_lo + (i - n_sync - n_rd));
#endif
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      sbp = sb;
      sb = sbn;
    };
    int it = 0;
    if (LATE && T_ >= DMA) {  // the prologue filled the whole ring: tile 0 has nothing to request
      tile(std::true_type{}, std::false_type{}, 0);
      it = 1;
    }
    for (; it < T_ - (DMA - 1); ++it) tile(std::true_type{}, std::true_type{}, it);
    for (; it < T_ - 1; ++it) tile(std::true_type{}, std::false_type{}, it);
    if constexpr (RD_OK) {
      // Shortcut tile by LDS-DMA: while the last K tile computes, the BM x BN shortcut values travel into the stage the
      // previous tile was read from (free since that tile's barrier) — whole 128- / 256-byte pixel rows per request (the
      // swapped-operand epilogue would otherwise fetch them as 32-byte fragments of 32 different lines per instruction),
      // no VGPRs, and a tile's time earlier than the epilogue could ask for them.  Same swizzle as the operand tiles.
      if (rd_on) {
        rd_off = sbp;
        constexpr int RB = BN * ES, LPR = RB / 16, PPP = 1024 / RB;  // row bytes, lanes per row, pixels per 1 KiB piece
        const i32x4 rrs = dc_rsrc_words(reinterpret_cast<const T*>(c_resid) + c_yoff);
#pragma unroll
        for (int j = 0; j < RD_PCS; ++j) {
          const int px_ = (j * NW + wave) * PPP + lane / LPR;        // tile row
          const int c = (lane % LPR) ^ (RB == 256 ? (px_ & 15) : ((px_ >> 1) & 7));
          const int yo = rowinfo[px_];
          const int co = n0 + c * VEC;
          const unsigned vo = (yo >= 0 && co < p.Cout) ? (unsigned)yo + (unsigned)co * ES : kOOB;
          dc_dma16(rrs, ldsw + sbp + j * NW * 1024, vo, 0);
        }
      }
    }
    tile(std::false_type{}, std::false_type{}, it);
  } else
  for (int it0 = 0; it0 < T_; it0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int it = it0 + u;
      if (it >= T_) break;
      const int buf = it & 1;
      const int slot = (u + 1) % PF;  // ring slot of tile it+1 (it0 is a multiple of PF)
      const bool more1 = it + 1 < T_, moreP = it + 1 + PF < T_;
#pragma unroll
      for (int g = 0; g < NST; ++g) {
        const int q = g / SPC, st = g % SPC, cur = q & 1;
        if (st == 0 && q + 1 < NCH) frag_load(buf, q + 1, cur ^ 1);
        if (g == GBAR && more1) {  // every fragment read of this stage has been issued (and is waited for here)
          __syncthreads();
          frag_load(buf ^ 1, 0, 0);
        }
        if (g == 1 && more1) lstore(buf ^ 1, slot);
        if (g == 2 && moreP) gload_a(slot);
        if (g == 3 && moreP) gload_b(slot);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b) {
            if constexpr (SPC == 4)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][a][st], bv[cur][b][st], acc[a][b], 0, 0, 0);
            else
              acc[a][b] = dc_mfma16<T>(av[cur][a], bv[cur][b], acc[a][b]);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  stamp(5);
  // ---- epilogue ---------------------------------------------------------------------------------------
  // in-workgroup split-K: wave wk keeps registers [wk*RPW, (wk+1)*RPW) of every fragment and receives
  // the other waves' partials for them through LDS, so all waves store (no idle waves, 1/WK of the
  // LDS traffic of a gather-to-one reduction).  The body is instantiated once per value of wk (wave-uniform
  // branch) so that every accumulator index is a compile-time constant: no v_cndmask register selects.
  auto finish = [&](auto wk_tag) {
    constexpr int MYK = decltype(wk_tag)::value;
    const bool wide = WIDE_OK && p.wide_epi;  // uniform
    f32x4 wres[WIDE_OK ? WVEC : 1];             // shortcut vectors (8 halves each) of this thread's output vectors
    unsigned woff[WIDE_OK ? WVEC : 1];
    if constexpr (WIDE_OK) {
      if (wide) {
#pragma unroll
        for (int i = 0; i < WVEC; ++i) {
          const int v = t + i * NT, row = v / (BN / 8), cv = v - row * (BN / 8);
          const int yo = rowinfo[row];
          const int co = n0 + cv * 8;
          woff[i] = (yo >= 0 && co < p.Cout) ? (unsigned)yo + co * ES : kOOB;  // Cout % 8 == 0: a vector is all in or all out
          if (c_resid) wres[i] = dc_bload4(rr, woff[i], 0);
        }
      }
    }
    if (WK > 1) {
      __syncthreads();  // tile buffers are free
      float* part = reinterpret_cast<float*>(smem);
      // layout: [dst wave q][src wave (!= q) slot][wr*WC+wc][a][b][e][lane]
#pragma unroll
      for (int q = 0; q < WK; ++q) {
        if (q == MYK) continue;
        const int srcslot = MYK < q ? MYK : MYK - 1;
        float* dst = part + ((((q * (WK - 1) + srcslot) * WR * WC + wr * WC + wc) * FM * FN) * RPW) * 64 + lane;
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b)
#pragma unroll
            for (int e = 0; e < RPW; ++e) dst[((a * FN + b) * RPW + e) * 64] = acc[a][b][q * RPW + e];
      }
      __syncthreads();
#pragma unroll
      for (int sslot = 0; sslot < WK - 1; ++sslot) {
        const float* src = part + ((((MYK * (WK - 1) + sslot) * WR * WC + wr * WC + wc) * FM * FN) * RPW) * 64 + lane;
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b)
#pragma unroll
            for (int e = 0; e < RPW; ++e) acc[a][b][MYK * RPW + e] += src[((a * FN + b) * RPW + e) * 64];
      }
    }
    stamp(6);
    if constexpr (SWP) {
      // Swapped-operand accumulators: register r of fragment (a, b) is pixel wr*TM + a*32 + (lane & 31), channel
      // wc*TN + b*32 + 8*(r >> 2) + 4*(lane >> 5) + (r & 3): four runs of 4 consecutive channels.  float32: a run IS a 16-byte
      // vector.  float16: after the affine, v_permlane32_swap between the registers of runs g and g+1 leaves lanes 0..31 with
      // channels 8g..8g+7 and lanes 32..63 with 8g+8..8g+15 of their pixel: 16-byte vectors again, formed in registers.
      constexpr int NG = RPW / 4;  // runs per fragment this wave finalises
      const int h = lane >> 5;
      const float* scl = epi_sc;
      const float* shl = epi_sc + BN;
      int yo[FM];
#pragma unroll
      for (int a = 0; a < FM; ++a) yo[a] = rowinfo[wr * TM + a * 32 + (lane & 31)];
      if (p.vec_epi && (ES == 4 || NG >= 2)) {
        constexpr int NV = ES == 4 ? NG : (NG >= 2 ? NG / 2 : 1);  // 16-byte vectors per fragment
        f32x4 rv[FM][FN][NV];
        unsigned off[FM][FN][NV];
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b)
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const int g0 = MYK * NG + (ES == 4 ? j : 2 * j);
              const int co = n0 + wc * TN + b * 32 + (ES == 4 ? 8 * g0 + 4 * h : 8 * (g0 + h));
              off[a][b][j] = (yo[a] >= 0 && co < p.Cout) ? (unsigned)yo[a] + (unsigned)co * ES : kOOB;
              rv[a][b][j] = f32x4{0.f, 0.f, 0.f, 0.f};  // no shortcut: + 0 (one add instead of a select per element)
              if (c_resid && !rd_on) rv[a][b][j] = dc_bload4(rr, off[a][b][j], 0);
            }
        // ReLU is a template tag of `emit` below (uniform branch, like the shortcut): a ReLU-less layer stores its value
        // untouched, so a NaN / inf accumulator (a numerically broken model, a float16 overflow) propagates as it does in the
        // reference and in the element-wise path instead of being masked by max(x, -inf).
        if constexpr (RD_OK) {
          if (rd_on) {
            dc_wait_vm<0>();
            dc_lds_barrier();  // every wave's pieces of the shortcut tile have landed
            constexpr int RB = BN * ES;
#pragma unroll
            for (int a = 0; a < FM; ++a) {
              const int px_ = wr * TM + a * 32 + (lane & 31);
              const int sw = RB == 256 ? (px_ & 15) : ((px_ >> 1) & 7);
#pragma unroll
              for (int b = 0; b < FN; ++b)
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                  const int c = (wc * TN + b * 32 + 8 * (2 * j + h)) / 8;  // 16-byte chunk of the row (WK == 1: g0 = 2j)
                  rv[a][b][j] = *reinterpret_cast<const f32x4*>(smem + rd_off + px_ * RB + ((c ^ sw) * 16));
                }
            }
          }
        }
        // float16: the shortcut add reads its half straight from the packed register (v_fma_mix_f32: one instruction instead of a
        // conversion and an add — the same exactly rounded sum), two results are rounded and packed by one v_cvt_pk_f16_f32 and the
        // ReLU is a v_pk_max_f16 on the packed pair (rounding is monotonic and 0 / -inf are exact: max-then-round == round-then-max):
        // 28 VALU instructions per 16-byte vector with a shortcut, 20 without, instead of 48 — with three workgroups per CU
        // in their epilogues at once this phase is bound by VALU issue.
        auto emit = [&](auto res_tag, auto relu_tag) {
          constexpr bool HAS_RES = decltype(res_tag)::value, RELU = decltype(relu_tag)::value;
          const f16x2 rl2 = {(_Float16)0.f, (_Float16)0.f};
#pragma unroll
          for (int b = 0; b < FN; ++b)
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const int g0 = MYK * NG + (ES == 4 ? j : 2 * j);
              if constexpr (ES == 4) {
                const int cb = wc * TN + b * 32 + 8 * g0 + 4 * h;
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(scl + cb), h4 = *reinterpret_cast<const f32x4*>(shl + cb);
#pragma unroll
                for (int a = 0; a < FM; ++a) {
                  f32x4 o;
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    float v = acc[a][b][4 * g0 + e] * s4[e] + h4[e];
                    if (HAS_RES) v += rv[a][b][j][e];
                    o[e] = RELU ? fmaxf(v, 0.f) : v;
                  }
                  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), yr, off[a][b][j], 0, 0);
                }
              } else {
                const int cb0 = wc * TN + b * 32 + 8 * g0 + 4 * h, cb1 = cb0 + 8;
                const f32x4 s0 = *reinterpret_cast<const f32x4*>(scl + cb0), h0 = *reinterpret_cast<const f32x4*>(shl + cb0);
                const f32x4 s1 = *reinterpret_cast<const f32x4*>(scl + cb1), h1 = *reinterpret_cast<const f32x4*>(shl + cb1);
#pragma unroll
                for (int a = 0; a < FM; ++a) {
                  float lo[4], hi[4];
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    lo[e] = acc[a][b][4 * g0 + e] * s0[e] + h0[e];
                    hi[e] = acc[a][b][4 * g0 + 4 + e] * s1[e] + h1[e];
                  }
                  dc_permlane32_swap4(lo, hi);
                  const u32x4 rz = __builtin_bit_cast(u32x4, rv[a][b][j]);
                  u32x4 o;
#pragma unroll
                  for (int i = 0; i < 4; ++i) {
                    float x0 = i < 2 ? lo[2 * i] : hi[2 * i - 4], x1 = i < 2 ? lo[2 * i + 1] : hi[2 * i - 3];
                    if constexpr (std::is_same_v<T, __bf16>) {
                      // bfloat16: no mixed-precision add — the shortcut pair is widened by a shift / a mask (exact), added in float,
                      // ReLU'd in float and the pair rounded once by v_cvt_pk_bf16_f32
                      if (HAS_RES) {
                        x0 += __builtin_bit_cast(float, rz[i] << 16);
                        x1 += __builtin_bit_cast(float, rz[i] & 0xffff0000u);
                      }
                      if (RELU) x0 = fmaxf(x0, 0.f), x1 = fmaxf(x1, 0.f);
                      const f32x2 xp = {x0, x1};
                      o[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(xp, bf16x2));
                    } else {
                      if (HAS_RES) {
                        x0 = dc_add_half_lo(rz[i], x0);
                        x1 = dc_add_half_hi(rz[i], x1);
                      }
                      const f32x2 xp = {x0, x1};
                      f16x2 hp = __builtin_convertvector(xp, f16x2);
                      if (RELU) hp = __builtin_elementwise_max(hp, rl2);
                      o[i] = __builtin_bit_cast(unsigned, hp);
                    }
                  }
                  __builtin_amdgcn_raw_buffer_store_b128(o, yr, off[a][b][j], 0, 0);
                }
              }
            }
        };
        if (c_resid) {
          if (p.relu) emit(std::true_type{}, std::true_type{});
          else emit(std::true_type{}, std::false_type{});
        } else {
          if (p.relu) emit(std::false_type{}, std::true_type{});
          else emit(std::false_type{}, std::false_type{});
        }
      } else {
        // element-wise form (odd channel counts, sigmoid heads, unaligned views, split-K 4 in float16)
#pragma unroll
        for (int b = 0; b < FN; ++b)
#pragma unroll
          for (int a = 0; a < FM; ++a)
#pragma unroll
            for (int gg = 0; gg < NG; ++gg) {
              const int g = MYK * NG + gg;
              const int cb = wc * TN + b * 32 + 8 * g + 4 * h;
              const f32x4 s4 = *reinterpret_cast<const f32x4*>(scl + cb), h4 = *reinterpret_cast<const f32x4*>(shl + cb);
              unsigned eo[4];
              float rvv[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int co = n0 + cb + e;
                eo[e] = (yo[a] >= 0 && co < p.Cout) ? (unsigned)yo[a] + (unsigned)co * ES : kOOB;
                rvv[e] = c_resid ? Elem<T>::load(rr, eo[e]) : 0.f;
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                float v = acc[a][b][4 * g + e] * s4[e] + h4[e] + rvv[e];
                if (p.relu) v = fmaxf(v, 0.f);
                if (n0 + cb + e < p.sigmoid_ch) v = 1.f / (1.f + expf(-v));
                Elem<T>::store(v, yr, eo[e]);
              }
            }
      }
      return;
    }
    if constexpr (WIDE_OK) {
      if (wide) {
        float* stg = reinterpret_cast<float*>(smem);
        __syncthreads();  // every wave is past its reads of the tile buffers / the split-K partials
#pragma unroll
        for (int b = 0; b < FN; ++b)
#pragma unroll
          for (int a = 0; a < FM; ++a)
#pragma unroll
            for (int e = 0; e < RPW; ++e) {
              const int r = MYK * RPW + e;
              const int row = wr * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
              stg[row * WPS + wc * TN + b * 32 + (lane & 31)] = acc[a][b][r] * sc[b] + sh[b];
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < WVEC; ++i) {
          const int v = t + i * NT, row = v / (BN / 8), cv = v - row * (BN / 8);
          const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + row * WPS + cv * 8);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + row * WPS + cv * 8 + 4);
          typedef T t8 __attribute__((ext_vector_type(8)));  // 8 halves / 8 bfloat16s
          t8 rz = __builtin_bit_cast(t8, wres[i]);
          t8 o;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            float x = (q < 4 ? lo[q] : hi[q - 4]) + (c_resid ? (float)rz[q] : 0.f);
            if (p.relu) x = fmaxf(x, 0.f);
            o[q] = (T)x;
          }
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), yr, woff[i], 0, 0);
        }
        return;
      }
    }
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const int co = n0 + wc * TN + b * 32 + (lane & 31);
      const bool cok = co < p.Cout;
      const bool sig = co < p.sigmoid_ch;
#pragma unroll
      for (int a = 0; a < FM; ++a) {
        unsigned off[RPW];
        float rv[RPW];
#pragma unroll
        for (int e = 0; e < RPW; ++e) {
          const int r = MYK * RPW + e;
          const int yo = rowinfo[wr * TM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
          off[e] = (yo >= 0 && cok) ? (unsigned)yo + co * ES : kOOB;  // masked lanes: load 0 / store dropped
        }
        if (EARLY_RESID) {
#pragma unroll
          for (int e = 0; e < RPW; ++e) rv[e] = c_resid ? rs[(a * FN + b) * RPW + e] : 0.f;
        } else if (c_resid) {  // all shortcut loads of the fragment in flight at once
#pragma unroll
          for (int e = 0; e < RPW; ++e) rv[e] = Elem<T>::load(rr, off[e]);
        } else {
#pragma unroll
          for (int e = 0; e < RPW; ++e) rv[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < RPW; ++e) {
          float v = acc[a][b][MYK * RPW + e] * sc[b] + sh[b] + rv[e];
          if (p.relu) v = fmaxf(v, 0.f);
          if (sig) v = 1.f / (1.f + expf(-v));
          Elem<T>::store(v, yr, off[e]);
        }
      }
    }
  };
  if constexpr (WK == 1) {
    finish(std::integral_constant<int, 0>{});
  } else if constexpr (WK == 2) {
    if (wk == 0) finish(std::integral_constant<int, 0>{});
    else finish(std::integral_constant<int, 1>{});
  } else if constexpr (WK == 4) {
    if (wk == 0) finish(std::integral_constant<int, 0>{});
    else if (wk == 1) finish(std::integral_constant<int, 1>{});
    else if (wk == 2) finish(std::integral_constant<int, 2>{});
    else finish(std::integral_constant<int, 3>{});
  } else {
    static_assert(WK == 8, "WK is 1, 2, 4 or 8");
    if (wk == 0) finish(std::integral_constant<int, 0>{});
    else if (wk == 1) finish(std::integral_constant<int, 1>{});
    else if (wk == 2) finish(std::integral_constant<int, 2>{});
    else if (wk == 3) finish(std::integral_constant<int, 3>{});
    else if (wk == 4) finish(std::integral_constant<int, 4>{});
    else if (wk == 5) finish(std::integral_constant<int, 5>{});
    else if (wk == 6) finish(std::integral_constant<int, 6>{});
    else finish(std::integral_constant<int, 7>{});
  }
  stamp(7);
}

// The instantiations of one row of conv_gemm_variants.h: single problem, multi-problem and, where the row is marked _MC, multi-class
// (what the row's table entry in conv_gemm.cpp points to).
#define DC_CONV_GEMM_ROW(T, NAME, BM, BN, BK, WR, WC, WK, PF, DMA, SWP, WITH_MC)                                     \
  template __global__ void conv_gemm_kernel<T, BM, BN, BK, WR, WC, WK, PF, false, DMA, SWP>(const ConvGemmParams);   \
  template __global__ void conv_gemm_kernel<T, BM, BN, BK, WR, WC, WK, PF, false, DMA, SWP, true>(const ConvMultiArgs); \
  DC_CONV_GEMM_MC_##WITH_MC(T, BM, BN, BK, WR, WC, WK, PF, DMA, SWP)
#define DC_CONV_GEMM_MC_false(T, BM, BN, BK, WR, WC, WK, PF, DMA, SWP)
#define DC_CONV_GEMM_MC_true(T, BM, BN, BK, WR, WC, WK, PF, DMA, SWP) \
  template __global__ void conv_gemm_kernel<T, BM, BN, BK, WR, WC, WK, PF, true, DMA, SWP>(const ConvGemmParams);

}  // namespace dc
