// wino_f32.hip — the float32 Winograd F(2x2, 3x3) kernel of the stride-1 3x3 convolutions and its host side: the forms wino_f23,
// wino_f23_w16, wino_f23_5x6, wino_f23_5x6_w16, wino_f23_mix and wino_f23_mix_w16 of forms.cpp (its float16 counterpart: wino_f16.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_gemm.h"  // DC_KARG_TOUCH, DC_KARG_HOLD
#include "kernel_prims.h"
#include "kernels.h"

namespace dc {

// =====================================================================================================================
// Winograd F(2x2, 3x3): Y = A^T [ (G g G^T) . (B^T d B) ] A per 4x4 input patch d -> 2x2 outputs, summed over input
// channels as 16 independent GEMMs (one per transform position (i, j)): 2.25x fewer MFMA flops than the direct form.
//
// At batch 1 a res4 layer has only 391 tiles x 256 channels, so the kernel is built around operand TRAFFIC, not flops:
//  * workgroup = 4 x 8 tiles (two 16-tile MFMA fragments) x 16 output channels, 8 waves = (transform row i) x (fragment);
//    a wave owns the 4 positions (i, 0..3) of its fragment: 4 accumulators of v_mfma_f32_16x16x4_f32;
//  * the 10 x 18 input pixels the block reads are staged ONCE per 32 channels in LDS (ring of 3, one barrier per 32
//    channels); every wave reads the two patch rows its transform row needs and does B^T d B in registers (packed fp32)
//    right before its MFMAs — the transformed input never exists in memory;
//  * the transformed filters are the big stream (16/9 of the filter bytes, no reuse inside a workgroup): pre-packed on
//    the host so that each wave reads its B fragments straight from global memory, 1 KB contiguous per load, one
//    sub-step ahead; workgroups that share them (same 16 output channels) are adjacent in the grid;
//  * 104 VGPRs (96 in the 16-wave form) and 80.7 KB of LDS (75.6 KB on 5 x 6-tile blocks): two workgroups per CU, so that forwards in flight can share CUs (with the register-
//    hungrier pipelined variant of the probe the kernel was as fast alone but worth nothing with three forwards in flight);
//  * the inverse transform reduces over j in registers and over i (four waves) through LDS, then applies the folded
//    BatchNorm/Scale affine, the shortcut and ReLU like the gather-GEMM's epilogue.
// Round 5 (tools/probes/winograd16_probe.hip, profiles/r05_winograd16_probe.txt):
//  * LDS row pitch 672 floats, no skew.  A ds_read_b128 is served in four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,
//    28-31}, ...: MI355X_MICROARCH.md, LDS), one LDS cycle per group whose lanes touch 64 distinct banks.  A fragment read
//    addresses row(r) * pitch + 2 c * WPSTR + 4 kg floats (r = lane[3] tile row, c = lane[2:0] tile column, kg = lane[5:4]
//    channel quad); with WPSTR = 36 the groups are conflict-free iff two rows' pitch is a multiple of 64 floats: 2 * 672 =
//    21 * 64.  The round-1 layout (pitch 648 + a 4-float skew per row pair) paid 8 LDS cycles per read instead of 4;
//  * buffer (V#) addressing for the staged pixels and the filter fragments: loop-invariant per-thread voffsets, the channel
//    step in soffset, zero padding = an out-of-range voffset — no 64-bit address arithmetic, no predicated loads, no zero
//    fills in the K loop (70 -> 44 VALU instructions per 32 MFMAs: on gfx950 VALU work is paid on top of fp32 MFMA work);
//  * NG = 2 (tile name wino_f23_w16): SIXTEEN waves, the two 16-channel sub-steps of a staged step dealt to two groups of
//    eight.  A launch of at most one workgroup per CU (res4 at batch 1: 240) leaves two waves per SIMD, which cannot cover
//    each other's barrier, LDS and transform phases (K loop 27.3 k cycles for 16.4 k of MFMA); four waves per SIMD from ONE
//    workgroup do (23.3 k), once the LDS reads are conflict-free (with the old layout the 16-wave form was LDS-bound and
//    slower: 35.5 k).  Under load (grids of several rounds, forwards in flight) two 8-wave workgroups per CU are faster
//    than one 16-wave one: the autotuner decides per shape, tune_in_flight under the caller's load.
// Measured on the res4 3x3 shape (1x34x46, 256 -> 256; operands rotated through 355 MB): round-1 kernel 18.7 us alone /
// 13.4 us per image at 8 images per launch; NG = 1 now 17.5 / 11.7; NG = 2 15.95 / 13.5.
namespace {
constexpr int WBTY = 4, WBTX = 8, WBN = 16, WKC = 32;   // (WBTY x WBTX tiles: the default block)
constexpr int WPSTR = WKC + 4;                           // floats per staged pixel
constexpr int WPITCH = 672;                              // floats per staged pixel row of the default block: >= 18 * WPSTR = 648, and 2 * WPITCH % 64 == 0
constexpr int WNTH = 512;
// The block geometry of wino_f23_kernel: a 16-row MFMA fragment holds FR x FC tiles (lane q = lane & 15 -> tile (q / FC, q % FC); rows
// past FR * FC carry no tile), a workgroup's block is two fragments, stacked (2 FR x FC tiles) or side by side (FR x 2 FC); PITCH is
// the LDS row pitch of the staged pixels in floats.  The geometry enters the kernel in four places only: the staging map, the per-lane
// patch-row offsets, the epilogue's q -> (ty, tx), and the host's grid.  Filter image, K loop, ring and epilogue arithmetic are shared,
// and a tile's sums do not depend on the slot it sits in: the geometries give the same bits.
//  * 4 x 8 = {2 x 8, stacked, pitch 672}: 10 x 18 staged pixels.  The form of every shape until the dilated res5 layers, and the default.
//  * 5 x 6 = {5 x 3, side by side, pitch 524}: 12 x 14 staged pixels, 15 of a fragment's 16 rows in use.  A 9 x 12 tile grid (a
//    phase image of res5 3x3 dilation 2 at 544x736) is 2 x 2 = 4 such blocks against 3 x 2 = 6 of the 4 x 8 ones: 768 -> 512 workgroups,
//    two per CU in one round.  Offered to the autotuner where it needs strictly fewer blocks only (wino_fewer_blocks).
//  * mixed (WinoGMix) = both in ONE launch: the tile grid is cut once, straight, into a region of 4 x 8 blocks (at the grid's origin) and a
//    region of 5 x 6 blocks (wino_plan_cover); a workgroup takes its geometry, wave-uniformly, from its block index.  The four places above
//    are computed per geometry in front of the K loop and in the epilogue; ring (on the larger stage's stride), K loop and epilogue
//    arithmetic are one code path.  A res4 image (17 x 23 tiles) is 9 + 4 = 13 blocks against 15 of 4 x 8 and 16 of 5 x 6.
template <int FR_, int FC_, bool SIDE_, int PITCH_>
struct WinoGeom {
  static constexpr int FR = FR_, FC = FC_, NT = FR_ * FC_, PITCH = PITCH_;
  static constexpr bool SIDE = SIDE_;
  static constexpr int BTY = SIDE_ ? FR_ : 2 * FR_, BTX = SIDE_ ? 2 * FC_ : FC_;  // tiles of a block
  static constexpr int RH = 2 * BTY + 2, RW = 2 * BTX + 2;                        // staged pixels
  static constexpr int STAGE = RH * PITCH_ + 8;                                   // + the dump slot of the staging threads past the block
  static constexpr int PIXELS = RH * RW;
  static constexpr bool MIX = false;
  // tile (row, column) inside the block of row q of fragment tf: the fragment's first tile + (q / FC, q % FC)
  static constexpr int frow(int tf) { return SIDE_ ? 0 : FR_ * tf; }
  static constexpr int fcol(int tf) { return SIDE_ ? FC_ * tf : 0; }
  static constexpr int trow(int tf, int q) { return frow(tf) + q / FC_; }
  static constexpr int tcol(int tf, int q) { return fcol(tf) + q % FC_; }
  // The LDS model of the comment above: a ds_read_b128 is served in groups of 16 lanes, each made of the eight fragment rows {0-3, 12-15}
  // of one channel quad and the rows {4-11} of the next one; a group takes one LDS cycle iff its lanes' 16-byte slots differ mod 16.
  // (A row without a tile reads the last tile's address: a broadcast.)  True: every fragment read is conflict-free.
  static constexpr bool conflict_free() {
    for (int tf = 0; tf < 2; ++tf)
      for (int flip = 0; flip < 2; ++flip) {
        bool seen[16] = {};
        for (int q = 0; q < NT; ++q) {
          const int slot = ((2 * trow(tf, q) * PITCH_ + 2 * tcol(tf, q) * WPSTR) / 4 + ((q >= 4 && q < 12) != (flip != 0) ? 1 : 0)) & 15;
          if (seen[slot]) return false;
          seen[slot] = true;
        }
      }
    return true;
  }
  static_assert(NT <= 16 && PITCH_ >= RW * WPSTR && WPSTR == 36 && conflict_free(), "conflict-free ds_read_b128 layout (see above)");
  static_assert(PITCH_ % 4 == 0 && WPSTR % 4 == 0 && STAGE % 4 == 0, "16-byte units");
};
using WinoG48 = WinoGeom<WBTY / 2, WBTX, false, WPITCH>;  // 2 * 672 = 21 * 64 floats
using WinoG56 = WinoGeom<5, 3, true, 524>;   // 524 / 2 = 6 (mod 16) slots per tile row, 2 per tile column: the tiles of each half of a group on distinct even slots
static_assert(WinoG48::BTY == 4 && WinoG48::BTX == 8 && WinoG48::RH == 10 && WinoG48::RW == 18, "the 4 x 8 block");
static_assert(WinoG56::BTY == 5 && WinoG56::BTX == 6 && WinoG56::RH == 12 && WinoG56::RW == 14, "the 5 x 6 block");
// a launch of blocks of both geometries: region A = WinoG48, region B = WinoG56 (per block: ConvGemmParams::w_mix_*); the ring's stride and the
// staging loads per thread are the larger of the two
struct WinoGMix {
  static constexpr int STAGE = std::max(WinoG48::STAGE, WinoG56::STAGE), PIXELS = std::max(WinoG48::PIXELS, WinoG56::PIXELS);
  static constexpr bool MIX = true;
};
__device__ __forceinline__ f32x2 wlo(f32x4 v) { return __builtin_shufflevector(v, v, 0, 1); }
__device__ __forceinline__ f32x2 whi(f32x4 v) { return __builtin_shufflevector(v, v, 2, 3); }
}  // namespace

template <int NG, class G>
__global__ __launch_bounds__(WNTH * NG, 4) void wino_f23_kernel(const ConvGemmParams p) {
  constexpr int NTH = WNTH * NG;
  constexpr int WSTAGE = G::STAGE;
  constexpr int WNLD = (G::PIXELS * (WKC / 4) + NTH - 1) / NTH;
  const long long t_entry = (long long)__builtin_amdgcn_s_memrealtime();
  DC_KARG_TOUCH(ka0, ka1, ka2, ka3, ka4);
  unsigned ka5 = 0;  // (mixed launches: the sixth line, the w_mix_* fields' (kernels.h asserts that they are one line), with the others)
  if constexpr (G::MIX) asm volatile("s_load_dword %0, %1, %2" : "=&s"(ka5) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(offsetof(ConvGemmParams, w_mix_na)));
  __shared__ __attribute__((aligned(16))) float stage[3][WSTAGE];
  // [g][i][b][tf][r][lane] partial inverse transforms: reuses the staging ring once the K loop is over (79 KB per
  // workgroup: two 8-wave workgroups fit the 160 KB of a CU)
  float (*part)[4][2][2][4][64] = reinterpret_cast<float (*)[4][2][2][4][64]>(&stage[0][0]);
  static_assert(sizeof(float) * NG * 4 * 2 * 2 * 4 * 64 <= sizeof(stage), "partials must fit in the staging ring");
  static_assert(2 * sizeof(stage) <= 160 * 1024, "two workgroups per CU");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  auto stamp = [&](int slot) {  // DC_DEBUG_TIMING: per-wave phase stamps (see conv_gemm_kernel)
    if (p.dbg && lane == 0) {
      long long* d = p.dbg + ((long)blockIdx.x * (8 * NG) + wave) * 12;
      d[slot] = (long long)__builtin_readcyclecounter();
      if (slot == 0) d[8] = t_entry, d[10] = (long long)__builtin_amdgcn_s_memrealtime();
      if (slot == 7) d[9] = (long long)__builtin_amdgcn_s_memrealtime();
    }
  };
  stamp(0);
  const int C = p.klen, H = p.x_rows, W = p.x_rowlen / p.klen;
  // dilation d: the image is d*d interleaved phase images, each an ordinary pad-1 3x3 problem on the pixels
  // (phy + d*u, phx + d*v); tiles, blocks and staged coordinates below live on the phase grid (u, v)
  // (the tile grid and the magic numbers of the block-index divisions come from the host: seven runtime integer
  // divisions were 2.8 k cycles of every workgroup's life)
  const int d = p.ddy;
  const int NBY = p.w_NBY, NBX = p.w_NBX;
  const int nblk = p.w_nblk;
  // Workgroup b runs on XCD (b % 8), each XCD with its own L2.  The transformed filters are the big stream (16/9 of the
  // filter bytes), shared by the nblk workgroups of a 16-channel slice: hand every XCD a CONTIGUOUS range of the
  // (slice-major) logical grid, so that a slice is fetched from HBM by one L2 (two at a range boundary) instead of by
  // all eight.  A locality hint only: any bijection of the grid computes the same result.
  int lb = blockIdx.x;
  if (p.xcd_on) {
    const int g8 = gridDim.x >> 3, r8 = gridDim.x & 7, q = blockIdx.x & 7;
    lb = q * g8 + min(q, r8) + (blockIdx.x >> 3);
  }
  const int nt = dc_fastdiv(lb, p.w_div_nblk), blk = lb - nt * nblk;  // same-filter workgroups are adjacent in the logical grid
  const int nph = dc_fastdiv(blk, p.w_div_nbyx), brem = blk - nph * (G::MIX ? p.w_mix_nab : NBY * NBX);
  const int n = dc_fastdiv(nph, p.w_div_dd), ph = nph - n * (d * d);
  const int phy = dc_fastdiv(ph, p.w_div_d), phx = ph - phy * d;
  // block (by, bx) of its region's block grid, whose first tile is (rty0, rtx0).  Mixed launches: blocks [0, nA) of a phase image are region
  // A (4 x 8, from the grid's origin), the others region B (5 x 6, from its own origin): scalar selects, everything here is uniform
  bool in_b = false;
  int by, bx, rty0 = 0, rtx0 = 0, oy0, ox0;  // (oy0, ox0): phase-grid coordinates of staged pixel (0, 0): pad 1
  if constexpr (G::MIX) {
    in_b = brem >= p.w_mix_na;
    const int br = in_b ? brem - p.w_mix_na : brem;
    by = in_b ? dc_fastdiv(br, p.w_mix_div_nbx) : dc_fastdiv(br, p.w_div_nbx), bx = br - by * (in_b ? p.w_mix_NBX : NBX);
    rty0 = in_b ? p.w_mix_ty0 : 0, rtx0 = in_b ? p.w_mix_tx0 : 0;
    oy0 = 2 * (rty0 + (in_b ? WinoG56::BTY : WinoG48::BTY) * by) - 1, ox0 = 2 * (rtx0 + (in_b ? WinoG56::BTX : WinoG48::BTX) * bx) - 1;
  } else {
    by = dc_fastdiv(brem, p.w_div_nbx), bx = brem - by * NBX;
    oy0 = 2 * G::BTY * by - 1, ox0 = 2 * G::BTX * bx - 1;
  }
  DC_KARG_HOLD(ka0, ka1, ka2, ka3, ka4);  // the block decode above needed kernel arguments: the dummy loads have landed
  if constexpr (G::MIX) asm volatile("" ::"s"(ka5));
  const int kg = lane >> 4;
  const int grp = NG == 1 ? 0 : __builtin_amdgcn_readfirstlane(wave >> 3);  // (an SGPR: it enters the filter loads' soffset)
  const int i = wave & 3, tf = (wave >> 2) & 1;
  // B^T row i as a combination of two patch rows: i=0: d0-d2, 1: d1+d2, 2: d2-d1, 3: d1-d3
  const int ra = i == 0 ? 0 : (i == 2 ? 2 : 1), rb = i == 0 ? 2 : (i == 1 ? 2 : (i == 2 ? 1 : 3));
  const float sb = i == 1 ? 1.f : -1.f;
  // V# addressing (see dc_rsrc): per-thread byte offsets are loop invariant, the 32-channel step travels in soffset, a pixel
  // outside the image is an out-of-range voffset (zeros); the image base (n is uniform) sits in the descriptor
  const __amdgpu_buffer_rsrc_t xr = dc_rsrc(reinterpret_cast<const float*>(p.x) + (long)n * p.x_img_stride, 0x7fffffffu);
  const __amdgpu_buffer_rsrc_t ur = dc_rsrc(p.w, 0x7fffffffu);
  unsigned gofs[WNLD];
  int sofs[WNLD], ofs_a, ofs_b;
  if constexpr (!G::MIX) {
    // (written out, not through index_setup below: the same statements behind a generic lambda cost the 16-wave 4 x 8 kernel the packed form of
    // five fp32 instructions of its K loop in the compiler's late scheduling)
#pragma unroll
    for (int q = 0; q < WNLD; ++q) {
      const int e = t + q * NTH;
      const int pix = e / (WKC / 4), cq = e % (WKC / 4);
      const int py = pix / G::RW, px = pix % G::RW;
      const int iy = phy + d * (oy0 + py), ix = phx + d * (ox0 + px);
      const bool ok = pix < G::PIXELS && oy0 + py >= 0 && ox0 + px >= 0 && iy < H && ix < W;
      gofs[q] = ok ? (unsigned)(iy * p.x_row_stride + ix * C + cq * 4) * 4u : kOOB;
      sofs[q] = (pix < G::PIXELS ? py * G::PITCH + px * WPSTR + cq * 4 : WSTAGE - 8 + (t & 1) * 4) >> 2;  // in float4 units (past the block: the dump slot)
    }
    // (a fragment row without a tile reads the last tile's patch: in range, a broadcast, and kept out of the stores below)
    const int qt = G::NT < 16 ? min(lane & 15, G::NT - 1) : lane & 15;
    const int r = qt / G::FC, c = G::fcol(tf) + qt % G::FC;
    ofs_a = (2 * (G::frow(tf) + r) + ra) * G::PITCH + 2 * c * WPSTR + kg * 4;
    ofs_b = (2 * (G::frow(tf) + r) + rb) * G::PITCH + 2 * c * WPSTR + kg * 4;
  } else {
    // the staging map and the per-lane patch-row offsets of a block of geometry GG
    auto index_setup = [&](auto geom) {
      using GG = decltype(geom);
  #pragma unroll
      for (int q = 0; q < WNLD; ++q) {
        const int e = t + q * NTH;
        const int pix = e / (WKC / 4), cq = e % (WKC / 4);
        const int py = pix / GG::RW, px = pix % GG::RW;
        const int iy = phy + d * (oy0 + py), ix = phx + d * (ox0 + px);
        const bool ok = pix < GG::PIXELS && oy0 + py >= 0 && ox0 + px >= 0 && iy < H && ix < W;
        gofs[q] = ok ? (unsigned)(iy * p.x_row_stride + ix * C + cq * 4) * 4u : kOOB;
        sofs[q] = (pix < GG::PIXELS ? py * GG::PITCH + px * WPSTR + cq * 4 : GG::STAGE - 8 + (t & 1) * 4) >> 2;  // in float4 units (past the block: the dump slot)
      }
      // (a fragment row without a tile reads the last tile's patch: in range, a broadcast, and kept out of the stores below)
      const int qt = GG::NT < 16 ? min(lane & 15, GG::NT - 1) : lane & 15;
      const int r = qt / GG::FC, c = GG::fcol(tf) + qt % GG::FC;
      ofs_a = (2 * (GG::frow(tf) + r) + ra) * GG::PITCH + 2 * c * WPSTR + kg * 4;
      ofs_b = (2 * (GG::frow(tf) + r) + rb) * GG::PITCH + 2 * c * WPSTR + kg * 4;
    };
    if (in_b)
      index_setup(WinoG56{});
    else
      index_setup(WinoG48{});
    __builtin_assume((ofs_a & 3) == 0 && (ofs_b & 3) == 0);  // (every term is a multiple of 4 floats; behind the select the compiler no longer sees it, and would split the 16-byte LDS reads)
  }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned uvo = ((unsigned)((nt * 4 + i) * (C / 16)) * (4 * 64 * 4) + (unsigned)lane * 4u) * 4u;  // bytes (< 2 GiB: wino_eligible)
  // Registers are kept to 110 per wave on purpose: four waves per SIMD = two workgroups per CU (this kernel's, or one of
  // the gather-GEMM's), which is what lets forwards in flight share a CU; LDS reads are therefore issued right before
  // their use (the other resident waves hide their latency) and only the filter fragments run one sub-step ahead.
  f32x4 g[WNLD], b[2][4], da[4], db[4];
  auto gload = [&](int K) {
#pragma unroll
    for (int q = 0; q < WNLD; ++q) g[q] = dc_bload4(xr, gofs[q], (unsigned)(K * WKC * 4));
  };
  // (the stage is indexed in 16-byte units: the compiler cannot prove the alignment of a float index and would split every store
  // into two ds_write2_b32, whose lanes — 16 bytes apart — collide four ways on the 32 write banks)
  auto sstore = [&](int buf) {
#pragma unroll
    for (int q = 0; q < WNLD; ++q) reinterpret_cast<f32x4*>(&stage[buf][0])[sofs[q]] = g[q];
  };
  auto bload = [&](int slot, int k16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) b[slot][j] = dc_bload4(ur, uvo + (unsigned)j * 1024u, (unsigned)k16 * 4096u);
  };
  auto lread = [&](int buf, int h) {
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      da[c4] = *reinterpret_cast<const f32x4*>(&stage[buf][ofs_a + c4 * WPSTR + h * 16]);
      db[c4] = *reinterpret_cast<const f32x4*>(&stage[buf][ofs_b + c4 * WPSTR + h * 16]);
    }
  };
  auto compute = [&](int bslot) {
    f32x2 tl[4], th[4];
    const f32x2 sb2 = {sb, sb};
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      tl[c4] = wlo(da[c4]) + sb2 * wlo(db[c4]);
      th[c4] = whi(da[c4]) + sb2 * whi(db[c4]);
    }
    f32x2 vl[4], vh[4];
    vl[0] = tl[0] - tl[2], vh[0] = th[0] - th[2];
    vl[1] = tl[1] + tl[2], vh[1] = th[1] + th[2];
    vl[2] = tl[2] - tl[1], vh[2] = th[2] - th[1];
    vl[3] = tl[1] - tl[3], vh[3] = th[1] - th[3];
    // four independent accumulators between two MFMAs on the same one (a dependent 8-pass MFMA would need s_nops)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vl[j][0], b[bslot][j][0], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vl[j][1], b[bslot][j][1], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vh[j][0], b[bslot][j][2], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vh[j][1], b[bslot][j][3], acc[j], 0, 0, 0);
  };
  const int NS = C / WKC;
  // the epilogue's per-channel constants are requested here (two registers carried through the K loop) instead of behind it,
  // where their round trip was exposed
  const int co = nt * WBN + (lane & 15);
  const float sc = p.scale ? p.scale[co] : 1.f, sh = p.shift ? p.shift[co] : 0.f;
  stamp(1);
  // pipeline: global -> registers (3 steps ahead) -> LDS ring of 3 (2 steps ahead) -> MFMA; filters one sub-step ahead
  // the first two stages are requested together (a second register set, dead after the prologue) so that their
  // latencies overlap instead of adding up
  f32x4 g1[WNLD];
  gload(0);
  bload(0, grp);
  if (NS > 1) {
#pragma unroll
    for (int q = 0; q < WNLD; ++q) g1[q] = dc_bload4(xr, gofs[q], (unsigned)(WKC * 4));
  }
  stamp(2);
  sstore(0);
  if (NS > 2) gload(2);
  if (NS > 1) {
#pragma unroll
    for (int q = 0; q < WNLD; ++q) reinterpret_cast<f32x4*>(&stage[1][0])[sofs[q]] = g1[q];
  }
  stamp(3);
  if constexpr (NG == 1) {
    // one staged step: U = K % 3 is a compile-time constant so that the ring buffer offsets fold into the instructions
    auto step = [&](int K, auto u_tag) {
      constexpr int U = decltype(u_tag)::value;
      __syncthreads();  // buffers <= K+1 are complete; buffer (K+2)%3 is free
      lread(U, 0);
      bload(1, 2 * K + 1);
      compute(0);
      if (K + 2 < NS) sstore((U + 2) % 3);
      lread(U, 1);
      bload(0, 2 * K + 2 < 2 * NS ? 2 * K + 2 : 0);  // the tail load is a harmless re-read of step 0
      compute(1);
      if (K + 3 < NS) gload(K + 3);
    };
    for (int K0 = 0; K0 < NS; K0 += 3) {
      step(K0, std::integral_constant<int, 0>{});
      if (K0 + 1 < NS) step(K0 + 1, std::integral_constant<int, 1>{});
      if (K0 + 2 < NS) step(K0 + 2, std::integral_constant<int, 2>{});
    }
  } else {
    // group g computes sub-step g of every staged step; U = K % 3 (ring slot) and S = K % 2 (filter-fragment slot) are
    // compile-time constants: six steps per round of the loop
    auto step = [&](int K, auto u_tag, auto s_tag) {
      constexpr int U = decltype(u_tag)::value, S = decltype(s_tag)::value;
      __syncthreads();
      lread(U, grp);
      bload(S ^ 1, K + 1 < NS ? 2 * (K + 1) + grp : 0);  // the tail load is a harmless re-read of step 0
      compute(S);
      if (K + 2 < NS) sstore((U + 2) % 3);
      if (K + 3 < NS) gload(K + 3);
    };
    for (int K0 = 0; K0 < NS; K0 += 6) {
      step(K0, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
      if (K0 + 1 < NS) step(K0 + 1, std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
      if (K0 + 2 < NS) step(K0 + 2, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
      if (K0 + 3 < NS) step(K0 + 3, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
      if (K0 + 4 < NS) step(K0 + 4, std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
      if (K0 + 5 < NS) step(K0 + 5, std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{});
    }
  }
  stamp(4);
  // inverse transform: over j in registers (P[b] = sum_j M[i][j] A[j][b]), over i (and the two wave groups) through LDS
  __syncthreads();  // every wave is done reading the staging ring, which the partials now overwrite
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    part[grp][i][0][tf][r4][lane] = acc[0][r4] + acc[1][r4] + acc[2][r4];
    part[grp][i][1][tf][r4][lane] = acc[1][r4] - acc[2][r4] - acc[3][r4];
  }
  __syncthreads();
  stamp(5);
  const int a = (wave >> 1) & 1, bq = wave & 1;  // this wave finalises output pixel (a, bq) of the tiles of fragment tf
  float* yb = reinterpret_cast<float*>(p.y);
  const float* rbp = reinterpret_cast<const float*>(p.resid);
  stamp(6);
  // NG = 2: the sixteen waves split the four accumulator rows (group g finalises rows 2g, 2g+1) and add the two groups' partial
  // sums, group 0's first: the order of every sum is fixed, the result does not depend on which wave arrives when
#pragma unroll
  for (int rr = 0; rr < 4 / NG; ++rr) {
    const int r4 = NG == 1 ? rr : 2 * grp + rr;
    float p0 = part[0][0][bq][tf][r4][lane], p1 = part[0][1][bq][tf][r4][lane], p2 = part[0][2][bq][tf][r4][lane], p3 = part[0][3][bq][tf][r4][lane];
    if constexpr (NG == 2) {
      p0 += part[NG - 1][0][bq][tf][r4][lane], p1 += part[NG - 1][1][bq][tf][r4][lane];
      p2 += part[NG - 1][2][bq][tf][r4][lane], p3 += part[NG - 1][3][bq][tf][r4][lane];
    }
    float v = a == 0 ? p0 + p1 + p2 : p1 - p2 - p3;
    const int q = 4 * (lane >> 4) + r4;  // D layout: row (tile in fragment) = 4*(lane/16) + r, col (channel) = lane%16
    int ty, tx;
    bool has_tile;
    auto tile_of = [&](auto geom) {
      using GG = decltype(geom);
      ty = rty0 + by * GG::BTY + GG::frow(tf) + q / GG::FC, tx = rtx0 + bx * GG::BTX + GG::fcol(tf) + q % GG::FC;
      has_tile = GG::NT == 16 || q < GG::NT;
    };
    if constexpr (G::MIX) {
      if (in_b)
        tile_of(WinoG56{});
      else
        tile_of(WinoG48{});
    } else {
      tile_of(G{});
    }
    const int oy = phy + d * (2 * ty + a), ox = phx + d * (2 * tx + bq);
    if (has_tile && oy < p.OH && ox < p.OW) {
      const long off = (long)n * p.y_img_stride + (long)oy * p.y_row_stride + (long)ox * p.y_pix_stride + co;
      v = v * sc + sh;
      if (rbp) v += rbp[off];
      if (p.relu) v = fmaxf(v, 0.f);
      yb[off] = v;
    }
  }
  stamp(7);
}

bool wino_same3x3(const ConvGemmParams& p) {
  const int d = p.ddy;  // dilation (1 or more), the same along x and y, with pad = dilation ("same" convolution)
  if (p.nty != 3 || p.ntx != 3 || p.sy != 1 || d < 1 || d > 4 || p.dy0 != -d) return false;
  const int C = p.klen;
  if (C <= 0) return false;
  if (p.sx != C || p.ddx != d * C || p.x0 != -d * C) return false;        // stride 1, dilation d, pad d along x
  if (p.x_rowlen % C != 0 || p.x_row_stride != p.x_rowlen) return false;  // dense NHWC rows of C channels
  return p.OH == p.x_rows && p.OW == p.x_rowlen / C;                      // "same" convolution
}

ConvGemmParams wino_launch_params(const ConvGemmParams& p, long grid, int bty, int btx, int blocks_per_wg) {
  ConvGemmParams q = p;
  q.xcd_on = xcd_map_on() && grid >= 16;
  const int d = p.ddy;
  q.w_TY = ((p.OH + d - 1) / d + 1) / 2, q.w_TX = ((p.OW + d - 1) / d + 1) / 2;
  q.w_NBY = (q.w_TY + bty - 1) / bty, q.w_NBX = (q.w_TX + btx - 1) / btx;
  q.w_nblk = p.NB * d * d * q.w_NBY * q.w_NBX;
  dc_magic((unsigned)((q.w_nblk + blocks_per_wg - 1) / blocks_per_wg), q.w_div_nblk);
  dc_magic((unsigned)(q.w_NBY * q.w_NBX), q.w_div_nbyx);
  dc_magic((unsigned)(d * d), q.w_div_dd);
  dc_magic((unsigned)d, q.w_div_d);
  dc_magic((unsigned)q.w_NBX, q.w_div_nbx);
  return q;
}

bool wino_eligible(const ConvGemmParams& p) {
  if (p.esize != 4 || !wino_same3x3(p)) return false;
  const int C = p.klen;
  if (C % WKC != 0 || p.Cout % WBN != 0 || p.sigmoid_ch != 0) return false;
  // 32-bit byte offsets (buffer addressing): one image of the input and the packed filter image stay below 2 GiB
  if ((long long)p.x_rows * p.x_row_stride * 4 >= 0x7fffffffLL || (long long)wino_packed_floats(p.Cout, C) * 4 >= 0x7fffffffLL) return false;
  return true;
}

long wino_blocks(int TY, int TX, int bty, int btx) { return (long)((TY + bty - 1) / bty) * ((TX + btx - 1) / btx); }

template <class G>
static long wino_grid_of(const ConvGemmParams& p) {
  const int d = p.ddy;
  const int TY = ((p.OH + d - 1) / d + 1) / 2, TX = ((p.OW + d - 1) / d + 1) / 2;
  return (long)p.NB * d * d * wino_blocks(TY, TX, G::BTY, G::BTX) * (p.Cout / WBN);
}
long wino_grid(const ConvGemmParams& p) { return wino_grid_of<WinoG48>(p); }
long wino_grid_5x6(const ConvGemmParams& p) { return wino_grid_of<WinoG56>(p); }

// the 5 x 6 forms enter the per-shape timing only where they need strictly fewer workgroups than the 4 x 8 ones (at 544x736: the dilated
// res5 layers, 9 x 12 tiles per phase image: 4 blocks against 6; res4 takes 16 against 15, res3 56 against 54, res2 224 against 204): the
// other Winograd layers keep their tuning time.  set_tile takes them wherever the kernel is eligible.  (The tune signature, Net::tune_key, does
// not carry the dilation: two 3x3 layers of one net that differ in nothing but their dilation share a signature, the first of them in the plan
// decides whether the 5 x 6 forms are timed for both, and both run the form chosen — correct on either, the kernel is general; no such pair
// exists in the ResNet nets this library lowers.)
bool wino_fewer_blocks(const ConvGemmParams& p) { return wino_grid_of<WinoG56>(p) < wino_grid_of<WinoG48>(p); }

// The cover of the mixed forms: ONE straight cut of the TY x TX tile grid, region A (rows or columns in front of the cut) on 4 x 8 blocks,
// region B (from the cut on) on 5 x 6 blocks, either of them possibly empty; fewest blocks; on a tie a pure cover before a cut one (a 9 x 12
// grid keeps its four 5 x 6 blocks although 2 + 2 blocks would do), then fewest 5 x 6 blocks, then the horizontal cut, then the smaller one.
// Which side gets which geometry is no choice of its own: the block count of a cut at `a` with the sides swapped
// is that of the cut at (extent - a).  A cut inside a 4 x 8 block would make region A's last blocks overhang region B; a cut on the next
// multiple of the block's extent needs no more blocks, so only those (and the grid's far edge: the pure 4 x 8 cover) are candidates.
WinoCover wino_plan_cover(int TY, int TX) {
  WinoCover best{};
  best.blocks = -1;
  for (int vertical = 0; vertical < 2; ++vertical) {
    const int ext = vertical ? TX : TY, step = vertical ? WinoG48::BTX : WinoG48::BTY;
    for (int cut = 0; cut <= ext; cut = cut == ext ? ext + 1 : std::min(cut + step, ext)) {
      WinoCover c{};
      c.vertical = vertical, c.cut = cut;
      const int aty = vertical ? TY : cut, atx = vertical ? cut : TX, bty = vertical ? TY : TY - cut, btx = vertical ? TX - cut : TX;
      if (aty > 0 && atx > 0) c.a_nby = (aty + WinoG48::BTY - 1) / WinoG48::BTY, c.a_nbx = (atx + WinoG48::BTX - 1) / WinoG48::BTX;
      if (bty > 0 && btx > 0) c.b_nby = (bty + WinoG56::BTY - 1) / WinoG56::BTY, c.b_nbx = (btx + WinoG56::BTX - 1) / WinoG56::BTX;
      c.na = c.a_nby * c.a_nbx, c.nb = c.b_nby * c.b_nbx, c.blocks = c.na + c.nb;
      c.b_ty0 = vertical ? 0 : cut, c.b_tx0 = vertical ? cut : 0;
      const bool is_cut = c.na > 0 && c.nb > 0, best_cut = best.na > 0 && best.nb > 0;
      if (best.blocks < 0 || c.blocks < best.blocks || (c.blocks == best.blocks && (is_cut < best_cut || (is_cut == best_cut && c.nb < best.nb)))) best = c;
    }
  }
  return best;
}
static long wino_mix_grid_tiles(const ConvGemmParams& p, int& TY, int& TX) {
  const int d = p.ddy;
  TY = ((p.OH + d - 1) / d + 1) / 2, TX = ((p.OW + d - 1) / d + 1) / 2;
  return (long)p.NB * d * d * wino_plan_cover(TY, TX).blocks * (p.Cout / WBN);
}
long wino_grid_mix(const ConvGemmParams& p) {
  int TY, TX;
  return wino_mix_grid_tiles(p, TY, TX);
}
// the mixed forms enter the per-shape timing where their cover needs strictly fewer blocks than both pure ones (at 544x736: res4 13 against
// 15 / 16, res3 52 against 54 / 56, res2 198, by a vertical cut, against 204 / 224; the dilated res5 phase images keep the pure 5 x 6 cover) ...
bool wino_mix_offered(int TY, int TX) {
  return wino_plan_cover(TY, TX).blocks < std::min(wino_blocks(TY, TX, WinoG48::BTY, WinoG48::BTX), wino_blocks(TY, TX, WinoG56::BTY, WinoG56::BTX));
}
// ... and the launch is large enough for workgroups to matter: `images` (phase) images of TY x TX tiles and Cout output channels on 4 x 8 blocks
// are at least kWinoMixMinWorkgroups workgroups, half of the 256 CUs.  A smaller launch leaves most of the chip's workgroup slots free with
// either cover, its time is one workgroup's, alone and with neighbours in flight: what a shorter grid frees there nobody waits for, and the two
// extra candidates would only lengthen the tuning of every small shape (a 72 x 104 image's res2 layers: 9 x 13 tiles, 5 blocks against 6, 24
// workgroups).  The smallest launches of the benchmark shape that are offered: res4, 240 workgroups.  (128 comes from this argument about
// workgroup slots, not from a measurement: no launch between 24 and 240 workgroups was timed on the mixed forms.)
constexpr long kWinoMixMinWorkgroups = 128;
bool wino_mix_offered_launch(int TY, int TX, long images, int Cout) {
  return wino_mix_offered(TY, TX) && images * wino_blocks(TY, TX, WinoG48::BTY, WinoG48::BTX) * (Cout / WBN) >= kWinoMixMinWorkgroups;
}
bool wino_mix_fewer_blocks(const ConvGemmParams& p) {
  int TY, TX;
  return wino_mix_grid_tiles(p, TY, TX) > 0 && wino_mix_offered_launch(TY, TX, (long)p.NB * p.ddy * p.ddy, p.Cout);
}

size_t wino_packed_floats(int Cout, int Cin) { return (size_t)16 * Cout * Cin; }

void wino_pack_filters(const float* g, int Cout, int Cin, float* out) {
  static const double G[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci) {
      const float* w = g + ((size_t)co * Cin + ci) * 9;
      double tmp[4][3], U[4][4];
      for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 3; ++b) tmp[a][b] = G[a][0] * w[b] + G[a][1] * w[3 + b] + G[a][2] * w[6 + b];
      for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) U[a][b] = tmp[a][0] * G[b][0] + tmp[a][1] * G[b][1] + tmp[a][2] * G[b][2];
      const int nt = co / 16, col = co % 16, k16 = ci / 16, kg = (ci % 16) / 4, s = ci % 4;
      const int lane = kg * 16 + col;
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
          out[(((((size_t)nt * 4 + i) * (Cin / 16) + k16) * 4 + j) * 64 + lane) * 4 + s] = (float)U[i][j];
    }
}

// NG = 1: wino_f23 (8 waves per workgroup), 2: wino_f23_w16 (16); G: the block geometry (4 x 8, or 5 x 6: wino_f23_5x6, wino_f23_5x6_w16; both: below)
template <int NG, class G>
static int launch_wino_f23(const ConvGemmParams& p, void* stream) {
  if (p.esize != 4 || !wino_eligible(p)) return (int)hipErrorInvalidValue;
  const long grid = wino_grid_of<G>(p);
  if (grid <= 0) return 0;
  if (grid > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((wino_f23_kernel<NG, G>), dim3((unsigned)grid), dim3(NG * WNTH), 0, (hipStream_t)stream, wino_launch_params(p, grid, G::BTY, G::BTX, 1));
  return (int)hipGetLastError();
}
int launch_wino_f23(const ConvGemmParams& p, void* stream) { return launch_wino_f23<1, WinoG48>(p, stream); }
int launch_wino_f23_w16(const ConvGemmParams& p, void* stream) { return launch_wino_f23<2, WinoG48>(p, stream); }
int launch_wino_f23_5x6(const ConvGemmParams& p, void* stream) { return launch_wino_f23<1, WinoG56>(p, stream); }
int launch_wino_f23_5x6_w16(const ConvGemmParams& p, void* stream) { return launch_wino_f23<2, WinoG56>(p, stream); }

// the mixed forms: region A's block grid in w_NBY / w_NBX / w_div_nbx as the 4 x 8 forms have it, region B's in w_mix_*
template <int NG>
static int launch_wino_f23_mix(const ConvGemmParams& p, void* stream) {
  if (p.esize != 4 || !wino_eligible(p)) return (int)hipErrorInvalidValue;
  int TY, TX;
  const long grid = wino_mix_grid_tiles(p, TY, TX);
  if (grid <= 0) return 0;
  if (grid > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const WinoCover c = wino_plan_cover(TY, TX);
  ConvGemmParams q = wino_launch_params(p, grid, WinoG48::BTY, WinoG48::BTX, 1);
  q.w_NBY = c.a_nby, q.w_NBX = c.a_nbx;
  q.w_nblk = p.NB * p.ddy * p.ddy * c.blocks;
  q.w_mix_na = c.na, q.w_mix_nab = c.blocks, q.w_mix_ty0 = c.b_ty0, q.w_mix_tx0 = c.b_tx0, q.w_mix_NBX = c.b_nbx;
  dc_magic((unsigned)q.w_nblk, q.w_div_nblk);
  dc_magic((unsigned)c.blocks, q.w_div_nbyx);
  dc_magic((unsigned)c.a_nbx, q.w_div_nbx);
  dc_magic((unsigned)c.b_nbx, q.w_mix_div_nbx);
  hipLaunchKernelGGL((wino_f23_kernel<NG, WinoGMix>), dim3((unsigned)grid), dim3(NG * WNTH), 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}
int launch_wino_f23_mix(const ConvGemmParams& p, void* stream) { return launch_wino_f23_mix<1>(p, stream); }
int launch_wino_f23_mix_w16(const ConvGemmParams& p, void* stream) { return launch_wino_f23_mix<2>(p, stream); }

long wino_form_blocks(int variant, int TY, int TX) {
  if (variant == kWinoVariant || variant == kWinoVariant16) return wino_blocks(TY, TX, WinoG48::BTY, WinoG48::BTX);
  if (variant == kWinoVariant56 || variant == kWinoVariant56x16) return wino_blocks(TY, TX, WinoG56::BTY, WinoG56::BTX);
  if (variant == kWinoVariantMix || variant == kWinoVariantMix16) return wino_plan_cover(TY, TX).blocks;
  return -1;
}

}  // namespace dc
