// kernels.h — launch interface of the gfx950 kernels (the .hip sources and conv_gemm.cpp, forms.cpp).  Plain structs, no HIP types
// in the signatures except the opaque stream, so the graph runtime (net_*.cpp) stays host-only C++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace dc {

constexpr int kMaxTaps = 32;  // tap-validity masks are one 32-bit word per staged row

// magic {multiplier, shift word} of n / d for 0 <= n < 2^31 and a divisor known on the host (the device divides with dc_fastdiv,
// kernel_prims.h): sh = 31 + ceil(log2 d), mul = floor(2^sh / d) + 1, n / d = (n * mul) >> sh; d <= 1 sets bit 31 of the shift word
void dc_magic(unsigned d, unsigned (&mg)[2]);
// DC_XCD_MAP (on unless set to 0, read once): the per-XCD tile map of the single-problem gather-GEMM launches and of the Winograd forms
bool xcd_map_on();

// element kind of the device images (the values of DC_OPT_DTYPE): float32, float16, bfloat16.  Host tensors, the per-channel
// affine vectors and every accumulation are float in all three.
enum ElemKind { kElemF32 = 0, kElemF16 = 1, kElemBF16 = 2 };
inline int elem_kind_size(int kind) { return kind == kElemF32 ? 4 : 2; }
inline const char* elem_kind_name(int kind) { return kind == kElemF16 ? "f16" : kind == kElemBF16 ? "bf16" : "f32"; }

// out[pixel][co] = act( (sum_k A[pixel][k] * W[co][k]) * scale[co] + shift[co] (+ resid[pixel][co]) )
//   pixel = (n, oy, ox) over an NB x OH x OW grid,
//   A[pixel][.] = concatenation over a (nty x ntx) grid of TAPS of `klen` consecutive floats of source row
//                 oy*sy + dy0 + ty*ddy, starting at element ox*sx + x0 + tx*ddx  (0 outside the row/image),
//   W packed [Cout][Ktot] with k contiguous, taps in (ty, tx) order (Ktot = nty*ntx*klen).
// Covers every Convolution of the path (1x1, 1x1 stride 2, 3x3, dilated 3x3, the 7x7 stem seen as
// 7 row-taps of 8 NHWC4 pixels) and, per output-parity class, the stride-2 Deconvolution heads.
// The tap grid is arithmetic so the kernel advances it with scalar adds (no table loads in the K loop).
constexpr int kMaxClasses = 4;
// One output-residue class of a strided Deconvolution inside a MULTI-CLASS launch: the classes of a stride-s transposed
// convolution are s*s ordinary gather-GEMMs over the same input that differ only in tap grid, K, filter image and the
// interleaved output pixels they own, so they run as ONE launch (class = a range of the grid, heaviest class first so
// that its workgroups start first).  Fields mean what the same-named ConvGemmParams fields mean.
struct ConvClass {
  int nty, ntx, dy0, ddy, x0, ddx, Ktot, x_bias;
  int OH, OW, M;
  int tiles_m;          // m tiles of the class (filled by launch_conv_gemm)
  unsigned div_ohw[2];  // (filled by launch_conv_gemm)
  unsigned div_ow[2];
  long w_off;           // element offset of the class's filter image inside `w`
  long y_off;           // element offset of the class's first output inside `y` (and `resid`)
};

// MULTI-PROBLEM launches (round 4): the SAME layer over several tensors in one launch — the four scales of an image pyramid
// (python/pose/estimate_pose.py:81-128 runs them as four forwards; base_conv_layer.cpp:326-341 as one SGEMM per image), the
// crops of a crowd image, and, inside each of them, the residue classes of a strided deconvolution.  Filters, epilogue
// constants, klen, sy/sx, Cout are the layer's and stay in ConvGemmParams; everything that depends on a tensor's shape or
// address is per problem.  The table travels in the kernel arguments (ConvMultiArgs): filters are pulled through the L2s once
// per layer instead of once per scale, one dispatch ramp and one tail per layer instead of four.
constexpr int kMaxProblems = 16;
struct ConvProblem {
  const void* x;
  void* y;            // pre-offset to the first output element of the problem
  const void* resid;  // same addressing as y, or null (all problems of a launch alike)
  long x_img_stride, y_img_stride;
  long w_off;         // element offset of the problem's filter image inside `w` (deconvolution classes)
  int x_row_stride, x_rows, x_rowlen;
  int nty, ntx, dy0, ddy, x0, ddx, Ktot, x_bias;
  int OH, OW, M;
  int tiles_m;          // (filled by prepare_conv_multi)
  unsigned div_ohw[2];  // (filled)
  unsigned div_ow[2];   // (filled)
  int y_row_stride, y_pix_stride;
  int dense_x, dense_y;  // (filled) as ConvGemmParams::dense_x / dense_y
  int NB;
  int pad_;
};
struct ConvMultiTable {
  // XCD row qy of the (1 << mc_lgx) x (8 >> mc_lgx) arrangement walks, of EVERY problem k in turn, the m tiles
  // [tiles_m[k]*qy/gy, tiles_m[k]*(qy+1)/gy): end[qy][k] = m tiles of problems 0..k in that walk (INT_MAX past the last
  // problem), so a workgroup finds its problem with 16 scalar compares on one 64-byte line
  int end[8][kMaxProblems];
  ConvProblem prob[kMaxProblems];
};

struct ConvGemmParams {
  int esize;          // bytes per activation / filter element: 4 (float) or 2 (_Float16 / __bf16); strides are in elements
  const void* x;
  long x_img_stride;  // elements between images
  int x_row_stride;   // elements between rows
  int x_rows;         // H of the source
  int x_rowlen;       // valid elements in a row (W*C)
  int sy, sx;         // source step per output pixel: rows / elements
  int nty, ntx;       // tap grid
  int dy0, ddy;       // source-row offset of tap row ty: dy0 + ty*ddy
  int x0, ddx;        // element offset of tap column tx: x0 + tx*ddx
  int klen;           // K elements per tap (multiple of the variant's BK)
  int x_bias;         // min over taps of (dy*x_row_stride + xoff) (<= 0); filled by launch_conv_gemm
  const void* w;
  int Ktot;
  int NB, OH, OW;
  int M;  // NB*OH*OW
  int Cout;
  void* y;  // pre-offset to the first output element of this launch
  long y_img_stride;
  int y_row_stride;  // elements per oy step
  int y_pix_stride;  // elements per ox step
  const void* resid;  // same addressing as y (may alias y), or null
  const float* scale;  // [Cout] or null (=1)
  const float* shift;  // [Cout] or null (=0)
  int relu;
  int sigmoid_ch;  // channels [0, sigmoid_ch) get the logistic
  // --- filled by launch_conv_gemm (host-side precomputation keeps integer divisions out of the prologue) ---
  int xcd_on;              // XCD-aware tile map in use
  int xcd_lgx;             // the 8 XCDs form a (1 << xcd_lgx) x (8 >> xcd_lgx) arrangement over (n tiles) x (m tiles): XCD (qx, qy)
                           // owns n tiles [tn*qx/gx, tn*(qx+1)/gx) and m tiles [tm*qy/gy, tm*(qy+1)/gy) — computed with shifts in
                           // the kernel (a per-XCD table in the argument block cost every workgroup a second, dependent
                           // kernel-argument fetch: ~0.5 us before its first useful instruction)
  int tiles_m;
  unsigned div_rw[2][2];   // magic numbers for a division by the rectangle width: floor(tn/gx) and that + 1
  unsigned div_ohw[2];     // magic {multiplier, shift} for m / (OH*OW)
  unsigned div_ow[2];      // ... for m / OW
  unsigned div_tn[2];      // ... for block / tiles_n (linear map)
  int tiles_n;
  long long* dbg;  // optional [grid][4 waves][6] device timestamps (DC_DEBUG_TIMING), else null
  // --- multi-class launches (the stride-2 deconvolution heads): ncls > 1 and cls[0..ncls) replace the single-problem
  //     fields nty..x_bias / Ktot / OH / OW / M above; sy, sx, klen, strides, Cout, epilogue are common to all classes
  // --- Winograd launches (filled by the wino_f23 launch): tile-grid geometry and the magic numbers of its divisions
  int w_TY, w_TX, w_NBY, w_NBX, w_nblk;
  unsigned w_div_nblk[2], w_div_nbyx[2], w_div_dd[2], w_div_d[2], w_div_nbx[2];
  int wide_epi;  // (filled by launch_conv_gemm) float16: 16-byte epilogue through LDS — Cout and the output strides are multiples of 8
  int vec_epi;   // (filled) 16-byte output vectors are legal: Cout, the output strides and the bases are multiples of 16 bytes, no sigmoid
  int dense_x;   // (filled) 1x1 / stride-1 layer over a dense NHWC tensor: output pixel m reads the klen elements at m * sx (no decode)
  int dense_y;   // (filled) the output pixels are dense: pixel m is written at m * y_pix_stride
  int ncls;
  int mc_lgx;  // multi-class tile map: the 8 XCDs form a (1 << mc_lgx) x (8 >> mc_lgx) grid over (n tiles) x (m tiles of every class)
  // --- mixed Winograd launches (wino_f23_mix: blocks of two geometries, wino_plan_cover): per phase image, blocks [0, w_mix_na) are region A,
  //     4 x 8 tiles from the grid's origin on the w_NBY x w_NBX grid above; blocks [w_mix_na, w_mix_nab) are region B, 5 x 6 tiles from tile
  //     (w_mix_ty0, w_mix_tx0), w_mix_NBX of them per block row.  One 64-byte line of its own (bytes 0x140-0x17f of the block, asserted below;
  //     w_mix_pad_ fills line 0x100 up): the kernel requests it at entry with the other lines, and every other field keeps its place in its line.
  int w_mix_pad_;
  int w_mix_na, w_mix_nab, w_mix_ty0, w_mix_tx0, w_mix_NBX;
  unsigned w_mix_div_nbx[2];
  int w_mix_reserved0_;
  void* form_ws;  // the executor's V / M workspace of the wino_f43 form (Net::wino43_dev_: 36 R (Cin + Cout) floats); null for every other form
  int w_mix_reserved_[6];
  ConvClass cls[kMaxClasses];
  // --- multi-problem launches: nprob > 0 and the ConvMultiTable that follows the block in the kernel arguments
  //     (ConvMultiArgs) replace every per-tensor field above
  int nprob;
  int ekind;  // ElemKind of x / w / y / resid (esize alone does not tell float16 from bfloat16)
};
static_assert(offsetof(ConvGemmParams, form_ws) == offsetof(ConvGemmParams, w_mix_na) + 32 &&
                  offsetof(ConvGemmParams, w_mix_na) % 64 == 0 && offsetof(ConvGemmParams, w_mix_div_nbx) + 8 <= offsetof(ConvGemmParams, w_mix_na) + 64 &&
                  offsetof(ConvGemmParams, cls) == offsetof(ConvGemmParams, w_mix_na) + 64,
              "the w_mix_* fields are one 64-byte line of the argument block, the multi-class table starts on the next");
// kernel arguments of a multi-problem launch: the table travels IN the argument block (3.6 KB of the 4 KB a HIP kernel may
// take), so a workgroup finds its problem with scalar loads from the same segment as everything else — with the table behind
// a pointer in device memory every workgroup paid one more dependent round trip (argument block -> table row -> problem)
// before its first useful instruction, ~5 % of a batch-8 float16 forward
struct ConvMultiArgs {
  ConvGemmParams p;
  ConvMultiTable t;
};
static_assert(sizeof(ConvMultiArgs) <= 4096, "HIP kernel arguments are limited to 4 KB");

// Tile variants of conv_gemm.  BM x BN output tile per 256-thread workgroup, 4 waves arranged
// WR x WC x WK (WK = waves splitting the K range of the same output tile, reduced through LDS).
struct ConvVariant {
  const char* name;
  int BM, BN, WR, WC, WK;
};
int conv_num_variants();
const ConvVariant& conv_variant(int i);
// workgroups this variant launches for the problem
int conv_variant_bk(int i);
int conv_variant_esize(int i);
// The bfloat16 tiles are a table of their own (v_mfma_f32_32x32x16_bf16): tile i of it is variant kBf16Variant0 + i wherever a
// variant number travels (Launch::variant, tune caches by name); conv_variant* above answer for those numbers too.
constexpr int kBf16Variant0 = 2000;
int conv_num_bf16_variants();
inline bool is_bf16_variant(int v) { return v >= kBf16Variant0 && v < kBf16Variant0 + conv_num_bf16_variants(); }
int conv_variant_ekind(int v);
bool conv_variant_exists(int v);  // a gather-GEMM tile of either table
// every tile variant of one element kind, in table order (the candidates of a launch before its K and class checks)
const int* conv_variants_of(int ekind, int* count);
int conv_variant_by_name(const char* name);  // -1: no gather-GEMM tile of that name
bool conv_variant_multiclass(int i);  // has a multi-class instantiation (ConvGemmParams::ncls > 1)
long conv_grid(const ConvGemmParams& p, int variant);
// returns hipError_t as int
int launch_conv_gemm(const ConvGemmParams& p, int variant, void* stream);
// Multi-problem launch, prepared once (host side): `p` carries the layer's common fields (esize, klen, sy, sx, w, Cout, scale,
// shift, relu, sigmoid_ch), `table.prob[0..nprob)` the per-tensor ones (pointers included).  Fills the derived fields of both
// (x_bias, magic numbers, tiles, dense / vector-epilogue flags, the XCD arrangement and table.end) and returns the grid, or
// -1 if this variant cannot take the launch.
long prepare_conv_multi(ConvGemmParams& p, ConvMultiTable& table, int nprob, int variant);
bool conv_variant_multiproblem(int i);
int launch_conv_multi(const ConvMultiArgs& a, int variant, long grid, void* stream);

// ---- Winograd F(2x2, 3x3) for the stride-1 3x3 convolutions of dilation d = pad (float32) --------------------------------
// Same ConvGemmParams as the gather-GEMM (x/y/resid/scale/shift/relu, NB, OH, OW, Cout, strides; klen = input channels,
// x_rows = H, x_rowlen = W*klen); `w` is the transformed-filter image made by wino_pack_filters().  Launched as the forms
// wino_f23 and wino_f23_w16 (conv_form below).
bool wino_eligible(const ConvGemmParams& p);   // geometry / type the kernel takes
// what both Winograd forms take: a 3x3 "same" convolution, stride 1, dilation d = pad (1..4) along y and x, dense NHWC rows of klen
// channels (each form adds its element kind, channel multiples, output alignment and 2 GiB limits)
bool wino_same3x3(const ConvGemmParams& p);
// `p` as a Winograd form launches it over `grid` workgroups: the per-XCD map (DC_XCD_MAP, grids of 16 or more), the geometry of the
// bty x btx tile blocks and the magic numbers of the kernel's block-index divisions, the first one by blocks_per_wg blocks at a time
ConvGemmParams wino_launch_params(const ConvGemmParams& p, long grid, int bty, int btx, int blocks_per_wg);
long wino_grid(const ConvGemmParams& p);                   // of the 4 x 8-tile forms
long wino_grid_5x6(const ConvGemmParams& p);               // of the 5 x 6-tile forms
bool wino_fewer_blocks(const ConvGemmParams& p);           // the 5 x 6 forms need strictly fewer workgroups: where they are offered to the autotuner
// the cover of a TY x TX tile grid by one straight cut: region A (rows [0, cut) of a horizontal cut, columns [0, cut) of a vertical one) as
// a_nby x a_nbx blocks of 4 x 8 tiles from the origin, region B (the rest) as b_nby x b_nbx blocks of 5 x 6 tiles from tile (b_ty0, b_tx0)
struct WinoCover {
  int vertical, cut, blocks, na, nb, a_nby, a_nbx, b_nby, b_nbx, b_ty0, b_tx0;
};
WinoCover wino_plan_cover(int TY, int TX);                 // fewest blocks, then a pure cover before a cut one, then fewest 5 x 6 blocks; either region may be empty
long wino_grid_mix(const ConvGemmParams& p);               // of the mixed forms
bool wino_mix_offered(int TY, int TX);                     // the mixed cover needs strictly fewer blocks than both pure ones ...
bool wino_mix_offered_launch(int TY, int TX, long images, int Cout);  // ... and `images` (phase) images x Cout channels are a launch of half the CUs or more ...
bool wino_mix_fewer_blocks(const ConvGemmParams& p);       // ... for this layer: where the mixed forms are offered to the autotuner
int launch_wino_f23_mix(const ConvGemmParams& p, void* stream);
int launch_wino_f23_mix_w16(const ConvGemmParams& p, void* stream);
// the four forms of one geometry: 8 or 16 (_w16) waves per workgroup, 4 x 8- or 5 x 6-tile blocks
int launch_wino_f23(const ConvGemmParams& p, void* stream);
int launch_wino_f23_w16(const ConvGemmParams& p, void* stream);
int launch_wino_f23_5x6(const ConvGemmParams& p, void* stream);
int launch_wino_f23_5x6_w16(const ConvGemmParams& p, void* stream);
long wino_blocks(int TY, int TX, int bty, int btx);        // bty x btx-tile blocks that cover a TY x TX tile grid
long wino_form_blocks(int variant, int TY, int TX);        // ... blocks of the float32 Winograd form `variant`; -1: not one
size_t wino_packed_floats(int Cout, int Cin);
// g: [Cout][Cin][3][3] (Caffe order) -> U = G g G^T per (co, ci), laid out so that one wave's B-operand load is 1 KB
// contiguous: [Cout/16][4 i][Cin/16][4 j][64 lanes][4]
void wino_pack_filters(const float* g, int Cout, int Cin, float* out);
// ---- the same for a float16 net (wino_f16.hip): `w` is the image made by wino_half_pack_filters() uploaded as _Float16, `scale`
// must carry the extra factors 4 (the staged pixels are pre-multiplied by 1/4) and row_scale[co]; no shortcut operand
bool wino_half_eligible(const ConvGemmParams& p);
long wino_half_grid(const ConvGemmParams& p);
size_t wino_half_packed_elems(int Cout, int Cin);
void wino_half_pack_filters(const float* g, int Cout, int Cin, bool rowscale, float* out, float* row_scale);
int launch_wino_half(const ConvGemmParams& p, void* stream);
// ---- the streaming form of the dense float16 1x1 / stride-1 layers (stream1x1.hip): filters resident in registers, the pixels walked in
// 32-pixel steps through an LDS-DMA ring.  `w` is the image made by stream1x1_pack_filters() uploaded as _Float16; x / y / resid / scale /
// shift / relu as the gather-GEMM (the epilogue is the same instruction sequence: bit-identical results)
bool stream1x1_eligible(const ConvGemmParams& p);
long stream1x1_grid(const ConvGemmParams& p);
size_t stream1x1_packed_elems(int Cout, int K);
void stream1x1_pack_filters(const float* g, int Cout, int K, float* out);
int launch_stream1x1(const ConvGemmParams& p, void* stream);
// ---- the float32 form (stream1x1_f32.hip): 16-pixel steps of v_mfma_f32_16x16x4_f32, one workgroup per CU (two at K <= 128); K = 64, 128, 256 or 512, Cout % 64 == 0
bool stream1x1f_eligible(const ConvGemmParams& p);
long stream1x1f_grid(const ConvGemmParams& p);
size_t stream1x1f_packed_elems(int Cout, int K);
void stream1x1f_pack_filters(const float* g, int Cout, int K, float* out);
int launch_stream1x1f(const ConvGemmParams& p, void* stream);
// ---- Winograd F(4x4, 3x3), float32, unfused ("wino_f43", wino43_f32.hip + the batched instantiation of the kernel above): the input transformed
// once per layer into V[36][R][Cin] (R = NB d d TY TX tiles of 4 x 4 output pixels on the dilation-phase grid), the 36 points multiplied as
// plain [R][Cin] x [Cin][Cout] products by ws1x1f_kernel<.., BATCH> into M[36][R][Cout], the inverse transform with the folded affine and
// ReLU.  V and M live in p.form_ws (wino43_workspace_bytes); `w` is the image made by wino43_pack_filters().  No shortcut operand.
bool wino43_eligible(const ConvGemmParams& p);
bool wino43_offered(const ConvGemmParams& p);   // where the per-shape timing tries it: kWino43MinTiles tiles or more
long wino43_tiles(const ConvGemmParams& p);     // R
long wino43_grid(const ConvGemmParams& p);      // workgroups of the multiply
size_t wino43_workspace_bytes(const ConvGemmParams& p);
size_t wino43_packed_floats(int Cout, int Cin);
// g: [Cout][Cin][3][3] -> U = G g G^T per (co, ci) in double, rounded once; point p = 6 i + j is the [Cout][Cin] matrix at out + p Cout Cin,
// in stream1x1f_pack_filters' order
void wino43_pack_filters(const float* g, int Cout, int Cin, float* out);
int launch_wino_f43(const ConvGemmParams& p, void* stream);
// the two transform kernels of wino43_f32.hip (R tiles; V / M as above)
int launch_wino43_input(const ConvGemmParams& p, float* V, long R, int TY, int TX, void* stream);
int launch_wino43_output(const ConvGemmParams& p, const float* M, long R, int TY, int TX, void* stream);
// the 36 products (stream1x1_f32.hip): M[p] = V[p] U[p], p = 0..35
long stream1x1f_batched_grid(long R, int Cin, int Cout);
int launch_stream1x1f_batched(const float* V, const float* U, float* M, long R, int Cin, int Cout, void* stream);
// ---- the float32 stem on the same skeleton ("ws7x7f"): conv1 7x7 / 2 over the NHWC4 image as the lowering's 7-row-tap launch describes it; a
// 1 KiB request gathers an output pixel's 7 x 8 input pixels (K = 224, the row-tap image's columns); `w` from stem_ws_pack_filters()
bool stem_ws_eligible(const ConvGemmParams& p);
long stem_ws_grid(const ConvGemmParams& p);
size_t stem_ws_packed_elems();
void stem_ws_pack_filters(const float* rowtap, float* out);  // rowtap: [64][224] = the row-tap image (k = ky 32 + kx 4 + ci)
int launch_stem_ws(const ConvGemmParams& p, void* stream);
// ---- the float16 stem (stem_f16.hip): conv1 7x7 / 2 over the NHWC4 image, as the lowering's 7-row-tap launch describes it (4 or 8 channels
// per pixel, at most 4 of them real); `w` is the image made by stem7x7_pack_filters(), uploaded as _Float16
bool stem7x7_eligible(const ConvGemmParams& p);
long stem7x7_grid(const ConvGemmParams& p);
size_t stem7x7_packed_elems();
void stem7x7_pack_filters(const float* g, int C, float* out);  // g: [64][C][7][7], C <= 4
int launch_stem7x7(const ConvGemmParams& p, void* stream);
// multi-problem (NetGroup): prepare_conv_multi / launch_conv_multi end here for the ws1x1 form; p.w must be the packed image
long stream1x1_prepare_multi(const ConvGemmParams& p, const ConvMultiTable& tb, int nprob);  // the grid, or -1
int launch_stream1x1_multi(const ConvMultiArgs& a, void* stream);                              // a.p.nprob, a.t as filled by the caller
// ---- the same two kernels for a bfloat16 net ("bs1x1", "bs7x7"): v_mfma_f32_32x32x16_bf16 on the same register images, the epilogue of the
// bfloat16 gather-GEMM (shortcut widened by a shift / a mask, added and ReLU'd in fp32, one rounding by v_cvt_pk_bf16_f32: bit-identical to a
// bf16 tile without split-K).  `w` is the image of stream1x1_pack_filters() / stem7x7_pack_filters() uploaded as __bf16 (no row scale)
bool stream1x1_bf16_eligible(const ConvGemmParams& p);
int launch_stream1x1_bf16(const ConvGemmParams& p, void* stream);
long stream1x1_bf16_prepare_multi(const ConvGemmParams& p, const ConvMultiTable& tb, int nprob);
int launch_stream1x1_bf16_multi(const ConvMultiArgs& a, void* stream);
bool stem7x7_bf16_eligible(const ConvGemmParams& p);
int launch_stem7x7_bf16(const ConvGemmParams& p, void* stream);

// ---- FORMS: the convolution kernels outside the tile tables.  A form has a filter image of its own (Launch::form_w) and is timed against
// the tiles per shape.  Its variant number travels in Launch::variant and tune caches like a tile's, and DC_CONV_VARIANT takes it.
constexpr int kWinoVariant = 1000;    // "wino_f23": Winograd F(2x2, 3x3), float32, 8 waves per workgroup (wino_f32.hip)
constexpr int kWinoVariant16 = 1001;  // "wino_f23_w16": its 16-wave form (launches of at most one workgroup per CU)
constexpr int kWinoHalf = 1002;       // "wino_h23": the float16 Winograd kernel (wino_f16.hip): fp16 operands, fp32 accumulate
constexpr int kStreamHalf = 1003;     // "ws1x1": the float16 streaming form of the dense 1x1 layers (stream1x1.hip)
constexpr int kStemHalf = 1004;       // "stem7x7": the float16 7x7 / stride-2 stem (stem_f16.hip)
constexpr int kStreamFloat = 1005;    // "ws1x1f": the float32 streaming 1x1 form (stream1x1_f32.hip)
constexpr int kStemFloat = 1006;      // "ws7x7f": the float32 stem on that kernel's skeleton (stream1x1_f32.hip)
constexpr int kWinoVariant56 = 1007;     // "wino_f23_5x6": wino_f23 on 5 x 6-tile blocks (two 5 x 3-tile fragments side by side) instead of 4 x 8
constexpr int kWinoVariant56x16 = 1008;  // "wino_f23_5x6_w16": its 16-wave form
constexpr int kStreamBf16 = 1009;        // "bs1x1": the streaming form of the dense 1x1 layers of a bfloat16 net (stream1x1.hip, v_mfma_f32_32x32x16_bf16)
constexpr int kStemBf16 = 1010;          // "bs7x7": the 7x7 / stride-2 stem of a bfloat16 net (stem_f16.hip)
constexpr int kWinoVariantMix = 1011;     // "wino_f23_mix": wino_f23 on a cover of 4 x 8- and 5 x 6-tile blocks in one launch (wino_plan_cover)
constexpr int kWinoVariantMix16 = 1012;   // "wino_f23_mix_w16": its 16-wave form
constexpr int kWinoF43 = 1013;            // "wino_f43": Winograd F(4x4, 3x3), float32, unfused: transform, 36 batched ws1x1f products, inverse (wino43_f32.hip)
constexpr int kFormVariant0 = kWinoVariant, kNumForms = 14;
enum FormGeometry { kForm3x3, kForm1x1, kFormStem };  // the layers a form takes: 3x3, dense 1x1, the 7-row-tap stem
struct ConvForm {
  int variant;
  const char *name, *label;  // in tune caches, reports and set_tile; in the kernel column of plan texts
  int ekind, geometry, waves;  // the element kind of the nets it serves, FormGeometry, waves per workgroup
  const char* const* timing_slots;  // DC_DEBUG_TIMING: the names of its phase slots 1..7
  bool (*eligible)(const ConvGemmParams& p);
  long (*grid)(const ConvGemmParams& p);
  int (*launch)(const ConvGemmParams& p, void* stream);
  bool own_scale;      // runs on an epilogue scale of its own (Launch::form_scale) and takes no shortcut operand
  bool merges;         // a NetGroup merges a member on it as the direct layer it also is; else the member runs apart
  // a multi-problem candidate of NetGroup launches (on the members' shared image), else null
  long (*prepare_multi)(const ConvGemmParams& p, const ConvMultiTable& tb, int nprob);
  int (*launch_multi)(const ConvMultiArgs& a, void* stream);
  int sibling;         // the form on the same image that autotuning compares it with in whole passes, else -1
  const char* env;     // its switch: -1 where measured faster, 0 never, >= 1 wherever eligible; unset = env_default
  // null: a candidate of the per-shape timing wherever eligible; else only where this says so (set_tile and tune caches take it wherever eligible)
  bool (*offered)(const ConvGemmParams& p) = nullptr;
  int env_default = -1;  // what the switch means while unset (0: the form is opt-in)
  // a throughput form: Net::autotune times it alone like any other (the figure is in the tune report, where deepcut_tools.tune_in_flight finds
  // it) but does not choose it — the latency plan of one forward keeps its tile; the form enters a plan by tune_in_flight, set_tile, a tune
  // cache or its switch at >= 1
  bool load_only = false;
};
const ConvForm* conv_form(int variant);  // null: not a form (a tile)

// ---- any variant, tile or form
const char* variant_name(int v);
int variant_by_name(const char* name);  // -1: no tile or form of that name
std::string variant_kernel_label(int v);  // the kernel column of plan texts
long variant_grid(const ConvGemmParams& p, int v);
int launch_conv(const ConvGemmParams& p, int v, void* stream);  // returns hipError_t as int

// The remaining kernels take `ekind` = the ElemKind of the device images (float / _Float16 / __bf16); host-side tensors
// and the per-channel affine vectors are always float.

// MAX pooling, NHWC, windows clipped to the image (pooling_layer.cpp:140-187).
int launch_maxpool(const void* x, void* y, int ekind, int NB, int H, int W, int C, int OH, int OW, int k, int s,
                   int pad, void* stream);

// y = act(x*a[c] + b[c] + z)   (a,b,z optional) — the stand-alone BatchNorm/Scale/ReLU/Eltwise/Sigmoid
// layers when they are not folded into a producing convolution.
int launch_eltwise(const void* x, const void* z, const float* a, const float* b, void* y, int ekind, long total, int C,
                   int relu, int sigmoid, void* stream);

// crop the top-left (offset oh,ow) OH x OW window of an NHWC tensor (crop_layer.cpp:37-50)
int launch_crop(const void* x, void* y, int ekind, int NB, int H, int W, int C, int oh, int ow, int OH, int OW,
                void* stream);

// layout changes at the Blob boundary (host side is NCHW float, blob.hpp:153-164)
// src NCHW [NB,C,H,W] -> dst NHWC with channel pitch CP (>= C, extra channels zeroed)
int launch_nchw_to_nhwc(const float* src, void* dst, int ekind, int NB, int C, int H, int W, int CP, void* stream);
// src NHWC pitch CP, channels [c0, c0+C) -> dst NCHW [NB,C,H,W], float (dst_esize 4) or — from a 16-bit image only — the
// image's own element type (dst_esize 2: the gather payload of an fp16 net, the bf16 values of a bf16 net as they are)
int launch_nhwc_to_nchw(const void* src, void* dst, int ekind, int NB, int C, int H, int W, int CP, int c0,
                        void* stream, int dst_esize = 4);
// packed filter image float -> half (fp16 nets)
int launch_f32_to_f16(const float* src, void* dst, long n, void* stream);
// ... -> bfloat16, rounded to nearest even (bf16 nets)
int launch_f32_to_bf16(const float* src, void* dst, long n, void* stream);

// pose decode (estimate_pose.py:131-143) from NHWC score / refinement maps (channel pitch + first channel)
// Multi-person consumers of the maps.  The reference repository stops at the maps; what these kernels
// invert is the label ENCODING of its training layer (src/caffe/layers/pose_data_layer.cpp:686-802): a cell (row, col)
// stands for the image point pt = (col*8 + 4, row*8 + 4) / scale; loc_pred holds (joint - pt)*scale / sqrt(53);
// next_pred channel pair l holds ((next joint - pt)*scale - mean[l]) / std[l] for regression edge l.
// part_select: per (image, joint) map, the local maxima (value >= thr, maximal in the (2r+1)^2 window, ties to the lower
//           cell index) ordered by (score desc, cell asc); the first max_det go to
//           out[((n*J+j)*max_det + k)*5 + {0..4}] = x, y, score, row, col (x, y refined with loc_pred and divided by scale),
//           counts[n*J+j] = how many were written.  Deterministic for every input (no arrival-order truncation).
//           spill: NB*J*H*W keys of scratch.
int launch_part_select(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, int NB, int H, int W, int J, float thr,
                       int radius, double scale, int max_det, unsigned long long* spill, int* counts, double* out, void* stream);
// pairwise: out[(d*E + l)*2 + k] = pt_k + (next_pred[2l+k] at the detection's cell * std[l][k] + mean[l][k]) / scale
int launch_pairwise_decode(const void* next, int ncp, int nc0, int ekind, int NB, int H, int W, int E, double scale, int ndet,
                           const int* det /* [ndet][3] image, row, col */, const double* mean, const double* stdev, double* out,
                           void* stream);

// Bottom-up assembly of people from those candidates (people.hip; the grouping rule is this project's own: the reference stops at
// the maps).  Limits of the two kernels: candidates per joint, joints, people per image.
constexpr int kPeopleMaxDet = 64, kPeopleMaxJoints = 32, kPeopleMaxPeople = 256;
// pair cost: counts / dets are part_select's outputs (max_det <= kPeopleMaxDet), lut[a*J + c] = the lowest edge index whose (joint,
//           next joint) is (a, c), or -1; mean / stdev [E][2] (never null: 0 / 1 where the caller has none).  With d_f = |prediction
//           of (a, i)'s cell on edge a->c - position of (c, k)| and d_r = |prediction of (c, k)'s cell on edge c->a - position of
//           (a, i)| (image pixels), cost[(((b*J + a)*J + c)*max_det + i)*max_det + k] = scale * mean of those of the two that have an
//           edge; +inf without an edge, for a == c and for slots beyond a count.  Symmetric: [c][a][k][i] is the same number.
int launch_pair_cost(const void* next, int ncp, int nc0, int ekind, int NB, int H, int W, int J, int max_det, double scale, const int* counts,
                     const double* dets, const int* lut, const double* mean, const double* stdev, double* cost, void* stream);
// greedy assembly (one workgroup per image): order [J] = the joints in processing order; link: NB*max_people*max_det doubles of
//           scratch; -> n_people [NB], people [NB][max_people][J][3] = x, y, score (0 where a joint is missing), cand
//           [NB][max_people][J] = candidate index or -1.  The rule: include/deepcut_hip.h, dc_net_assemble_people.
int launch_assemble(int NB, int J, int max_det, int max_people, int min_joints, double max_cost, double seed_thr, const int* counts,
                    const double* dets, const double* cost, const int* order, double* link, int* n_people, double* people, int* cand,
                    void* stream);
// completion (stage D, one workgroup per image and joint; the rule: include/deepcut_hip.h, dc_complete_params): prob / loc in element
//           type `ekind`, next in `next_ekind` (float32 on the sparse pairwise path whatever the net's type); dets, lut, mean, stdev as
//           launch_pair_cost; n_people and cand_in are launch_assemble's outputs and are only read; radius = the assembly's NMS radius.
//           -> people[b][q][j] of every joint filled, cand_out [NB][max_people][J] = cand_in with -2 where a joint was filled (a
//           buffer of its own: every entry is written).  fill_radius <= kCompleteMaxRadius.
constexpr int kCompleteMaxRadius = 16;
int launch_complete(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, const void* next, int ncp, int nc0,
                    int next_ekind, int NB, int H, int W, int J, int max_det, int max_people, double scale, int radius, float fill_thr,
                    int fill_radius, int min_support, const double* dets, const int* lut, const double* mean, const double* stdev,
                    const int* n_people, const int* cand_in, double* people, int* cand_out, void* stream);
// duplicate suppression (stage E, one workgroup per image; the rule: include/deepcut_hip.h, dc_dedupe_params): n_in [NB], people_in
//           [NB][max_people][J][3] and cand_in [NB][max_people][J] are the previous stage's outputs and are only read; sigma is a HOST
//           array [J] or null (all 1.0) and travels as a kernel argument.  -> n_out, people_out, cand_out of the same shapes (buffers of
//           their own, every entry written), kept_from / suppressed_by [NB][max_people] (device, either may be null).  Dynamic LDS:
//           dedupe_lds_bytes(J, max_people), up to 128 KiB.
size_t dedupe_lds_bytes(int J, int max_people);
int launch_dedupe(int NB, int J, int max_people, double max_dist, int min_common, double min_size, int absorb, const double* sigma,
                  const int* n_in, const double* people_in, const int* cand_in, int* n_out, double* people_out, int* cand_out,
                  int* kept_from, int* suppressed_by, void* stream);

// The three passes that write into video frames (draw.hip, redact.hip, heat.hip) share one shape.  On the device (frame_tile.h): one
// workgroup per kDrawTileW x kDrawTileH pixel tile, one thread per 2 x 2 pixel block, so the thread that owns a chroma sample owns its
// luma pixels and no two threads write one byte — "the ownership" below.  On the host: the tile binner of the two passes that walk
// primitives (tile_bins.h) and the stager that moves tables and host frames (FrameStage, net_internal.h).
//
// Skeleton overlay (draw.hip; the rule: include/deepcut_hip.h, dc_draw_people — this project's own).  The host (draw.cpp) snaps the
// joints to 1/16-pixel fixed point, converts the colours and bins the primitives, in drawing order, into the tiles; one workgroup draws
// one non-empty tile, every thread walking the tile's primitives in order, kDrawChunk at a time through LDS.
constexpr int kDrawTileW = 32, kDrawTileH = 32, kDrawChunk = 64;
struct DrawPrim {       // 32 bytes
  int ax, ay, bx, by;   // the ends in 1/16 pixel, |v| <= 2^19; a disc has b == a
  int r16;              // radius in 1/16 pixel, 1..1024
  int capsule;          // 0: the disc at a; 1: the capsule from a to b
  int alpha;            // 0..256
  unsigned colour;      // byte 0, 1, 2 = B, G, R (BGR24) or Y, Cb, Cr (NV12)
};
struct DrawTile {
  int frame, tx, ty;  // the frame and the tile's column and row
  int first, count;   // its primitives: index[first .. first + count), ascending = drawing order
};
struct DrawPlanes {
  unsigned char* plane0;  // as FramePlanes, written
  unsigned char* plane1;
  int pitch0, pitch1;
};
// every part of what a pass uploads (frame table, tiles, index, primitives, tables, colours, staged planes) starts at a multiple of 256 bytes
inline size_t frame_up(size_t bytes) { return (bytes + 255) / 256 * 256; }
// format: DC_PIX_BGR24 or DC_PIX_NV12.  Grid = n_tiles (> 0).  Every pointer is device memory.
int launch_draw(int format, const DrawPlanes* frames, int height, int width, const DrawTile* tiles, int n_tiles, const int* index,
                const DrawPrim* prims, void* stream);

// Redaction (redact.hip; the rule: include/deepcut_hip.h, dc_redact_people — this project's own).  The host (redact.cpp) turns people
// into DrawPrims (alpha and colour unused; a head disc's r16 may reach 16384) and bins them into the drawing kernel's tiles; one
// workgroup redacts one non-empty tile, one thread one 2 x 2 pixel block (the ownership), in three phases between barriers:
// which B x B blocks hold a covered pixel centre, the blocks' sums in LDS (MOSAIC), the stores.
constexpr int kRedactMosaic = 0, kRedactFill = 1;  // DC_REDACT_MOSAIC, DC_REDACT_FILL
// format: DC_PIX_BGR24 or DC_PIX_NV12; effect: kRedactMosaic or kRedactFill; block: 2, 4, 8, 16 or 32; fill: bytes as DrawPrim::colour.
// Grid = n_tiles (> 0).  Every pointer is device memory.
int launch_redact(int format, int effect, int block, unsigned fill, const DrawPlanes* frames, int height, int width, const DrawTile* tiles,
                  int n_tiles, const int* index, const DrawPrim* prims, void* stream);

// Appearance descriptors (appearance.hip; the rule: include/deepcut_hip.h, dc_describe_people — this project's own).  The host
// (appearance.cpp) makes the capsules of every person's sampled limbs with the redaction's body radius, the person's index in
// DrawPrim::colour, and bins them in person order into the drawing kernel's tiles; one workgroup reads one non-empty tile, one thread one
// 2 x 2 pixel block, and counts per person the bytes of the covered pixels into desc [nb][P][3][16] (c, v >> 4): an LDS histogram per
// person, then one integer atomicAdd per non-zero bin.  desc is zeroed by the caller on the same stream; no frame byte is stored.
constexpr int kAppearBins = 16, kAppearDesc = 3 * kAppearBins;  // DC_APPEARANCE_BINS; ints per person
// format: DC_PIX_BGR24 or DC_PIX_NV12.  Grid = n_tiles (> 0).  Every pointer is device memory.
int launch_describe(int format, const DrawPlanes* frames, int height, int width, const DrawTile* tiles, int n_tiles, const int* index,
                    const DrawPrim* prims, int P, int* desc, void* stream);

// Overlays from people in device memory (overlay.hip; the rules are dc_draw_people's and dc_redact_people's, the bytes theirs).  A builder
// kernel — one workgroup per frame, one thread per person — makes the DrawPrims draw.cpp / redact.cpp make on the host, in their order,
// dropping what TileBins::add drops; self-binning forms of the two tile kernels then run over EVERY tile of every frame, each workgroup
// walking its frame's primitives in passes of 256, compacting in order those whose grown box holds a pixel centre of the tile
// (TileBins::add's rule) and handing them to the tile code of frame_tile.h.  A tile nothing reaches loads and stores no pixel.
constexpr int kOverlayMaxIds = 256;  // only_ids / keep_ids, each
constexpr int kOverlayMaxFrames = 64;  // the frame entries' limit on nb
// a host list of n ids (<= kOverlayMaxIds) / a host table of nb frames (<= kOverlayMaxFrames) into device memory AS KERNEL ARGUMENTS of a
// one-workgroup launch: no host buffer has to outlive an upload, and the host waits for nothing
int launch_overlay_put_ids(const long long* host, int n, long long* to, void* stream);
int launch_overlay_put_frames(const DrawPlanes* host, int nb, DrawPlanes* to, void* stream);
struct OverlayBuild {                // a builder launch's arguments, by value (below the 4 KiB of kernel arguments)
  int redact;                        // 0: the drawing's primitives; 1: the redaction's
  int P, J, H, W, n_edges;
  unsigned char edges[2 * 128];      // [n_edges][2]
  double min_score;
  // the drawing: r16 of joints and limbs, the alphas, the colours as DrawPrim::colour (converted on the host)
  int rj, rl, alpha, alpha_filled, by_person, n_palette;
  unsigned untracked, palette[256];
  // the redaction: dc_redact_style's fields, the radius bounds as rint(16 radius); n_only / n_keep < 0: no such list
  int region, head_a, head_b, n_only, n_keep;
  double head_scale, body_scale, r_lo, r_hi;
};
// primitives a person can make at the most, and so a frame's stretch of `prims`: P * overlay_prims_per_person
constexpr int overlay_prims_per_person(int J, int n_edges) { return 1 + n_edges + J; }
// n_people [nb], people [nb][P][J][3], cand [nb][P][J] or null, ids [nb][P] or null, only_ids / keep_ids (read when n_only / n_keep >= 0)
// -> prims [nb][P * per_person] (frame b's first n_prims[b] entries), n_prims [nb], redacted [nb][P] or null (the redaction's).  Every
// pointer is device memory.  Grid = nb.
int launch_overlay_build(const OverlayBuild& q, int nb, const int* n_people, const double* people, const int* cand, const long long* ids,
                         const long long* only_ids, const long long* keep_ids, DrawPrim* prims, int* n_prims, int* redacted, void* stream);
// the tile kernels over all tiles of nb frames: prims / n_prims as the builder left them, stride = P * per_person
int launch_draw_all(int format, const DrawPlanes* frames, int nb, int height, int width, const DrawPrim* prims, const int* n_prims,
                    int stride, void* stream);
int launch_redact_all(int format, int effect, int block, unsigned fill, const DrawPlanes* frames, int nb, int height, int width,
                      const DrawPrim* prims, const int* n_prims, int stride, void* stream);

// Label overlay (label.hip; the rule: include/deepcut_hip.h, dc_label_people — this project's own).  A primitive is one label with both
// its layers; its pixel box is the plate rectangle [x, x + s (6 n + 1)) x [y, y + 9 s), also when the plate is not made.  The host
// (label.cpp) makes the texts, places and clamps the labels, converts the colours and bins the boxes into the tiles (tile_bins.h); one
// workgroup writes one non-empty tile, every thread walking the tile's labels in order, kLabelChunk at a time through LDS.  The device
// form (overlay.hip): a builder launch of the overlay_build_kernel pattern, then label_all_kernel over every tile, kLabelPass labels
// tested at a time.  A frame holds at most 256 labels (one per person), so 256 labels stacked on one tile take four trips through the
// binned walk and two through the self-binning one.
constexpr int kLabelMaxChars = 24;  // DC_LABEL_MAX_CHARS: a text holds at most 23 characters
constexpr int kLabelChunk = 64, kLabelPass = 128;
struct LabelPrim {                       // 56 bytes
  int x, y;                              // the plate's upper left pixel, clamped into the frame
  int n, s;                              // characters (1..23) and scale (1..8)
  unsigned text_colour, plate_colour;    // bytes as DrawPrim::colour
  int alpha_text, alpha_plate;           // 0..256; 0: that layer is not made
  unsigned char text[kLabelMaxChars];    // text[0 .. n): places in the font table (label_font.h)
};
// format: DC_PIX_BGR24 or DC_PIX_NV12.  Grid = n_tiles (> 0); index names places in `prims`.  Every pointer is device memory.
int launch_label(int format, const DrawPlanes* frames, int height, int width, const DrawTile* tiles, int n_tiles, const int* index,
                 const LabelPrim* prims, void* stream);
struct LabelBuild {  // the label builder's arguments, by value
  int P, J, H, W;
  int scale, gap, anchor, alpha_text, alpha_plate, plate_by_person, n_palette, n_prefix;
  double min_score;
  unsigned text_colour, plate_colour, palette[256];  // converted on the host
  unsigned char prefix[4];                           // places in the font table
};
// n_people [nb], people [nb][P][J][3], ids [nb][P] or null -> prims [nb][P] (frame b's first n_labels[b] entries, in person order),
// n_labels [nb].  Every pointer is device memory.  Grid = nb.
int launch_label_build(const LabelBuild& q, int nb, const int* n_people, const double* people, const long long* ids, LabelPrim* prims,
                       int* n_labels, void* stream);
// label_all_kernel over all tiles of nb frames: prims / n_labels as the builder left them, stride = P
int launch_label_all(int format, const DrawPlanes* frames, int nb, int height, int width, const LabelPrim* prims, const int* n_labels,
                     int stride, void* stream);

// Score-map overlay (heat.hip; the rule: include/deepcut_hip.h, dc_draw_heatmap — this project's own).  The host (heat.cpp) computes
// the per-axis sample tables t = rint(256 u), clamped, and converts the colours; one workgroup blends one kDrawTileW x kDrawTileH pixel
// tile of one frame, one thread one 2 x 2 pixel block (the ownership), after staging the patch of map cells the tile's tables
// reach into LDS as 16-bit q = rint(4096 clamp01(s)), the drawn channels only, channel-major.
constexpr int kHeatMaxJoints = 32;
constexpr int kHeatMaxPatch = kDrawTileW * 8 / 8 + 2;  // cells per side at the largest scale, 8: 32 pixels = 32 cells, + 1 for the second tap, + 1 of rounding
struct HeatParams {
  const DrawPlanes* frames;       // [nb], written
  const void* map;                // NHWC view: cell (b, y, x) channel c at ((b Hm + y) Wm + x) cp + c0 + c in the launch's element type;
                                  // NCHW: float32 [nb][C][Hm][Wm]
  const int *tx, *ty, *cx, *cy;   // t of every luma column [W] and row [H]; of every chroma block column and row (NV12; else null)
  const unsigned* colour;         // DC_HEAT_MAX: [256] by v >> 4; DC_HEAT_BY_JOINT: [n_joints] by place in the list; bytes as DrawPrim::colour
  int H, W, Hm, Wm, C, cp, c0;
  int n_joints, by_joint, alpha, alpha_score, vmin;
  int vgate;      // a tile whose staged q are all below it blends nothing: max(vmin, the least v with A(v) > 0)
  int max_cells;  // the largest patch (cells) of any tile: the launch's LDS is n_joints * max_cells * 2 bytes
  unsigned char joints[kHeatMaxJoints];
};
// format: DC_PIX_BGR24 or DC_PIX_NV12; ekind: the map's element type; nchw != 0: the float32 NCHW map.  Grid = tiles x frames.
int launch_heat(int format, int ekind, int nchw, const HeatParams& p, int nb, void* stream);

// Tracking people from frame to frame (track.hip; the rule: include/deepcut_hip.h, dc_tracker_update — this project's own).  A slot's
// state is one block of track_slot_bytes(T, J) bytes, all zero = no track and next_id 0:
//   long long next_id (+ 8 bytes of padding) | long long id[T] | double pose[T][J][3] | double vel[T][J][2] | int live[T] | int misses[T]
//   | int hits[T]
// Limits: T and P <= kPeopleMaxPeople, J <= kPeopleMaxJoints.
struct TrackParams {
  int T, J, max_misses, min_common, motion;
  double max_dist, min_size;
  int assign;  // the matching rule of an update: 0 = step 4 (greedy), 1 = step 4' (optimal assignment); selects the kernel instantiation
};
struct TrackSlot {  // the arrays of one slot inside its block
  long long* next_id;
  long long* id;
  double* pose;
  double* vel;
  int* live;
  int* misses;
  int* hits;
};
inline size_t track_slot_bytes(int T, int J) { return 16 + (size_t)T * (8 + (size_t)J * 5 * 8 + 3 * 4); }
#ifdef __HIP__  // the kernel and the host side both take a block apart with this
#define DC_HOST_DEVICE __host__ __device__
#else
#define DC_HOST_DEVICE
#endif
DC_HOST_DEVICE inline TrackSlot track_slot(unsigned char* block, int T, int J) {
  TrackSlot s;
  s.next_id = (long long*)block;
  s.id = (long long*)(block + 16);
  s.pose = (double*)(s.id + T);
  s.vel = s.pose + (size_t)T * J * 3;
  s.live = (int*)(s.vel + (size_t)T * J * 2);
  s.misses = s.live + T;
  s.hits = s.misses + T;
  return s;
}
// Which slot every image of a launch updates, passed to the kernel BY VALUE (64 bytes: nothing to upload and nothing that has to outlive
// the call): byte b of the words = slot of image b, b < 64.
constexpr int kTrackMaxImages = 64;
struct TrackSlotMap {
  unsigned int w[kTrackMaxImages / 4];
};
inline void track_slot_map_set(TrackSlotMap& m, int b, int slot) { m.w[b >> 2] |= (unsigned)(slot & 0xff) << ((b & 3) * 8); }
// one workgroup per slot s (S of them), whose block is state + s * slot_stride (a multiple of 16).  It applies the images b = 0 .. NB - 1
// with map[b] == s in ascending b, each on the state the one before left; a slot no image names is not touched.  Image b: reads
// n_people[b] (clamped to [0, P]) and people [NB][P][J][3] from device memory, writes the state back in place, dist[b * T *
// kPeopleMaxPeople + i * P + q] (scratch the caller keeps: the matching reads it back), ids [NB][P] and place [NB][P].  sig2 [J] =
// sigma_j^2.  NB <= kTrackMaxImages, every map[b] in [0, S).
// sm (null: off, the instances and the work of a tracker without smoothing): step 8 of the rule behind step 7 of every image, on the
// filters filt [S][T][J] (all zero = every filter empty) -> smooth [NB][P][J][3], src [NB][P][J] (0 nothing, 1 observed, 2 bridged) and,
// where cand_in [NB][P][J] is given, cand_out = cand_in with -3 at the bridged joints (every entry written; cand_in is only read).
struct TrackFilter {  // of one track place and joint, 48 bytes
  double fx, fy, dx, dy, fs;
  int gap, n;  // n: 0 holds nothing, 1 one observation, 2 running
};
struct TrackSmooth {
  double min_cutoff, beta, d_cutoff;
  int max_hold;
  TrackFilter* filt;
  double* smooth;
  int* src;
  const int* cand_in;
  int* cand_out;
};
// ap (null: off, the instances and the work of a tracker without appearance): steps 0', 5', 6' and 7' of the rule (include/deepcut_hip.h,
// dc_tracker_update_appearance), all integer.  A slot's appearance state is one block of track_appear_bytes(T) bytes at
// state + s * slot_stride, all zero = no valid model and an empty gallery:
//   long long gid[64] | int gage[64] | int gocc[64] | int gmodel[64][48] | int valid[T] | int model[T][48]
// desc [NB][P][3][16] (device; null: nobody has a valid descriptor) is only read; qdesc [NB][P][48] is scratch for the quantised
// descriptors; reid [NB][P] is written whole (1: the person took an id from the gallery).
constexpr int kTrackGallery = 64, kTrackModel = 48;  // DC_TRACK_GALLERY; 3 x DC_APPEARANCE_BINS
struct TrackAppearSlot {  // the arrays of one slot inside its block
  long long* gid;
  int* gage;
  int* gocc;
  int* gmodel;
  int* valid;
  int* model;
};
inline size_t track_appear_bytes(int T) { return (size_t)kTrackGallery * (8 + 4 + 4 + kTrackModel * 4) + (size_t)T * (4 + kTrackModel * 4); }
DC_HOST_DEVICE inline TrackAppearSlot track_appear_slot(unsigned char* block, int T) {
  TrackAppearSlot s;
  s.gid = (long long*)block;
  s.gage = (int*)(s.gid + kTrackGallery);
  s.gocc = s.gage + kTrackGallery;
  s.gmodel = s.gocc + kTrackGallery;
  s.valid = s.gmodel + kTrackGallery * kTrackModel;
  s.model = s.valid + T;
  return s;
}
struct TrackAppear {
  int min_pixels, alpha256, reid_max, max_age, min_hits;
  unsigned char* state;
  size_t slot_stride;  // a multiple of 8
  const int* desc;
  int* qdesc;
  int* reid;
};
int launch_track(int S, int NB, int P, const TrackParams& p, const double* sig2, unsigned char* state, size_t slot_stride, double* dist,
                 const int* n_people, const double* people, long long* ids, int* place, const TrackSlotMap& map, void* stream,
                 const TrackSmooth* sm = nullptr, const TrackAppear* ap = nullptr);

// The pairwise head at a list of cells (sparse_head.hip; the rule: include/deepcut_hip.h, dc_net_pairwise_at).  x3 / x5: the NHWC inputs
// of the head's 1x1 skip convolution ([NB][H][W], pitch cp3, K3 channels) and of its stride-2 3x3 deconvolution ([NB][h5][w5], pitch cp5,
// K5 channels), first channel already added, in the net's element type; vec3 / vec5: 4 consecutive channels of a cell may be read as one
// aligned vector (K % 4 == 0, pitch and first channel multiples of 4).  wimg / bias: sparse_head_pack_filters' image and bias_s + bias_d
// [Cout].  out: float32 [NB][H][W][Cout]; only the listed cells are written.
struct SparseHeadArgs {
  const void* x3;
  const void* x5;
  const float* wimg;
  const float* bias;
  float* out;
  int cp3, cp5, K3, K5, Cout;
  int NB, H, W, h5, w5, oh, ow;
  int vec3, vec5;
};
// the image's size in floats, and the image: ws [cout][k3], wd [k5][cout][3][3] -> [segment 0..9][ceil(cout/32)][K block of 8][64][4]
// (segment t < 9: tap ky*3 + kx = t over k5, at float offset t * ceil(cout/32) * ceil(k5/8) * 256; segment 9: the skip over k3, behind them)
size_t sparse_head_image_floats(int cout, int k3, int k5);
void sparse_head_pack_filters(const float* ws, const float* wd, int cout, int k3, int k5, float* out);
// p[i] = (float)(T)p[i] in place, T the 16-bit type of ekind (nothing for float32): the filters as a 16-bit net's dense head sees them
int launch_round_through(float* p, long n, int ekind, void* stream);
// Two launches: the n slots — part_select's candidates (counts [NB*J], dets [NB*J][MD][5], n = NB*J*MD, cells null) or n (image, row,
// col) triples on the device (cells; counts / dets null) — sorted into the four parity classes in `work` (4 + 4n ints of scratch), then
// the head at those cells.  Slots that are no cell of the map are skipped.
int launch_sparse_head(const SparseHeadArgs& a, int ekind, const int* counts, const double* dets, int J, int MD, const int* cells, int n,
                       int* work, void* stream);

// out[d*C + ch] = (float) map[((n*H + row)*W + col)*cp + c0 + ch] for detection d = (n, row, col) of det [ndet][3] (device; every cell
// inside the map: the caller checked): the raw values of a map at given cells
int launch_map_gather(const void* map, int cp, int c0, int ekind, int H, int W, int C, int ndet, const int* det, float* out, void* stream);

// Multi-scale fusion of the maps of a pyramid (pose.hip; the rule is this project's own, like the assembly above: include/deepcut_hip.h,
// dc_group_fuse_maps and dc_group_fuse_maps_mirrored).  Member m holds the maps of the same NB images at its own scale; map k (0 prob,
// 1 loc_pred, 2 next_pred) is the NHWC image ptr[k] of H x W cells with channel pitch cp[k], first channel c0[k]; q = scale of m / scale
// of the base member.
struct FuseMember {
  const void* ptr[3];
  int cp[3], c0[3];
  int H, W;
  double q;
};
// One record per (member, image), [M][NB]: on marks a member that saw the image flipped left to right, ws = (width - 1) * the scale the
// member ran that image at — the image entries fill every image of a member with (image width - 1) * the member's scale, the box entry
// (dc_group_decode_boxes) gives every box its own crop width and scale
struct FuseFlip {
  double ws;
  int on, pad_;
};
// One launch for every member, map and image: out[((b*Hb + r)*Wb + c)*Ctot + ch] (float32, NHWC, pitch Ctot = C[0] + C[1] + C[2]) =
// (sum over m ascending of bilinear sample of member m at the cell's point * gain[m*Ctot + ch] + bias[m*Ctot + ch]) * (1 / M).
// Channels [0, C[0]) are map 0, the next C[1] map 1, the last C[2] map 2; a map with C[k] = 0 takes no part (its ptr is not read).
// members / gain / bias are device tables ([M], [M][Ctot], [M][Ctot]); ekind is the members' common element type.
// flip and src both null: no member is mirrored, and neither table is read.  Both given ([M][NB], [M][Ctot]): the same kernel body with two
// differences — image b of a member with flip[m*NB + b].on is sampled at the column u = ((ws - (8c + 4) q) - 4) / 8, clamped to the member's
// whole map like every other sample, and output channel ch reads from
// member m the channel src[m*Ctot + ch] WITHIN its map (0 .. C[k] - 1; the identity for an unmirrored member); the sign changes are in
// gain / bias.  Exactly one of the two null: hipErrorInvalidValue.
int launch_fuse_maps(const FuseMember* members, const FuseFlip* flip, const float* gain, const float* bias, const int* src, int M, int ekind,
                     int NB, int Hb, int Wb, const int C[3], float* out, void* stream);

// Image pre-processing of the demo (python/pose/estimate_pose.py:83-103) on the device: replicate padding by
// coordinate clamping, Pillow's two-pass 8-bit bilinear resample (22-bit fixed-point weights from the host),
// mean subtraction and the zero canvas, written straight into the network's NHWC input image.
// mirror: the image is read flipped left to right — source column w - 1 - x wherever column x of the unpadded image would be read, so
// the replicate padding repeats the FLIPPED image's last column (source column 0) — and everything after that is unchanged: the result
// is, bit for bit, what the unmirrored path makes of the host-flipped image (dc_group_forward_images_mirrored).  BoxPrepParams::mirror is
// the same for every crop of a launch: crop column it.w - 1 - sx wherever column sx of the unpadded crop would be read, after the clamp.
//
// Source-pixel readers (the kernels' compile-time parameter; the rule: include/deepcut_hip.h, dc_frame).  kReadPacked is the packed
// BGR block `src` the existing entries hand over.  The two frame readers take image n's planes from a device table instead:
// kReadBgr the same three bytes through a row pitch, kReadNv12 a Y byte at (x, y) and the Cb, Cr pair at (x >> 1, y >> 1), converted
// to B, G, R where the pixel is fetched — after the clamp and the mirror reflection, with the image's absolute coordinates —, so
// everything behind the fetch (replicate padding, mirror, both resample passes, the direct branch, tmp, mean, canvas) is one body.
enum { kReadPacked = 0, kReadBgr = 1, kReadNv12 = 2 };
struct FramePlanes {
  const unsigned char* plane0;  // Y rows (NV12) or B,G,R rows (BGR24)
  const unsigned char* plane1;  // Cb,Cr rows (NV12); unused otherwise
  int pitch0, pitch1;           // bytes
};
struct FrameSource {
  const FramePlanes* planes;  // [n] device table, one entry per image of the batch (the box entry: one); nullptr with kReadPacked
  int reader;                 // kRead*
  int ky, rv, bu, gu, gv, y0;  // NV12: 16.16 fixed-point coefficients of the conversion and the luma offset (net_image.cpp frame_csc)
};
struct ImagePrepParams {
  const unsigned char* src;  // [n][h][w][3] BGR uint8 (kReadPacked)
  FrameSource frame;         // the frame readers' source; zero for kReadPacked
  int n, h, w;
  int out_h, out_w;          // canvas = the network input
  int use_h, use_w;          // top-left part of the resized image that lands on the canvas; the rest is zero
  const int* x_bounds;       // [new_w][2] first tap, tap count; nullptr: no horizontal pass
  const int* x_coeffs;       // [new_w][x_ksize]
  int x_ksize;
  const int* y_bounds;       // nullptr: no vertical pass
  const int* y_coeffs;
  int y_ksize;
  unsigned char* tmp;        // [n][rows][use_w][4]: rows row0..row0+rows of the horizontally resampled padded image
  int row0, rows;
  void* dst;                 // [n][out_h][out_w][dst_cp] float, _Float16 or __bf16 (dst_ekind); pad channels zeroed
  int dst_ekind, dst_cp;
  float mean[3];
  int mirror;                // 0 / 1
};
int launch_image_prep(const ImagePrepParams& p, void* stream);

// The same pre-processing for n person boxes of ONE image, in one launch: item i is the crop src[y0:y0+h, x0:x0+w] treated as an
// image of its own (the 64-px replicate padding repeats the CROP's last row / column: reads are clamped at the window's edges),
// resampled with its own tables and pasted at the top-left of canvas i.  Both resample passes run per output pixel (the
// horizontal pass of each tap row is recomputed in registers and clipped to 8 bits as Pillow's intermediate image is), so there is
// no intermediate buffer and no second launch.
struct BoxPrepItem {
  int x0, y0, h, w;        // the source window
  int use_h, use_w;        // top-left part of the resized crop that lands on the canvas; the rest of canvas i is zero
  const int* x_bounds;     // [new_w][2] (first tap, tap count) in padded-crop columns; nullptr: no horizontal pass
  const int* x_coeffs;     // [new_w][x_ksize]
  const int* y_bounds;     // nullptr: no vertical pass
  const int* y_coeffs;
  int x_ksize, y_ksize;
};
struct BoxPrepParams {
  const unsigned char* src;  // [img_h][img_w][3] BGR uint8 (kReadPacked)
  FrameSource frame;         // the frame readers' source (one table entry); zero for kReadPacked
  int img_h, img_w;
  int n;
  int out_h, out_w;          // the common canvas of every item (= the network input)
  const BoxPrepItem* items;  // [n], device memory
  void* dst;                 // [n][out_h][out_w][dst_cp] float, _Float16 or __bf16 (dst_ekind); pad channels zeroed
  int dst_ekind, dst_cp;
  float mean[3];
  int mirror;                // 0 / 1: every crop of this launch is read flipped left to right (dc_group_forward_boxes_mirrored)
};
int launch_box_prep(const BoxPrepParams& p, void* stream);

int launch_pose_decode(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, int NB, int H,
                       int W, int J, double scale, double* out, void* stream);
// launch_pose_decode with a scale, an offset and a valid cell extent per image (device table `items`, one per image): the arg-max
// runs over cells [0, rows) x [0, cols) only, x and y are divided by the item's scale and then shifted by (dx, dy)
struct PoseDecodeItem {
  double scale, dx, dy;
  int rows, cols;
};
int launch_pose_decode_items(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, int NB, int H,
                             int W, int J, const PoseDecodeItem* items, double* out, void* stream);

}  // namespace dc
