// conv_gemm.cpp — host side of the gather-GEMM (conv_gemm.h): the tile tables, the launch preparation and the three launches
// (single problem, multi-class, multi-problem).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "kernels.h"

namespace dc {

// The kernel (conv_gemm.h), declared only: conv_gemm_f32.hip, conv_gemm_f16.hip and conv_gemm_bf16.hip instantiate the rows of
// conv_gemm_variants.h for one element type each, the tables below point to those instantiations.
template <typename T, int BM, int BN, int BK, int WR, int WC, int WK, int PF, bool MC = false, int DMA = 0, bool SWP = false, bool MP = false>
__global__ void conv_gemm_kernel(const std::conditional_t<MP, ConvMultiArgs, ConvGemmParams> ka);

void dc_magic(unsigned d, unsigned (&mg)[2]) {
  if (d <= 1) {
    mg[0] = 0;
    mg[1] = 0x80000000u;
    return;
  }
  int l = 0;
  while ((1ull << l) < d) ++l;
  const int sh = 31 + l;
  const unsigned long long q = (((unsigned __int128)1) << sh) / d;
  mg[0] = (unsigned)(q + 1);
  mg[1] = (unsigned)(sh - 32);
}

namespace {
struct VariantEntry {
  ConvVariant v;
  void (*kernel)(const ConvGemmParams);
  int BK;
  int esize;
  void (*kernel_mc)(const ConvGemmParams);  // multi-class instantiation (the deconvolution heads), or null
  void (*kernel_mp)(const ConvMultiArgs);   // multi-problem instantiation (pyramid-grouped launches)
};
// the three instantiations of one tile: single problem, multi-class (or null), multi-problem
#define DC_TABLE_ROW(T, ES, NAME, BM, BN, BK, WR, WC, WK, PF, DMA, SWP, WITH_MC)                                \
  {{NAME, BM, BN, WR, WC, WK}, conv_gemm_kernel<T, BM, BN, BK, WR, WC, WK, PF, false, DMA, SWP>, BK, ES,        \
   WITH_MC ? conv_gemm_kernel<T, BM, BN, BK, WR, WC, WK, PF, WITH_MC, DMA, SWP> : nullptr,                      \
   conv_gemm_kernel<T, BM, BN, BK, WR, WC, WK, PF, false, DMA, SWP, true>},
const VariantEntry kVariants[] = {
#define DC_ROW_F32(...) DC_TABLE_ROW(float, 4, __VA_ARGS__)
#define DC_ROW_F16(...) DC_TABLE_ROW(_Float16, 2, __VA_ARGS__)
#define DC_ROW_BF16(...)
#include "conv_gemm_variants.h"
};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);
const VariantEntry kVariantsBf16[] = {
#define DC_ROW_F32(...)
#define DC_ROW_F16(...)
#define DC_ROW_BF16(...) DC_TABLE_ROW(__bf16, 2, __VA_ARGS__)
#include "conv_gemm_variants.h"
};
constexpr int kNumBf16Variants = sizeof(kVariantsBf16) / sizeof(kVariantsBf16[0]);
// the table entry of a variant number (callers have checked it with dc_variant_ok)
const VariantEntry& entry_of(int v) { return v >= kBf16Variant0 ? kVariantsBf16[v - kBf16Variant0] : kVariants[v]; }
bool dc_variant_ok(int v) { return (v >= 0 && v < kNumVariants) || (v >= kBf16Variant0 && v < kBf16Variant0 + kNumBf16Variants); }
}  // namespace

int conv_num_variants() { return kNumVariants; }
int conv_num_bf16_variants() { return kNumBf16Variants; }
const ConvVariant& conv_variant(int i) { return entry_of(i).v; }
int conv_variant_bk(int i) { return entry_of(i).BK; }
int conv_variant_esize(int i) { return entry_of(i).esize; }
int conv_variant_ekind(int i) { return is_bf16_variant(i) ? kElemBF16 : conv_variant_esize(i) == 2 ? kElemF16 : kElemF32; }
bool conv_variant_multiclass(int i) { return entry_of(i).kernel_mc != nullptr; }
const int* conv_variants_of(int ekind, int* count) {
  static const std::vector<int>* lists = [] {
    auto* l = new std::vector<int>[3];
    for (int v = 0; v < kNumVariants; ++v) l[kVariants[v].esize == 2 ? kElemF16 : kElemF32].push_back(v);
    for (int v = 0; v < kNumBf16Variants; ++v) l[kElemBF16].push_back(kBf16Variant0 + v);
    return l;
  }();
  const std::vector<int>& l = lists[ekind == kElemBF16 ? kElemBF16 : ekind == kElemF16 ? kElemF16 : kElemF32];
  *count = (int)l.size();
  return l.data();
}
bool conv_variant_exists(int v) { return dc_variant_ok(v); }
int conv_variant_by_name(const char* name) {
  for (int v = 0; v < kNumVariants; ++v)
    if (!std::strcmp(name, kVariants[v].v.name)) return v;
  for (int v = 0; v < kNumBf16Variants; ++v)
    if (!std::strcmp(name, kVariantsBf16[v].v.name)) return kBf16Variant0 + v;
  return -1;
}

long conv_grid(const ConvGemmParams& p, int variant) {
  const ConvVariant& v = entry_of(variant).v;
  const long tn = (p.Cout + v.BN - 1) / v.BN;
  if (p.ncls > 1) {
    long g = 0;
    for (int c = 0; c < p.ncls; ++c) g += (p.cls[c].M + v.BM - 1) / v.BM * tn;
    return g;
  }
  long tm = (p.M + v.BM - 1) / v.BM;
  return tm * tn;
}

// ---- gather-GEMM launch preparation, shared by the single-problem, multi-class and multi-problem launches

// the switches of the launches (on unless set to 0), each read once, at its first use
static int env_on(const char* name) { return getenv(name) ? atoi(getenv(name)) : 1; }
bool xcd_map_on() {  // DC_XCD_MAP: the per-XCD tile map of single-problem launches and of the Winograd forms
  static const int on = env_on("DC_XCD_MAP");
  return on != 0;
}
static bool dense_on() {  // DC_DENSE: dense_x / dense_y
  static const int on = env_on("DC_DENSE");
  return on != 0;
}
static bool wide_epi_on() {  // DC_WIDE_EPI: the float16 epilogue through LDS
  static const int on = env_on("DC_WIDE_EPI");
  return on != 0;
}

// buffer (V#) addressing carries 32-bit byte offsets: every tensor of a launch must stay below 2 GiB
static constexpr double k2GiB = 2147483647.0;
static bool images_fit(double es, double nb, long x_img_stride, long y_img_stride) {  // input and output of nb images, es-byte elements
  return es * nb * (double)x_img_stride < k2GiB && es * nb * (double)y_img_stride < k2GiB;
}
// most negative tap displacement: one of the four corners of the arithmetic grid (t: the launch, a class or a problem)
template <class T>
static int tap_bias(const T& t, int x_row_stride) {
  int bias = 0;
  for (int ty : {0, t.nty - 1})
    for (int tx : {0, t.ntx - 1}) bias = std::min(bias, (t.dy0 + ty * t.ddy) * x_row_stride + t.x0 + tx * t.ddx);
  return bias;
}
// the output-pixel divisions and the m tiles of the launch, a class or a problem
template <class T>
static void set_m_tiles(T& t, int BM) {
  dc_magic((unsigned)(t.OH * t.OW), t.div_ohw);
  dc_magic((unsigned)t.OW, t.div_ow);
  t.tiles_m = (t.M + BM - 1) / BM;
}
// the output (and shortcut) of one tensor takes 16-byte vectors: strides in whole vectors of es-byte elements, aligned bases
template <class T>
static bool out_vec16(const T& t, long es) {
  return (t.y_pix_stride * es) % 16 == 0 && (t.y_row_stride * es) % 16 == 0 && (t.y_img_stride * es) % 16 == 0 && ((uintptr_t)t.y & 15) == 0 &&
         (!t.resid || ((uintptr_t)t.resid & 15) == 0);
}
// vec_epi and wide_epi of a launch whose every tensor passes out_vec16 (vec).  wide_epi (float16) asks for Cout and the output strides
// in multiples of 8 halves: for 2-byte elements exactly what vec_epi asks
static void set_epi(ConvGemmParams& p, bool vec) {
  p.vec_epi = vec && (p.Cout * (long)p.esize) % 16 == 0 && p.sigmoid_ch == 0;
  p.wide_epi = wide_epi_on() && p.esize == 2 && p.vec_epi;
}
// dense_x / dense_y (ConvGemmParams) of the launch or a problem; sy, sx and klen are the layer's
template <class T>
static bool dense_x_of(const T& t, const ConvGemmParams& p) {
  return dense_on() && t.nty == 1 && t.ntx == 1 && t.dy0 == 0 && t.x0 == 0 && p.sy == 1 && t.x_rows == t.OH && t.x_row_stride == t.OW * p.sx &&
         t.x_img_stride == (long)t.OH * t.x_row_stride && t.x_rowlen >= (t.OW - 1) * p.sx + p.klen;
}
template <class T>
static bool dense_y_of(const T& t) {
  return dense_on() && t.y_row_stride == t.OW * t.y_pix_stride && t.y_img_stride == (long)t.OH * t.y_row_stride;
}
// XCD arrangement gx x gy of a multi-class or multi-problem launch (rows[c]: m tiles of class / problem c) minimising what one L2 has to
// fetch (its share of the filters + its share of the pixels): sets p.mc_lgx, returns the grid (8 x the longest walk of an XCD) or 0
static long mc_xcd_grid(ConvGemmParams& p, const int* rows, int n, long tn, double wtot, double atot) {
  long blk = 0, total = 0;
  double best = 1e300;
  for (int c = 0; c < n; ++c) total += rows[c] * tn;
  for (int lgx = 0; lgx <= 3; ++lgx) {
    const int gx = 1 << lgx, gy = 8 >> lgx;
    if (gx > tn) continue;
    long longest = 0;
    for (int xq = 0; xq < 8; ++xq) {
      const int qx = xq & (gx - 1), qy = xq >> lgx;
      const long ncnt = ((tn * (qx + 1)) >> lgx) - ((tn * qx) >> lgx);
      long cnt = 0;
      for (int c = 0; c < n; ++c) cnt += ((((long)rows[c] * (qy + 1)) >> (3 - lgx)) - (((long)rows[c] * qy) >> (3 - lgx))) * ncnt;
      longest = std::max(longest, cnt);
    }
    const double cost = (wtot / gx + atot / gy) * (1.0 + 0.02 * (longest * 8 - total) / (double)std::max(total, 1L));
    if (cost < best) best = cost, p.mc_lgx = lgx, blk = longest * 8;
  }
  return blk;
}

int launch_conv_gemm(const ConvGemmParams& p_in, int variant, void* stream) {
  if (!dc_variant_ok(variant)) return (int)hipErrorInvalidValue;
  const VariantEntry& e = entry_of(variant);
  ConvGemmParams p = p_in;
  if (p.esize != e.esize || (p.ekind == kElemBF16) != is_bf16_variant(variant)) return (int)hipErrorInvalidValue;
  const long tn = (p.Cout + e.v.BN - 1) / e.v.BN;
  const int nt = e.v.WR * e.v.WC * e.v.WK * 64;
  if (p.ncls > 1) {
    // multi-class launch: the residue classes of a strided deconvolution as consecutive ranges of ONE grid
    if (p.ncls > kMaxClasses || !e.kernel_mc || !images_fit(e.esize, p.NB, p.x_img_stride, p.y_img_stride)) return (int)hipErrorInvalidValue;
    double wtot = 0, atot = 0;
    int rows[kMaxClasses];
    for (int c = 0; c < p.ncls; ++c) {
      ConvClass& q = p.cls[c];
      const int ntaps = q.nty * q.ntx;
      if (ntaps < 1 || ntaps > kMaxTaps || p.klen % e.BK != 0 || q.Ktot != ntaps * p.klen || q.M <= 0) return (int)hipErrorInvalidValue;
      q.x_bias = tap_bias(q, p.x_row_stride);
      set_m_tiles(q, e.v.BM);
      rows[c] = q.tiles_m;
      wtot += (double)e.esize * p.Cout * (double)q.Ktot;
      atot += (double)e.esize * q.M * (double)p.klen * q.nty;
    }
    if (wtot >= k2GiB) return (int)hipErrorInvalidValue;
    p.wide_epi = p.vec_epi = p.dense_x = p.dense_y = 0;
    p.tiles_n = (int)tn;
    dc_magic((unsigned)tn, p.div_tn);
    p.xcd_on = 0;
    const long blk = mc_xcd_grid(p, rows, p.ncls, tn, wtot, atot);
    if (blk <= 0 || blk > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(e.kernel_mc, dim3((unsigned)blk), dim3(nt), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
  }
  const int ntaps = p.nty * p.ntx;
  if (ntaps < 1 || ntaps > kMaxTaps || p.klen % e.BK != 0 || p.Ktot != ntaps * p.klen) return (int)hipErrorInvalidValue;
  if (!images_fit(e.esize, p.NB, p.x_img_stride, p.y_img_stride) || (double)e.esize * p.Cout * (double)p.Ktot >= k2GiB) return (int)hipErrorInvalidValue;
  set_epi(p, out_vec16(p, p.esize));
  p.dense_x = dense_x_of(p, p);
  p.dense_y = dense_y_of(p);
  p.x_bias = tap_bias(p, p.x_row_stride);
  long grid = conv_grid(p, variant);
  if (grid <= 0) return 0;
  p.tiles_n = (int)tn;
  dc_magic((unsigned)tn, p.div_tn);
  set_m_tiles(p, e.v.BM);
  const long tm = p.tiles_m;
  p.xcd_on = 0;
  if (xcd_map_on() && grid >= 16) {
    // Blocks are observed to land on XCD (blockIdx % 8), each with its own 4 MB L2.  Cut the tile grid into 8
    // rectangles (gx along n, 8/gx along m) minimising the bytes an L2 must fetch for its rectangle
    // (filters of its n-range + pixels of its m-range); XCD q walks rectangle q.  A locality hint only.
    double best = 1e300;
    int best_lgx = -1;
    long best_grid = 0;
    for (int lgx = 0; lgx <= 3; ++lgx) {
      const int gx = 1 << lgx, gy = 8 >> lgx;
      if (gx > tn || gy > tm) continue;
      long maxrect = 0;
      for (int q = 0; q < 8; ++q) {
        const int qx = q & (gx - 1), qy = q >> lgx;
        const long rw = ((tn * (qx + 1)) >> lgx) - ((tn * qx) >> lgx), rh = ((tm * (qy + 1)) >> (3 - lgx)) - ((tm * qy) >> (3 - lgx));
        maxrect = std::max(maxrect, rw * rh);
      }
      const double w_bytes = (double)p.Cout * p.Ktot / gx, a_bytes = (double)p.M * p.klen * p.nty / gy;
      const double cost = (w_bytes + a_bytes) * (1.0 + 0.02 * (maxrect * 8 - grid) / (double)grid);
      if (cost < best) best = cost, best_lgx = lgx, best_grid = maxrect * 8;
    }
    if (best_lgx >= 0) {
      p.xcd_lgx = best_lgx;
      const unsigned w0 = (unsigned)(tn >> best_lgx);
      dc_magic(std::max(w0, 1u), p.div_rw[0]);
      dc_magic(w0 + 1, p.div_rw[1]);
      p.xcd_on = 1;
      grid = best_grid;
    }
  }
  hipLaunchKernelGGL(e.kernel, dim3((unsigned)grid), dim3(nt), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

bool conv_variant_multiproblem(int i) { return entry_of(i).kernel_mp != nullptr; }

// Multi-problem launch: host-side preparation (once per plan), see kernels.h.
long prepare_conv_multi(ConvGemmParams& p, ConvMultiTable& tb, int nprob, int variant) {
  if (const ConvForm* f = conv_form(variant)) {
    const long g = f->prepare_multi ? f->prepare_multi(p, tb, nprob) : -1;
    if (g > 0) p.nprob = nprob, p.ncls = 0;
    return g;
  }
  if (!dc_variant_ok(variant) || nprob < 1 || nprob > kMaxProblems) return -1;
  const VariantEntry& e = entry_of(variant);
  if (!e.kernel_mp || p.esize != e.esize || (p.ekind == kElemBF16) != is_bf16_variant(variant) || p.klen % e.BK != 0) return -1;
  const long es = p.esize;
  const long tn = (p.Cout + e.v.BN - 1) / e.v.BN;
  bool vec = true;
  double atot = 0;
  long w_lo = 0, w_hi = 0;
  int rows[kMaxProblems];
  for (int c = 0; c < nprob; ++c) {
    ConvProblem& q = tb.prob[c];
    const int ntaps = q.nty * q.ntx;
    if (ntaps < 1 || ntaps > kMaxTaps || q.Ktot != ntaps * p.klen || q.M <= 0 || q.NB <= 0) return -1;
    if (!images_fit(es, q.NB, q.x_img_stride, q.y_img_stride)) return -1;
    if ((q.resid != nullptr) != (tb.prob[0].resid != nullptr)) return -1;
    q.x_bias = tap_bias(q, q.x_row_stride);
    set_m_tiles(q, e.v.BM);
    rows[c] = q.tiles_m;
    q.dense_x = dense_x_of(q, p);
    q.dense_y = dense_y_of(q);
    vec = vec && out_vec16(q, es);
    w_lo = std::min(w_lo, q.w_off);
    w_hi = std::max(w_hi, q.w_off + (long)p.Cout * q.Ktot);
    atot += (double)es * q.M * (double)p.klen * q.nty;
  }
  const double wtot = (double)es * (double)(w_hi - w_lo);
  if (wtot >= k2GiB) return -1;
  p.nprob = nprob;
  p.ncls = 0;
  set_epi(p, vec);
  p.dense_x = p.dense_y = 0;
  p.xcd_on = 0;
  p.tiles_n = (int)tn;
  dc_magic((unsigned)tn, p.div_tn);
  const long blk = mc_xcd_grid(p, rows, nprob, tn, wtot, atot);
  if (blk <= 0 || blk > 0x7fffffffL) return -1;
  {
    const int lgx = p.mc_lgx, lgy = 3 - lgx;
    const unsigned w0 = (unsigned)(tn >> lgx);
    dc_magic(std::max(w0, 1u), p.div_rw[0]);
    dc_magic(w0 + 1, p.div_rw[1]);
    for (int qy = 0; qy < 8; ++qy) {
      int run = 0;
      for (int c = 0; c < kMaxProblems; ++c) {
        if (c < nprob && qy < (8 >> lgx)) {
          run += (int)((((long)tb.prob[c].tiles_m * (qy + 1)) >> lgy) - (((long)tb.prob[c].tiles_m * qy) >> lgy));
          tb.end[qy][c] = run;
        } else {
          tb.end[qy][c] = 0x7fffffff;
        }
      }
    }
  }
  return blk;
}

int launch_conv_multi(const ConvMultiArgs& a, int variant, long grid, void* stream) {
  if (const ConvForm* f = conv_form(variant)) return f->launch_multi ? f->launch_multi(a, stream) : (int)hipErrorInvalidValue;
  if (!dc_variant_ok(variant) || !entry_of(variant).kernel_mp || a.p.nprob < 1 || grid <= 0) return (int)hipErrorInvalidValue;
  const VariantEntry& e = entry_of(variant);
  const int nt = e.v.WR * e.v.WC * e.v.WK * 64;
  hipLaunchKernelGGL(e.kernel_mp, dim3((unsigned)grid), dim3(nt), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace dc
