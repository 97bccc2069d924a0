// wino43_f32.hip — Winograd F(4x4, 3x3) for the float32 stride-1 3x3 layers, UNFUSED (form "wino_f43" of forms.cpp): three kernels on one stream.
//   1. wino43_input_kernel: every 6 x 6 input patch transformed ONCE per layer, V[p][r][ci] = (B^T d B)[p] (p = 6 i + j, r = the tile's row);
//   2. ws1x1f_kernel<.., BATCH> (stream1x1_f32.hip): the 36 points as plain matrix products M[p] = V[p] U[p], nothing but MFMAs in the loop;
//   3. wino43_output_kernel: Y = A^T M A per tile, the folded BatchNorm / Scale affine, ReLU, the up-to-4 x 4 real pixels of the tile.
// A 4 x 4 output tile costs 36 products per (ci, co) where F(2x2, 3x3) spends 4 x 16 = 64: 0.5625 of the matrix work of wino_f23, for two
// bandwidth passes over V and M (2.25 x the activation bytes each) and two more launches.  The fused probe (tools/probes/winograd43_probe.hip)
// redid the input transform for every 16-channel slice and ran it on the matrix pipe's own datapath; here it runs once, in a kernel of its own.
//
// Tiles: a dilated layer (dilation d = pad, 1 or 2) is d x d independent pad-1 convolutions on its phase images (pixel (y' d + py, x' d + px) of the
// map is pixel (y', x') of phase (py, px)), as wino_f23 takes them.  Every phase image gets the same TY x TX tile grid, TY = ceil(ceil(H / d) / 4);
// the smaller phases' surplus tiles read zeros and store nothing.  Row r = ((n d d + phase) TY + ty) TX + tx; R rows, not padded.
// Points 0, +-1, +-2, inf:
//   B^T = [[4,0,-5,0,1,0],[0,-4,-4,1,1,0],[0,4,-4,-1,1,0],[0,-2,-1,2,1,0],[0,2,-1,-2,1,0],[0,4,0,-5,0,1]]
//   G   = [[1/4,0,0],[-1/6,-1/6,-1/6],[-1/6,1/6,-1/6],[1/24,1/12,1/6],[1/24,-1/12,1/6],[0,0,1]]
//   A^T = [[1,1,1,1,1,0],[0,1,-1,2,-2,0],[0,1,1,4,4,0],[0,1,-1,8,-8,1]]
// Error: the transforms' entries reach 8 and 1/24, so the form is ~20 x less exact than F(2x2, 3x3) (1.1e-5 x range on a res4 layer against
// 6e-7, tests/test_wino43_host.py), inside the Winograd tests' 1e-4 x range.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "kernel_prims.h"
#include "kernels.h"

namespace dc {
namespace {

struct W43Args {
  const void* x;     // input NHWC (input kernel) / unused
  float* V;          // [36][R][Cin] (input kernel: written)
  const float* M;    // [36][R][Cout] (output kernel: read)
  void* y;
  const float* scale;
  const float* shift;
  int R, TY, TX, d, H, W;     // rows; tile grid of a phase image; dilation; the map
  int C, lgq;                 // channels of the tensor the kernel reads (Cin / Cout) and log2(C / 4) where C / 4 is a power of two, else -1
  int ximg, xrow, xpix;       // input strides in bytes (images, rows, pixels)
  int yimg, yrow, ypix;       // output strides in bytes
  int relu;
};

// the tile of row r: image n, phase (py, px), tile (ty, tx)
struct W43Tile {
  int n, py, px, ty, tx;
};
__device__ __forceinline__ W43Tile w43_tile(const W43Args& a, unsigned r) {
  W43Tile t;
  const unsigned q0 = r / (unsigned)a.TX;
  t.tx = (int)(r - q0 * (unsigned)a.TX);
  const unsigned q1 = q0 / (unsigned)a.TY;
  t.ty = (int)(q0 - q1 * (unsigned)a.TY);
  const unsigned dd = (unsigned)(a.d * a.d), q2 = q1 / dd, ph = q1 - q2 * dd;
  t.n = (int)q2, t.py = (int)(ph / (unsigned)a.d), t.px = (int)(ph - (unsigned)t.py * (unsigned)a.d);
  return t;
}

// B^T applied to six values (the same along rows and columns)
__device__ __forceinline__ void w43_bt(const f32x4 (&d)[6], f32x4 (&o)[6]) {
  o[0] = 4.f * d[0] - 5.f * d[2] + d[4];
  const f32x4 s0 = d[4] - 4.f * d[2], s1 = d[3] - 4.f * d[1];
  o[1] = s0 + s1;
  o[2] = s0 - s1;
  const f32x4 s2 = d[4] - d[2], s3 = 2.f * (d[3] - d[1]);
  o[3] = s2 + s3;
  o[4] = s2 - s3;
  o[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}

// one thread: 4 channels of one tile.  36 16-byte loads (out of the image: an out-of-range offset, zeros), 36 16-byte stores
__global__ __launch_bounds__(256) void wino43_input_kernel(const W43Args a) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned cq4 = (unsigned)a.C >> 2;
  const unsigned r = a.lgq >= 0 ? idx >> a.lgq : idx / cq4, cq = idx - r * cq4;
  if (r >= (unsigned)a.R) return;
  const W43Tile t = w43_tile(a, r);
  const __amdgpu_buffer_rsrc_t xr = dc_rsrc(a.x);
  const unsigned base = (unsigned)t.n * (unsigned)a.ximg + cq * 16u;
  f32x4 v[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int yp = 4 * t.ty - 1 + i, yy = yp * a.d + t.py;
    const bool yok = yp >= 0 && yy < a.H;
    f32x4 row[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int xp = 4 * t.tx - 1 + j, xx = xp * a.d + t.px;
      const bool ok = yok && xp >= 0 && xx < a.W;
      row[j] = dc_bload4(xr, ok ? base + (unsigned)yy * (unsigned)a.xrow + (unsigned)xx * (unsigned)a.xpix : kOOB, 0u);
    }
    w43_bt(row, v[i]);  // d B: along the row
  }
  f32x4* const V = reinterpret_cast<f32x4*>(a.V) + (size_t)r * cq4 + cq;
  const size_t pstride = (size_t)a.R * cq4;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    f32x4 col[6], o[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) col[i] = v[i][j];
    w43_bt(col, o);  // B^T (d B): along the column
#pragma unroll
    for (int i = 0; i < 6; ++i) V[(size_t)(6 * i + j) * pstride] = o[i];
  }
}

// A^T applied to six values -> four
__device__ __forceinline__ void w43_at(const f32x4 (&m)[6], f32x4 (&o)[4]) {
  const f32x4 a0 = m[1] + m[2], a1 = m[1] - m[2], b0 = m[3] + m[4], b1 = m[3] - m[4];
  o[0] = m[0] + a0 + b0;
  o[1] = a1 + 2.f * b1;
  o[2] = a0 + 4.f * b0;
  o[3] = a1 + 8.f * b1 + m[5];
}

// one thread: 4 output channels of one tile.  36 16-byte loads, up to 16 16-byte stores
__global__ __launch_bounds__(256) void wino43_output_kernel(const W43Args a) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned cq4 = (unsigned)a.C >> 2;
  const unsigned r = a.lgq >= 0 ? idx >> a.lgq : idx / cq4, cq = idx - r * cq4;
  if (r >= (unsigned)a.R) return;
  const W43Tile t = w43_tile(a, r);
  const f32x4* const M = reinterpret_cast<const f32x4*>(a.M) + (size_t)r * cq4 + cq;
  const size_t pstride = (size_t)a.R * cq4;
  f32x4 w[4][6];  // A^T M: rows 0..3, columns 0..5
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    f32x4 col[6], o[4];
#pragma unroll
    for (int i = 0; i < 6; ++i) col[i] = M[(size_t)(6 * i + j) * pstride];
    w43_at(col, o);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i][j] = o[i];
  }
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (a.scale) sc = reinterpret_cast<const f32x4*>(a.scale)[cq];
  if (a.shift) sh = reinterpret_cast<const f32x4*>(a.shift)[cq];
  unsigned char* const yb = reinterpret_cast<unsigned char*>(a.y) + (size_t)t.n * (size_t)a.yimg + (size_t)cq * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 o[4];
    w43_at(w[i], o);
    const int yy = (4 * t.ty + i) * a.d + t.py;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = (4 * t.tx + j) * a.d + t.px;
      f32x4 v = o[j] * sc + sh;
      if (a.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      if (yy < a.H && xx < a.W) *reinterpret_cast<f32x4*>(yb + (size_t)yy * (size_t)a.yrow + (size_t)xx * (size_t)a.ypix) = v;
    }
  }
}

int lg2_or_minus1(int v) {
  for (int s = 0; s < 31; ++s)
    if ((1 << s) == v) return s;
  return -1;
}

void w43_geometry(const ConvGemmParams& p, int& TY, int& TX, long& R) {
  const int d = p.ddy;
  TY = ((p.OH + d - 1) / d + 3) / 4, TX = ((p.OW + d - 1) / d + 3) / 4;
  R = (long)p.NB * d * d * TY * TX;
}

W43Args w43_args(const ConvGemmParams& p, long R, int TY, int TX) {
  W43Args a{};
  a.R = (int)R, a.TY = TY, a.TX = TX, a.d = p.ddy, a.H = p.OH, a.W = p.OW;
  a.ximg = (int)(p.x_img_stride * 4), a.xrow = p.x_row_stride * 4, a.xpix = p.sx * 4;
  a.yimg = (int)(p.y_img_stride * 4), a.yrow = p.y_row_stride * 4, a.ypix = p.y_pix_stride * 4;
  a.relu = p.relu;
  return a;
}

constexpr long kWino43MinTiles = 64;

}  // namespace

long wino43_tiles(const ConvGemmParams& p) {
  int TY, TX;
  long R;
  w43_geometry(p, TY, TX, R);
  return R;
}

bool wino43_eligible(const ConvGemmParams& p) {
  if (p.esize != 4 || p.ekind != kElemF32 || !wino_same3x3(p) || p.ddy > 2 || p.resid || p.sigmoid_ch != 0 || p.ncls > 1 || p.nprob > 0) return false;
  const int C = p.klen;
  if ((C != 64 && C != 128 && C != 256 && C != 512) || p.Cout % 64 != 0) return false;
  if ((p.y_pix_stride * 4) % 16 != 0 || (p.y_row_stride * 4) % 16 != 0 || (p.y_img_stride * 4) % 16 != 0 || p.y_pix_stride < p.Cout) return false;
  const long R = wino43_tiles(p);
  // 32-bit offsets: the input through one buffer descriptor, a point's rows of V and M and its filters through the multiply's; the workgroup
  // and thread counts of the three launches
  if ((long)p.NB * p.x_img_stride * 4 >= 0x7fffffffL || (long)p.NB * p.y_img_stride * 4 >= 0x7fffffffL) return false;
  if (R <= 0 || R * C * 4 >= 0x7fffffffL || R * p.Cout * 4 >= 0x7fffffffL || (long)p.Cout * C * 4 >= 0x7fffffffL) return false;
  if (R * (C > p.Cout ? C : p.Cout) / 4 >= 0x7fffffffL || stream1x1f_batched_grid(R, C, p.Cout) <= 0) return false;
  return true;
}

// The per-shape timing tries the form where a layer has kWino43MinTiles tiles (four 16-row steps of the multiply) or more.  The filter image is 36 Cout Cin
// floats, 2.25 x wino_f23's, and every one of them is fetched for R rows of products: below a few steps a launch is the fetch of its filters
// and two more launches, on any load (a 72 x 104 image's res2 layers have 35 tiles, its res4 layers 4).  set_tile takes the form wherever eligible.
bool wino43_offered(const ConvGemmParams& p) { return wino43_tiles(p) >= kWino43MinTiles; }

long wino43_grid(const ConvGemmParams& p) { return stream1x1f_batched_grid(wino43_tiles(p), p.klen, p.Cout); }

size_t wino43_workspace_bytes(const ConvGemmParams& p) { return (size_t)36 * (size_t)wino43_tiles(p) * (size_t)(p.klen + p.Cout) * 4; }

size_t wino43_packed_floats(int Cout, int Cin) { return (size_t)36 * Cout * Cin; }

void wino43_pack_filters(const float* g, int Cout, int Cin, float* out) {
  static const double G[6][3] = {{1.0 / 4, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                 {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
  std::vector<float> U((size_t)36 * Cout * Cin);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci) {
      const float* w = g + ((size_t)co * Cin + ci) * 9;
      double tmp[6][3];
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 3; ++b) tmp[a][b] = G[a][0] * w[b] + G[a][1] * w[3 + b] + G[a][2] * w[6 + b];
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b)
          U[((size_t)(6 * a + b) * Cout + co) * Cin + ci] = (float)(tmp[a][0] * G[b][0] + tmp[a][1] * G[b][1] + tmp[a][2] * G[b][2]);
    }
  for (int p = 0; p < 36; ++p) stream1x1f_pack_filters(U.data() + (size_t)p * Cout * Cin, Cout, Cin, out + (size_t)p * Cout * Cin);
}

int launch_wino43_input(const ConvGemmParams& p, float* V, long R, int TY, int TX, void* stream) {
  W43Args a = w43_args(p, R, TY, TX);
  a.x = p.x, a.V = V, a.C = p.klen, a.lgq = lg2_or_minus1(p.klen / 4);
  const long threads = R * (p.klen / 4);
  hipLaunchKernelGGL(wino43_input_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int launch_wino43_output(const ConvGemmParams& p, const float* M, long R, int TY, int TX, void* stream) {
  W43Args a = w43_args(p, R, TY, TX);
  a.M = M, a.y = p.y, a.scale = p.scale, a.shift = p.shift, a.C = p.Cout, a.lgq = lg2_or_minus1(p.Cout / 4);
  const long threads = R * (p.Cout / 4);
  hipLaunchKernelGGL(wino43_output_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int launch_wino_f43(const ConvGemmParams& p, void* stream) {
  if (!wino43_eligible(p) || !p.form_ws) return (int)hipErrorInvalidValue;
  if (((uintptr_t)p.x & 15) || ((uintptr_t)p.y & 15) || ((uintptr_t)p.w & 15) || ((uintptr_t)p.scale & 15) || ((uintptr_t)p.shift & 15) || ((uintptr_t)p.form_ws & 15))
    return (int)hipErrorInvalidValue;
  int TY, TX;
  long R;
  w43_geometry(p, TY, TX, R);
  float* const V = reinterpret_cast<float*>(p.form_ws);
  float* const M = V + (size_t)36 * R * p.klen;
  int rc = launch_wino43_input(p, V, R, TY, TX, stream);
  if (rc) return rc;
  rc = launch_stream1x1f_batched(V, reinterpret_cast<const float*>(p.w), M, R, p.klen, p.Cout, stream);
  if (rc) return rc;
  return launch_wino43_output(p, M, R, TY, TX, stream);
}

}  // namespace dc
