// pose.hip — what reads the net's maps on the device: pose decode, part candidates, pairwise regression decode, multi-scale fusion.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "by_kind.h"
#include "kernels.h"

namespace dc {

// ------------------------------------------------------------------------------------------------
// pose decode on the device (estimate_pose.py:131-143 `_pose_from_mats`): per joint the FIRST maximum of
// the score map in row-major order, refined by the location-regression vector at that cell.  One block
// per (image, joint); only 5 x J doubles per image leave the GPU instead of the maps.
// ------------------------------------------------------------------------------------------------
// `items` (launch_pose_decode_items): image n's own scale, offset and valid cells [0, rows) x [0, cols); the region is walked in
// row-major order, so the first maximum is the restricted map's first maximum.
template <typename T>
__global__ __launch_bounds__(256) void pose_decode_kernel(const T* __restrict__ prob, int pcp, int pc0,
                                                          const T* __restrict__ loc, int lcp, int lc0, int H, int W,
                                                          int J, double scale, const PoseDecodeItem* __restrict__ items,
                                                          double* __restrict__ out) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int j = blockIdx.x, n = blockIdx.y, HW = H * W;
  int rows = H, cols = W;
  if (items) {
    const PoseDecodeItem& it = items[n];
    rows = min(it.rows, H), cols = min(it.cols, W), scale = it.scale;
  }
  const int cnt = rows * cols;
  float best = -3.402823466e+38f;
  int bi = 0x7fffffff;
  for (int q = threadIdx.x; q < cnt; q += 256) {
    const int p = cols == W ? q : (q / cols) * W + (q % cols);
    const float v = (float)prob[((long)n * HW + p) * pcp + pc0 + j];
    if (v > best) best = v, bi = p;  // strided scan keeps the smallest index per thread
  }
  sv[threadIdx.x] = best;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const float v2 = sv[threadIdx.x + s];
      const int i2 = si[threadIdx.x + s];
      if (v2 > sv[threadIdx.x] || (v2 == sv[threadIdx.x] && i2 < si[threadIdx.x])) {
        sv[threadIdx.x] = v2;
        si[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int p = si[0] == 0x7fffffff ? 0 : si[0];
    const int row = p / W, col = p - row * W;
    const double kLoc = 7.280109889280518;  // sqrt(53)  (_LOCREF_SCALE_MUL, estimate_pose.py:27)
    const double ox = (double)(float)loc[((long)n * HW + p) * lcp + lc0 + 2 * j];
    const double oy = (double)(float)loc[((long)n * HW + p) * lcp + lc0 + 2 * j + 1];
    double* o = out + (long)n * 5 * J;
    o[0 * J + j] = ((double)col * 8.0 + 4.0 + ox * kLoc) / scale;
    o[1 * J + j] = ((double)row * 8.0 + 4.0 + oy * kLoc) / scale;
    if (items) o[0 * J + j] += items[n].dx, o[1 * J + j] += items[n].dy;
    o[2 * J + j] = (double)(float)prob[((long)n * HW + p) * pcp + pc0 + j];
    o[3 * J + j] = oy * kLoc / scale;
    o[4 * J + j] = ox * kLoc / scale;
  }
}

int launch_pose_decode(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, int NB, int H,
                       int W, int J, double scale, double* out, void* stream) {
  if (NB <= 0 || J <= 0) return 0;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(pose_decode_kernel<T>, dim3(J, NB), dim3(256), 0, (hipStream_t)stream, (const T*)prob, pcp, pc0, (const T*)loc, lcp,
                       lc0, H, W, J, scale, (const PoseDecodeItem*)nullptr, out);
    return (int)hipGetLastError();
  });
}

int launch_pose_decode_items(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, int NB, int H,
                             int W, int J, const PoseDecodeItem* items, double* out, void* stream) {
  if (NB <= 0 || J <= 0) return 0;
  if (!items) return (int)hipErrorInvalidValue;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(pose_decode_kernel<T>, dim3(J, NB), dim3(256), 0, (hipStream_t)stream, (const T*)prob, pcp, pc0, (const T*)loc, lcp,
                       lc0, H, W, J, 1.0, items, out);
    return (int)hipGetLastError();
  });
}

// ---- multi-person consumers: part candidates (NMS) and pairwise regression decode ------------------------------------
// One workgroup per (image, joint) score map.  Every cell is tested for being the maximum of its (2r+1)^2 window (ties: the
// lower cell index wins) and, if so, becomes the 64-bit key (score bits without the sign << 32 | ~cell): keys are unique, and descending key
// order IS the output order (score descending, cell ascending).  The candidate SET does not depend on thread timing, and
// the list is then ordered by the whole workgroup: up to kPartLds keys by a bitonic sort in LDS; a map with more local
// maxima than that (threshold 0, radius 0) spills its keys to global memory and takes the first max_det by repeated
// workgroup-wide maximum.  Nothing is dropped in arrival order, so the result is deterministic for every input.
constexpr int kPartLds = 4096;  // keys sorted in LDS (32 KB)

template <typename T>
__global__ __launch_bounds__(256) void part_select_kernel(const T* __restrict__ prob, int pcp, int pc0, const T* __restrict__ loc, int lcp,
                                                          int lc0, int H, int W, int J, float thr, int radius, double scale, int max_det,
                                                          unsigned long long* __restrict__ spill, int* __restrict__ counts,
                                                          double* __restrict__ out) {
  __shared__ unsigned long long keys[kPartLds];
  __shared__ unsigned long long red[256];
  __shared__ int cnt;
  const int nj = blockIdx.x, n = nj / J, j = nj - n * J, t = threadIdx.x, HW = H * W;
  const T* base = prob + ((long)n * HW) * pcp + pc0 + j;
  unsigned long long* mine = spill + (long)nj * HW;
  if (t == 0) cnt = 0;
  __syncthreads();
  for (int cell = t; cell < HW; cell += 256) {
    const int row = cell / W, col = cell - row * W;
    const float v = (float)base[(long)cell * pcp];
    bool ok = v >= thr;
    for (int dy = -radius; ok && dy <= radius; ++dy) {
      const int y = row + dy;
      if (y < 0 || y >= H) continue;
      for (int dx = -radius; dx <= radius; ++dx) {
        const int x = col + dx;
        if (x < 0 || x >= W || (dy == 0 && dx == 0)) continue;
        const float u = (float)base[((long)y * W + x) * pcp];
        if (u > v || (u == v && y * W + x < cell)) {
          ok = false;
          break;
        }
      }
    }
    if (ok) {
      // the bit pattern orders NON-NEGATIVE floats only (a set sign bit would sort above every positive score).  Here v >= thr >= 0
      // (detect_parts refuses a negative threshold), which leaves one value with the sign bit set: -0.0 at threshold 0 (a blob written
      // by a caller may hold it; a sigmoid never does).  The sign bit is cleared, so -0.0 sorts with the zeros, by cell, and is emitted
      // as +0.0; every positive score keeps its bits.  Key 0 (the padding) stays below every candidate: the cell term is > 0.
      const unsigned long long key = ((unsigned long long)(__float_as_uint(v) & 0x7fffffffu) << 32) | (unsigned)(0xffffffffu - (unsigned)cell);
      const int slot = atomicAdd(&cnt, 1);  // LDS counter: the slot order varies, the set and (after sorting) the result do not
      if (slot < kPartLds) keys[slot] = key;
      mine[slot] = key;
    }
  }
  __syncthreads();
  const int m = cnt;
  const int take = min(m, max_det);
  if (t == 0) counts[nj] = take;
  double* o = out + (long)nj * max_det * 5;
  auto emit = [&](int k, unsigned long long key) {
    const double kLoc = 7.280109889280518;  // sqrt(53)
    const int cell = (int)(0xffffffffu - (unsigned)key);
    const int row = cell / W, col = cell - row * W;
    const T* l = loc + (((long)n * H + row) * W + col) * lcp + lc0 + 2 * j;
    double* q = o + (long)k * 5;
    q[0] = ((double)col * 8.0 + 4.0 + (double)(float)l[0] * kLoc) / scale;
    q[1] = ((double)row * 8.0 + 4.0 + (double)(float)l[1] * kLoc) / scale;
    q[2] = (double)__uint_as_float((unsigned)(key >> 32));
    q[3] = (double)row;
    q[4] = (double)col;
  };
  for (int k = take + t; k < max_det; k += 256) {
    double* q = o + (long)k * 5;
    q[0] = q[1] = q[2] = 0.0;
    q[3] = q[4] = -1.0;
  }
  if (m <= kPartLds) {
    int P = 1;
    while (P < m) P <<= 1;
    for (int i = m + t; i < P; i += 256) keys[i] = 0ull;  // below every real key (scores >= 0, cell term > 0)
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
      for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
        for (int i = t; i < P; i += 256) {
          const int ixj = i ^ j2;
          if (ixj > i) {
            const unsigned long long a = keys[i], b = keys[ixj];
            const bool desc = (i & k2) == 0;  // descending overall
            if (desc ? a < b : a > b) keys[i] = b, keys[ixj] = a;
          }
        }
        __syncthreads();
      }
    for (int k = t; k < take; k += 256) emit(k, keys[k]);
  } else {
    __threadfence_block();
    unsigned long long prev = ~0ull;
    for (int k = 0; k < take; ++k) {  // k-th largest key = the largest key below the previous one
      unsigned long long best = 0ull;
      for (int i = t; i < m; i += 256) {
        const unsigned long long v = mine[i];
        if (v < prev && v > best) best = v;
      }
      red[t] = best;
      __syncthreads();
      for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (t < s2 && red[t + s2] > red[t]) red[t] = red[t + s2];
        __syncthreads();
      }
      prev = red[0];
      if (t == 0) emit(k, prev);
      __syncthreads();
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pairwise_decode_kernel(const T* __restrict__ next, int ncp, int nc0, int NB, int H, int W, int E,
                                                              double scale, int ndet, const int* __restrict__ det,
                                                              const double* __restrict__ mean, const double* __restrict__ stdev,
                                                              double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)ndet * E) return;
  const int d = (int)(i / E), l = (int)(i - (long)d * E);
  const int n = det[3 * d], row = det[3 * d + 1], col = det[3 * d + 2];
  double* o = out + i * 2;
  if (n < 0 || n >= NB || row < 0 || row >= H || col < 0 || col >= W) {
    o[0] = o[1] = 0.0;
    return;
  }
  const T* p = next + (((long)n * H + row) * W + col) * ncp + nc0 + 2 * l;
  const double m0 = mean ? mean[2 * l] : 0.0, m1 = mean ? mean[2 * l + 1] : 0.0;
  const double s0 = stdev ? stdev[2 * l] : 1.0, s1 = stdev ? stdev[2 * l + 1] : 1.0;
  o[0] = ((double)col * 8.0 + 4.0 + (double)(float)p[0] * s0 + m0) / scale;
  o[1] = ((double)row * 8.0 + 4.0 + (double)(float)p[1] * s1 + m1) / scale;
}

// ---- multi-scale fusion of a pyramid's maps (the rule: include/deepcut_hip.h, dc_group_fuse_maps and dc_group_fuse_maps_mirrored; this
// project's own) -----------------------------------------------------------------------------------------------------------------------
// One workgroup per base cell (image, row, column), lanes along the channels of the three maps laid end to end: the maps are NHWC, so
// each corner read of a member and the store are contiguous runs of a wave.  The cell's sample position in every member — four corner
// cells and two weights — is computed once, by the thread of that member's index, and kept in LDS; the channel loop (406 channels of the
// full heads: two trips of 256) only reads it.  Members are summed in ascending order by every thread: nothing depends on timing.
// One body, two instantiations.  Mirror = false reads neither `flip` nor `src`.  Mirror = true differs in two expressions: a member that
// saw the image flipped left to right is sampled at the reflected column, and lane ch reads the member's channel src[m][ch] of the same
// map (left and right joints swapped, the regression edge replaced by its mirror image), with the sign change of the x components
// folded into the gain / bias table.  A corner read is then no longer one ascending run of the wave but a permutation of it INSIDE the
// same map, i.e. inside the same cache lines (14 / 28 / 364 channels of 2 or 4 bytes: 1 + 1 + 6 to 12 lines of 128 bytes per corner
// either way), and the store stays a contiguous run.  The flag is compile-time so that a group without a mirrored member pays no
// dependent integer load per member and channel.  The flip record is per (member, image): every box of the box entry has its own width
// and scale, so its reflected column is its own; the clamp stays at the member's whole map (the common canvas).
struct FuseCorner {
  int i00, i01, i10, i11;  // cell indices (y * W + x) of the four corners in the member's map
  float fx, fy;
};

__device__ __forceinline__ double fuse_mirrored_u(double ws, int c, double q) {
#pragma clang fp contract(off)  // the rule's own order: a product, two differences, a quotient
  const double a = (double)(8 * c + 4) * q;
  const double d = ws - a;
  return (d - 4.0) / 8.0;
}

template <typename T, bool Mirror>
__global__ __launch_bounds__(256) void fuse_maps_kernel(const FuseMember* __restrict__ members, const FuseFlip* __restrict__ flip,
                                                        const float* __restrict__ gain, const float* __restrict__ bias,
                                                        const int* __restrict__ src, int M, int Hb, int Wb, int C0, int C1, int Ctot,
                                                        float inv_m, float* __restrict__ out) {
  extern __shared__ FuseCorner fuse_lds[];  // [M]
  const int cell = blockIdx.x, t = threadIdx.x;
  const int b = cell / (Hb * Wb), rc = cell - b * (Hb * Wb), r = rc / Wb, c = rc - r * Wb;
  for (int m = t; m < M; m += 256) {
    const FuseMember& mem = members[m];
    const double q = mem.q;
    bool flipped = false;
    double ws = 0.0;
    if constexpr (Mirror) {  // the record of (member, image): one workgroup per cell, so the grid is NB * Hb * Wb
      const FuseFlip& ff = flip[(long)m * (gridDim.x / (unsigned)(Hb * Wb)) + b];
      flipped = ff.on, ws = ff.ws;
    }
    double u = flipped ? fuse_mirrored_u(ws, c, q) : ((double)(8 * c + 4) * q - 4.0) / 8.0;
    double v = ((double)(8 * r + 4) * q - 4.0) / 8.0;
    u = fmin(fmax(u, 0.0), (double)(mem.W - 1));
    v = fmin(fmax(v, 0.0), (double)(mem.H - 1));
    const int x0 = (int)floor(u), y0 = (int)floor(v);
    const int x1 = min(x0 + 1, mem.W - 1), y1 = min(y0 + 1, mem.H - 1);
    FuseCorner k;
    k.i00 = y0 * mem.W + x0, k.i01 = y0 * mem.W + x1, k.i10 = y1 * mem.W + x0, k.i11 = y1 * mem.W + x1;
    k.fx = (float)(u - (double)x0), k.fy = (float)(v - (double)y0);
    fuse_lds[m] = k;
  }
  __syncthreads();
  float* o = out + (long)cell * Ctot;
  for (int ch = t; ch < Ctot; ch += 256) {
    const int k = ch < C0 ? 0 : ch < C1 ? 1 : 2;
    const int cc = ch - (k == 0 ? 0 : k == 1 ? C0 : C1);
    float acc = 0.f;
    for (int m = 0; m < M; ++m) {
      const FuseMember& mem = members[m];
      const FuseCorner kc = fuse_lds[m];
      const long cp = mem.cp[k];
      int sc = cc;  // the channel within map k that this lane reads from member m
      if constexpr (Mirror) sc = src[(long)m * Ctot + ch];
      const T* p = (const T*)mem.ptr[k] + (long)b * mem.H * mem.W * cp + mem.c0[k] + sc;
      const float a00 = (float)p[kc.i00 * cp], a01 = (float)p[kc.i01 * cp], a10 = (float)p[kc.i10 * cp], a11 = (float)p[kc.i11 * cp];
      const float val = (1.f - kc.fy) * ((1.f - kc.fx) * a00 + kc.fx * a01) + kc.fy * ((1.f - kc.fx) * a10 + kc.fx * a11);
      acc += val * gain[(long)m * Ctot + ch] + bias[(long)m * Ctot + ch];
    }
    o[ch] = acc * inv_m;
  }
}

int launch_fuse_maps(const FuseMember* members, const FuseFlip* flip, const float* gain, const float* bias, const int* src, int M, int ekind,
                     int NB, int Hb, int Wb, const int C[3], float* out, void* stream) {
  const int Ctot = C[0] + C[1] + C[2];
  const long cells = (long)NB * Hb * Wb;
  if (cells <= 0 || Ctot <= 0) return 0;
  if (M < 1 || M > 1024 || cells > 0x7fffffffL || C[0] < 0 || C[1] < 0 || C[2] < 0 || !flip != !src) return (int)hipErrorInvalidValue;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto* kernel = flip ? fuse_maps_kernel<T, true> : fuse_maps_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)cells), dim3(256), (size_t)M * sizeof(FuseCorner), (hipStream_t)stream, members, flip, gain, bias,
                       src, M, Hb, Wb, C[0], C[0] + C[1], Ctot, 1.f / (float)M, out);
    return (int)hipGetLastError();
  });
}

int launch_part_select(const void* prob, int pcp, int pc0, const void* loc, int lcp, int lc0, int ekind, int NB, int H, int W, int J, float thr,
                       int radius, double scale, int max_det, unsigned long long* spill, int* counts, double* out, void* stream) {
  if (NB * J <= 0) return 0;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(part_select_kernel<T>, dim3(NB * J), dim3(256), 0, (hipStream_t)stream, (const T*)prob, pcp, pc0, (const T*)loc, lcp,
                       lc0, H, W, J, thr, radius, scale, max_det, spill, counts, out);
    return (int)hipGetLastError();
  });
}

int launch_pairwise_decode(const void* next, int ncp, int nc0, int ekind, int NB, int H, int W, int E, double scale, int ndet,
                           const int* det, const double* mean, const double* stdev, double* out, void* stream) {
  const long total = (long)ndet * E;
  if (total <= 0) return 0;
  const dim3 grid((unsigned)((total + 255) / 256));
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(pairwise_decode_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)next, ncp, nc0, NB, H, W, E, scale, ndet,
                       det, mean, stdev, out);
    return (int)hipGetLastError();
  });
}

}  // namespace dc
