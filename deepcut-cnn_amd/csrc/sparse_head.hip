// sparse_head.hip — the pairwise head (`next_pred`) evaluated at a list of cells only (gfx950): DC_OPT_SPARSE_PAIRWISE.
//
// Bottom-up people reads `next_pred` at the part candidates' cells and nowhere else (people.hip), a few hundred of the 6 256 cells of a
// 544x736 forward, so a net that leaves `next_pred` out of its plan (DC_OPT_OUTPUTS) can have the head computed at those cells alone.
// The rule is stated in include/deepcut_hip.h (dc_net_pairwise_at): per cell, the 1x1 skip convolution of X3 plus the 1, 2 or 4 taps
// of the stride-2 3x3 deconvolution of X5 that the parity of (row + oh, col + ow) selects.
//
// Two launches:
//   sparse_cells_kernel  one workgroup: the cells (part_select's candidates, or a list of (image, row, col)) sorted into the four
//                        parity classes by a prefix count, in slot order
//   sparse_head_kernel   grid (32-channel chunk, class): a gather-GEMM on v_mfma_f32_32x32x2_f32.  Rows = the class's cells, K = the
//                        skip's channels followed by the channels of every tap of the class, columns = the chunk's 32 channels.  The
//                        8 waves of a workgroup split K (wave w takes the 8-channel blocks j = w, w + 8, ...) and hold up to 4 row
//                        tiles of 32 cells each, so a filter fragment is loaded once per 128 cells: the usual few hundred cells read
//                        every filter byte of their class once.  The waves' partial sums are added in LDS in wave order.
// No float atomics: a cell's value is one fixed chain of fused multiply-adds (k ascending inside a wave's share, then waves 0..7, then
// the bias), whatever its place in the list, whoever else is in it.  A cell listed twice is computed twice and stored twice, the same bits.
//
// The filter image (sparse_head_pack_filters; ModelShared::vec_by_key): float32, [segment][chunk][K block of 8][64 lanes][4], segment
// t = ky*3 + kx for the deconvolution's nine taps (K = K5) and 9 for the skip (K = K3), K rounded up to 8 and Cout to 32 with zeros.
// Lane l of K block j holds W[k = 8j + 4(l / 32) + m][n = 32 chunk + l % 32] for m = 0..3: one 16-byte load per lane feeds four MFMAs,
// whose A operand is element m of the 4 consecutive channels the lane loaded of its cell.  16-bit nets: the same image with every filter
// rounded to the net's type and widened again (launch_round_through), activations widened on the way in; products and sums are float32.
#include <hip/hip_runtime.h>

#include "by_kind.h"
#include "kernels.h"

namespace dc {

namespace {

typedef float sh_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kShWaves = 8;      // waves per workgroup = the K split
constexpr int kShRowTiles = 4;   // 32-cell row tiles a wave accumulates at a time
constexpr int kShRowGroups = 4;  // grid.z: workgroups that share a class's cells, 128 at a time each (all but the first leave at once below 129 cells)

// 4 consecutive channels [k, k + 4) of one cell as float32: channels at or beyond K read as 0
template <typename T>
__device__ __forceinline__ float4 sh_load4(const T* __restrict__ p, int k, int K, bool vec) {
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {  // K % 4 == 0 and 4-element alignment: the group is inside or outside as a whole
    if (k < K) {
      if constexpr (sizeof(T) == 4) {
        r = *reinterpret_cast<const float4*>(p + k);
      } else {
        struct alignas(8) Four {
          T v[4];
        };
        const Four q = *reinterpret_cast<const Four*>(p + k);
        r = make_float4((float)q.v[0], (float)q.v[1], (float)q.v[2], (float)q.v[3]);
      }
    }
  } else {
    if (k < K) r.x = (float)p[k];
    if (k + 1 < K) r.y = (float)p[k + 1];
    if (k + 2 < K) r.z = (float)p[k + 2];
    if (k + 3 < K) r.w = (float)p[k + 3];
  }
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void round_through_kernel(float* __restrict__ p, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = (float)(T)p[i];
}

// one wave's share of one segment for NT row tiles: per K block of 8 one 16-byte filter load and NT 4-channel activation loads feed 4 NT
// MFMAs.  The loop is latency bound (two waves per SIMD, every load a trip to HBM or L2), so four K blocks are requested before the first
// is multiplied; the blocks are still multiplied in ascending order: the value does not depend on the batching.
template <typename T, int NT>
__device__ __forceinline__ void sh_block(sh_f32x16 (&acc)[NT], const float4& b4, const float4 (&a4)[NT]) {
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ti].x, b4.x, acc[ti], 0, 0, 0);
    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ti].y, b4.y, acc[ti], 0, 0, 0);
    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ti].z, b4.z, acc[ti], 0, 0, 0);
    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ti].w, b4.w, acc[ti], 0, 0, 0);
  }
}

template <typename T, int NT>
__device__ __forceinline__ void sh_segment(sh_f32x16 (&acc)[NT], const T* const (&src)[NT], const float* __restrict__ wseg,
                                           int nkb, int K, bool vec, int wv, int lane) {
  constexpr int U = NT <= 2 ? 4 : 2;  // K blocks in flight: what the registers hold beside NT accumulators  // K blocks in flight: what the registers hold beside NT accumulators without spilling
  const int kk4 = 4 * (lane >> 5);
  int j = wv;
  for (; j + (U - 1) * kShWaves < nkb; j += U * kShWaves) {
    float4 b4[U], a4[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) b4[u] = *reinterpret_cast<const float4*>(wseg + ((long)(j + u * kShWaves) * 64 + lane) * 4);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
        a4[u][ti] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src[ti]) a4[u][ti] = sh_load4(src[ti], 8 * (j + u * kShWaves) + kk4, K, vec);
      }
#pragma unroll
    for (int u = 0; u < U; ++u) sh_block<T, NT>(acc, b4[u], a4[u]);
  }
  for (; j < nkb; j += kShWaves) {
    const float4 b4 = *reinterpret_cast<const float4*>(wseg + ((long)j * 64 + lane) * 4);
    float4 a4[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      a4[ti] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src[ti]) a4[ti] = sh_load4(src[ti], 8 * j + kk4, K, vec);
    }
    sh_block<T, NT>(acc, b4, a4);
  }
}

}  // namespace

// Slot s of the input is a cell or nothing.  Candidates (dets != null): s = list * MD + i with list = image * J + joint, a cell when
// i < min(counts[list], MD), at (row, col) = dets[s*5 + 3], dets[s*5 + 4].  Triples (cells != null): s = entry s of [n][3] (image, row,
// col).  A cell outside the map is nothing.  Class q = 2 * ((row + oh) & 1) + ((col + ow) & 1); work[q] = the class's count,
// work[4 + q * cap + i] = the linear cell index (image * H + row) * W + col of its i-th member, members in slot order.
__global__ __launch_bounds__(256) void sparse_cells_kernel(const int* __restrict__ counts, const double* __restrict__ dets, int J, int MD,
                                                           const int* __restrict__ cells, int n, int NB, int H, int W, int oh, int ow, int cap,
                                                           int* __restrict__ work) {
  __shared__ int wave_cnt[4][4];  // [wave][class]
  __shared__ int base[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 4) base[t] = 0;
  __syncthreads();
  for (int s0 = 0; s0 < n; s0 += 256) {
    const int s = s0 + t;
    int q = -1, cell = 0;
    if (s < n) {
      int b = -1, r = -1, c = -1;
      if (dets) {
        const int list = s / MD, i = s - list * MD;
        if (i < min(counts[list], MD)) b = list / J, r = (int)dets[(long)s * 5 + 3], c = (int)dets[(long)s * 5 + 4];
      } else {
        b = cells[(long)s * 3], r = cells[(long)s * 3 + 1], c = cells[(long)s * 3 + 2];
      }
      if (b >= 0 && b < NB && r >= 0 && r < H && c >= 0 && c < W) q = ((r + oh) & 1) * 2 + ((c + ow) & 1), cell = (b * H + r) * W + c;
    }
    int rank = 0;
    for (int k = 0; k < 4; ++k) {
      const unsigned long long m = __ballot(q == k);
      if (q == k) rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wave_cnt[wv][k] = __popcll(m);
    }
    __syncthreads();
    if (q >= 0) {
      int off = base[q];
      for (int w2 = 0; w2 < wv; ++w2) off += wave_cnt[w2][q];
      if (off + rank < cap) work[4 + (long)q * cap + off + rank] = cell;
    }
    __syncthreads();
    if (t < 4) base[t] += wave_cnt[0][t] + wave_cnt[1][t] + wave_cnt[2][t] + wave_cnt[3][t];
    __syncthreads();
  }
  if (t < 4) work[t] = min(base[t], cap);
}

// One pass of a workgroup: NT row tiles (the class's cells base .. base + 32 NT - 1) against the chunk's 32 channels, over every segment
// of the class; then the waves' shares of K are added in wave order — ((w0 + w1) + ... + w6) in LDS, the last wave adds its own and the
// bias and stores.
template <typename T, int NT>
__device__ __forceinline__ void sh_pass(const SparseHeadArgs& p, const int* __restrict__ list, int cnt, int base, int chunk, int nchunk, int q,
                                        float* __restrict__ red) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 31, kk = lane >> 5;
  const int pr = q >> 1, pc = q & 1;
  const int nkb5 = (p.K5 + 7) / 8, nkb3 = (p.K3 + 7) / 8;
  const T* __restrict__ x3 = (const T*)p.x3;
  const T* __restrict__ x5 = (const T*)p.x5;
  const int HW = p.H * p.W;
  int cell[NT];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int row = base + 32 * ti + lr;
    cell[ti] = row < cnt ? list[row] : -1;
  }
  sh_f32x16 acc[NT];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[ti][v] = 0.f;
  // segment 0 = the skip; 1..4 = the taps (ky, kx) of the class: ky in {0, 2} for an even row + oh, {1} for an odd one, kx alike
#pragma unroll 1
  for (int sg = 0; sg < 5; ++sg) {
    int ky = 0, kx = 0;
    if (sg > 0) {
      const int a = (sg - 1) >> 1, bb = (sg - 1) & 1;
      if ((pr && a) || (pc && bb)) continue;
      ky = pr ? 1 : 2 * a, kx = pc ? 1 : 2 * bb;
    }
    const int K = sg ? p.K5 : p.K3, nkb = sg ? nkb5 : nkb3;
    const bool vec = sg ? p.vec5 : p.vec3;
    const int seg = sg ? ky * 3 + kx : 9;
    const float* __restrict__ wseg = p.wimg + ((long)seg * nchunk * nkb5 + (long)chunk * nkb) * 256;
    const T* src[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      src[ti] = nullptr;
      if (cell[ti] < 0) continue;
      if (sg == 0) {
        src[ti] = x3 + (long)cell[ti] * p.cp3;
      } else {
        const int b = cell[ti] / HW, rc = cell[ti] - b * HW, r = rc / p.W, c = rc - r * p.W;
        const int ty = r + p.oh - ky, tx = c + p.ow - kx;  // even where they are >= 0: the class's parity
        if (ty >= 0 && tx >= 0 && (ty >> 1) < p.h5 && (tx >> 1) < p.w5) src[ti] = x5 + (((long)b * p.h5 + (ty >> 1)) * p.w5 + (tx >> 1)) * p.cp5;
      }
    }
    sh_segment<T, NT>(acc, src, wseg, nkb, K, vec, wv, lane);
  }
  for (int w = 0; w < kShWaves - 1; ++w) {
    if (wv == w) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int idx = (ti * 16 + v) * 64 + lane;
          red[idx] = w ? red[idx] + acc[ti][v] : acc[ti][v];
        }
    }
    __syncthreads();
  }
  if (wv == kShWaves - 1) {
    const int ch = chunk * 32 + lr;
    const float bias = ch < p.Cout ? p.bias[ch] : 0.f;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = base + 32 * ti + 8 * (v >> 2) + 4 * kk + (v & 3);  // C/D map of the 32x32 MFMA: column = lane & 31
        if (row < cnt && ch < p.Cout) p.out[(long)list[row] * p.Cout + ch] = (red[(ti * 16 + v) * 64 + lane] + acc[ti][v]) + bias;
      }
  }
  __syncthreads();  // the next pass reuses `red`
}

template <typename T>
__global__ __launch_bounds__(kShWaves * 64) void sparse_head_kernel(SparseHeadArgs p, const int* __restrict__ work, int cap) {
  __shared__ float red[kShRowTiles * 16 * 64];
  const int chunk = blockIdx.x, q = blockIdx.y;
  const int cnt = work[q];
  if (cnt <= 0) return;  // the same for the whole workgroup
  const int* __restrict__ list = work + 4 + (long)q * cap;
  for (int base = blockIdx.z * 32 * kShRowTiles; base < cnt; base += gridDim.z * 32 * kShRowTiles) {
    const int ntile = min(kShRowTiles, (cnt - base + 31) / 32);  // uniform
    if (ntile == 1) sh_pass<T, 1>(p, list, cnt, base, chunk, gridDim.x, q, red);
    else if (ntile == 2) sh_pass<T, 2>(p, list, cnt, base, chunk, gridDim.x, q, red);
    else if (ntile == 3) sh_pass<T, 3>(p, list, cnt, base, chunk, gridDim.x, q, red);
    else sh_pass<T, 4>(p, list, cnt, base, chunk, gridDim.x, q, red);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void map_gather_kernel(const T* __restrict__ map, int cp, int c0, int H, int W, int C, int ndet,
                                                         const int* __restrict__ det, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)ndet * C) return;
  const int d = (int)(i / C), ch = (int)(i - (long)d * C);
  const int n = det[3 * d], row = det[3 * d + 1], col = det[3 * d + 2];
  out[i] = (float)map[(((long)n * H + row) * W + col) * cp + c0 + ch];
}

int launch_map_gather(const void* map, int cp, int c0, int ekind, int H, int W, int C, int ndet, const int* det, float* out, void* stream) {
  const long total = (long)ndet * C;
  if (total <= 0) return 0;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(map_gather_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)map, cp, c0, H, W, C,
                       ndet, det, out);
    return (int)hipGetLastError();
  });
}

size_t sparse_head_image_floats(int cout, int k3, int k5) {
  const size_t nchunk = (size_t)(cout + 31) / 32, nkb3 = (size_t)(k3 + 7) / 8, nkb5 = (size_t)(k5 + 7) / 8;
  return nchunk * 256 * (9 * nkb5 + nkb3);
}

void sparse_head_pack_filters(const float* ws, const float* wd, int cout, int k3, int k5, float* out) {
  const int nchunk = (cout + 31) / 32, nkb3 = (k3 + 7) / 8, nkb5 = (k5 + 7) / 8;
  for (int seg = 0; seg < 10; ++seg) {
    const int K = seg < 9 ? k5 : k3, nkb = seg < 9 ? nkb5 : nkb3;
    float* o = out + (size_t)seg * nchunk * nkb5 * 256;
    for (int ch = 0; ch < nchunk; ++ch)
      for (int j = 0; j < nkb; ++j)
        for (int l = 0; l < 64; ++l)
          for (int m = 0; m < 4; ++m) {
            const int k = 8 * j + 4 * (l >> 5) + m, n = 32 * ch + (l & 31);
            float v = 0.f;
            if (k < K && n < cout) v = seg < 9 ? wd[((size_t)k * cout + n) * 9 + seg] : ws[(size_t)n * k3 + k];
            o[(((size_t)ch * nkb + j) * 64 + l) * 4 + m] = v;
          }
  }
}

int launch_round_through(float* p, long n, int ekind, void* stream) {
  if (n <= 0 || ekind == kElemF32) return 0;
  const long blocks = std::min<long>((n + 255) / 256, 4096);
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(round_through_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n);
    return (int)hipGetLastError();
  });
}

int launch_sparse_head(const SparseHeadArgs& a, int ekind, const int* counts, const double* dets, int J, int MD, const int* cells, int n,
                       int* work, void* stream) {
  if (n <= 0) return 0;
  if (!dets == !cells || (dets && (!counts || J < 1 || MD < 1)) || !a.x3 || !a.x5 || !a.wimg || !a.bias || !a.out || !work || a.Cout < 1 ||
      a.K3 < 1 || a.K5 < 1 || a.NB < 1 || a.H < 1 || a.W < 1 || a.h5 < 1 || a.w5 < 1 || a.oh < 0 || a.ow < 0 || a.cp3 < a.K3 || a.cp5 < a.K5 ||
      (long)a.NB * a.H * a.W > 0x7fffffffL)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sparse_cells_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, dets, J, MD, cells, n, a.NB, a.H, a.W, a.oh, a.ow, n,
                     work);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(sparse_head_kernel<T>, dim3((unsigned)((a.Cout + 31) / 32), 4, kShRowGroups), dim3(kShWaves * 64), 0, (hipStream_t)stream, a, work, n);
    return (int)hipGetLastError();
  });
}

}  // namespace dc
