// layers.hip — the layer kernels beside the convolutions: max-pool, eltwise, crop, NCHW <-> NHWC, float32 -> float16 / bfloat16.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "by_kind.h"
#include "kernels.h"

namespace dc {

// the most negative finite value of T (Caffe's -FLT_MAX start of a max, pooling_layer.cpp:150: rounded into the type's range)
template <typename T>
__device__ __forceinline__ T dc_lowest() {
  if constexpr (std::is_same_v<T, float>) return (T)-3.402823466e+38f;
  else if constexpr (std::is_same_v<T, _Float16>) return (T)-65504.f;
  else return __builtin_bit_cast(T, (unsigned short)0xff7fu);  // -3.3895e38
}

// ------------------------------------------------------------------------------------------------
// MAX pooling (NHWC, 16 bytes of channels per thread), windows clipped to the image
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, int NB, int H, int W,
                                                      int C, int OH, int OW, int k, int s, int pad) {
  constexpr int V = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int cvn = C / V;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)NB * OH * OW * cvn;
  if (idx >= total) return;
  int cv = (int)(idx % cvn);
  long pix = idx / cvn;
  int ox = (int)(pix % OW);
  long t2 = pix / OW;
  int oy = (int)(t2 % OH);
  int n = (int)(t2 / OH);
  int hs = oy * s - pad, ws = ox * s - pad;
  int he = min(hs + k, H), we = min(ws + k, W);  // pooling_layer.cpp:150-155
  hs = max(hs, 0);
  ws = max(ws, 0);
  vec_t m;
#pragma unroll
  for (int q = 0; q < V; ++q) m[q] = dc_lowest<T>();
  for (int iy = hs; iy < he; ++iy)
    for (int ix = ws; ix < we; ++ix) {
      vec_t v = *reinterpret_cast<const vec_t*>(x + (((long)n * H + iy) * W + ix) * C + cv * V);
#pragma unroll
      for (int q = 0; q < V; ++q) m[q] = v[q] > m[q] ? v[q] : m[q];
    }
  *reinterpret_cast<vec_t*>(y + (((long)n * OH + oy) * OW + ox) * C + cv * V) = m;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_scalar_kernel(const T* __restrict__ x, T* __restrict__ y, int NB, int H,
                                                             int W, int C, int OH, int OW, int k, int s, int pad) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)NB * OH * OW * C;
  if (idx >= total) return;
  int c = (int)(idx % C);
  long pix = idx / C;
  int ox = (int)(pix % OW);
  long t2 = pix / OW;
  int oy = (int)(t2 % OH);
  int n = (int)(t2 / OH);
  int hs = oy * s - pad, ws = ox * s - pad;
  int he = min(hs + k, H), we = min(ws + k, W);
  hs = max(hs, 0);
  ws = max(ws, 0);
  float m = -3.402823466e+38f;
  for (int iy = hs; iy < he; ++iy)
    for (int ix = ws; ix < we; ++ix) {
      float v = (float)x[(((long)n * H + iy) * W + ix) * C + c];
      m = v > m ? v : m;
    }
  y[idx] = (T)m;
}

template <typename T>
static int launch_maxpool_t(const void* x, void* y, int NB, int H, int W, int C, int OH, int OW, int k, int s, int pad,
                            void* stream) {
  constexpr int V = 16 / sizeof(T);
  if (C % V == 0) {
    long total = (long)NB * OH * OW * (C / V);
    if (total <= 0) return 0;
    hipLaunchKernelGGL(maxpool_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)x, (T*)y, NB, H, W, C, OH, OW, k, s, pad);
  } else {
    long total = (long)NB * OH * OW * C;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(maxpool_scalar_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const T*)x, (T*)y, NB, H, W, C, OH, OW, k, s, pad);
  }
  return (int)hipGetLastError();
}

int launch_maxpool(const void* x, void* y, int ekind, int NB, int H, int W, int C, int OH, int OW, int k, int s,
                   int pad, void* stream) {
  return dc_by_kind(ekind, [&](auto* tag) {
    return launch_maxpool_t<std::remove_pointer_t<decltype(tag)>>(x, y, NB, H, W, C, OH, OW, k, s, pad, stream);
  });
}

// ------------------------------------------------------------------------------------------------
// stand-alone elementwise: y = act(x*a[c] + b[c] + z)   (arithmetic in float)
// ------------------------------------------------------------------------------------------------
__device__ inline float dc_act(float v, int relu, int sigmoid) {
  if (relu) v = fmaxf(v, 0.f);
  if (sigmoid) v = 1.f / (1.f + expf(-v));
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void eltwise_vec_kernel(const T* __restrict__ x, const T* __restrict__ z,
                                                          const float* __restrict__ a, const float* __restrict__ b,
                                                          T* __restrict__ y, long totalv, int C, int relu, int sigmoid) {
  constexpr int V = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < totalv; i += stride) {
    vec_t v = reinterpret_cast<const vec_t*>(x)[i];
    vec_t zz;
    if (z) zz = reinterpret_cast<const vec_t*>(z)[i];
    int c = (int)((i * V) % C);
    vec_t o;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      float f = (float)v[q];
      if (a) f *= a[c + q];
      if (b) f += b[c + q];
      if (z) f += (float)zz[q];
      o[q] = (T)dc_act(f, relu, sigmoid);
    }
    reinterpret_cast<vec_t*>(y)[i] = o;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void eltwise_scalar_kernel(const T* __restrict__ x, const T* __restrict__ z,
                                                             const float* __restrict__ a, const float* __restrict__ b,
                                                             T* __restrict__ y, long total, int C, int relu,
                                                             int sigmoid) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    float v = (float)x[i];
    int c = (int)(i % C);
    if (a) v *= a[c];
    if (b) v += b[c];
    if (z) v += (float)z[i];
    y[i] = (T)dc_act(v, relu, sigmoid);
  }
}

template <typename T>
static int launch_eltwise_t(const void* x, const void* z, const float* a, const float* b, void* y, long total, int C,
                            int relu, int sigmoid, void* stream) {
  constexpr int V = 16 / sizeof(T);
  if (total <= 0) return 0;
  if (C % V == 0 && total % V == 0) {
    long tv = total / V;
    long blocks = (tv + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(eltwise_vec_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                       (const T*)z, a, b, (T*)y, tv, C, relu, sigmoid);
  } else {
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(eltwise_scalar_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const T*)x, (const T*)z, a, b, (T*)y, total, C, relu, sigmoid);
  }
  return (int)hipGetLastError();
}

int launch_eltwise(const void* x, const void* z, const float* a, const float* b, void* y, int ekind, long total, int C,
                   int relu, int sigmoid, void* stream) {
  return dc_by_kind(ekind, [&](auto* tag) {
    return launch_eltwise_t<std::remove_pointer_t<decltype(tag)>>(x, z, a, b, y, total, C, relu, sigmoid, stream);
  });
}

// ------------------------------------------------------------------------------------------------
// crop (NHWC)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void crop_kernel(const T* __restrict__ x, T* __restrict__ y, int NB, int H, int W,
                                                   int C, int oh, int ow, int OH, int OW) {
  long total = (long)NB * OH * OW * C;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int c = (int)(i % C);
    long pix = i / C;
    int ox = (int)(pix % OW);
    long t2 = pix / OW;
    int oy = (int)(t2 % OH);
    int n = (int)(t2 / OH);
    y[i] = x[(((long)n * H + (oy + oh)) * W + (ox + ow)) * C + c];
  }
}

int launch_crop(const void* x, void* y, int ekind, int NB, int H, int W, int C, int oh, int ow, int OH, int OW,
                void* stream) {
  long total = (long)NB * OH * OW * C;
  if (total <= 0) return 0;
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(crop_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, NB, H, W, C,
                       oh, ow, OH, OW);
    return (int)hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------------------
// NCHW float (Blob side) <-> NHWC float / half (device image) through a 32x32 LDS tile, both sides coalesced
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int C,
                                                           int HW, int CP) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int c = c0 + ty + 8 * k, pix = p0 + tx;
    tile[ty + 8 * k][tx] = (c < C && pix < HW) ? src[((long)n * C + c) * HW + pix] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int pix = p0 + ty + 8 * k, c = c0 + tx;
    if (pix < HW && c < CP) dst[((long)n * HW + pix) * CP + c] = (T)tile[tx][ty + 8 * k];
  }
}

template <typename T, typename D>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* __restrict__ src, D* __restrict__ dst, int C,
                                                           int HW, int CP, int cbase) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int pix = p0 + ty + 8 * k, c = c0 + tx;
    tile[ty + 8 * k][tx] = (pix < HW && c < C) ? (float)src[((long)n * HW + pix) * CP + cbase + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int c = c0 + ty + 8 * k, pix = p0 + tx;
    if (c < C && pix < HW) dst[((long)n * C + c) * HW + pix] = (D)tile[tx][ty + 8 * k];
  }
}

int launch_nchw_to_nhwc(const float* src, void* dst, int ekind, int NB, int C, int H, int W, int CP, void* stream) {
  int HW = H * W;
  if (NB <= 0 || HW <= 0) return 0;
  dim3 grid((HW + 31) / 32, (CP + 31) / 32, NB);
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, src, (T*)dst, C, HW, CP);
    return (int)hipGetLastError();
  });
}

int launch_nhwc_to_nchw(const void* src, void* dst, int ekind, int NB, int C, int H, int W, int CP, int c0,
                        void* stream, int dst_esize) {
  int HW = H * W;
  if (NB <= 0 || HW <= 0) return 0;
  if ((dst_esize != 2 && dst_esize != 4) || (dst_esize == 2 && ekind == kElemF32)) return (int)hipErrorInvalidValue;  // f32 image -> 16-bit copy: not offered
  dim3 grid((HW + 31) / 32, (C + 31) / 32, NB);
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    if (dst_esize == 2)
      hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, T>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)src, (T*)dst, C, HW, CP, c0);
    else
      hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, float>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)src, (float*)dst, C, HW, CP, c0);
    return (int)hipGetLastError();
  });
}

// float -> half conversion of a packed filter image (upload path of fp16 nets)
__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, long n) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = (_Float16)src[i];
}
int launch_f32_to_f16(const float* src, void* dst, long n, void* stream) {
  if (n <= 0) return 0;
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, (_Float16*)dst, n);
  return (int)hipGetLastError();
}
// ... and to bfloat16 (bf16 nets): round to nearest even, NaN stays NaN (v_cvt_pk_bf16_f32)
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, long n) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = (__bf16)src[i];
}
int launch_f32_to_bf16(const float* src, void* dst, long n, void* stream) {
  if (n <= 0) return 0;
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, (__bf16*)dst, n);
  return (int)hipGetLastError();
}

}  // namespace dc
