// image_prep.hip — image and person-box pre-processing on the device: resample, mean / layout / element type, box crops.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "by_kind.h"
#include "kernels.h"

namespace dc {

// ---- image pre-processing -----------------------------------------------------------------------------------------
// Integer work at a few bytes per pixel: HBM/latency-bound, one thread per output pixel, no LDS.
__device__ __forceinline__ int clip8_fixed(int acc) {
  const int v = acc >> 22;  // PRECISION_BITS = 32 - 8 - 2 (Pillow Resample.c)
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- source-pixel readers (kernels.h kRead*) -------------------------------------------------------------------------
// SrcRow<R>(src, h, w, frame, n, y) is row y of image n; px(x, ...) its pixel at column x as B, G, R.  y and x are coordinates of the
// whole image (the box kernel adds its window's origin), already clamped and reflected.
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <int R>
struct SrcRow;
template <>
struct SrcRow<kReadPacked> {
  const unsigned char* r;
  __device__ __forceinline__ SrcRow(const unsigned char* src, int h, int w, const FrameSource&, int n, int y)
      : r(src + ((long)n * h + y) * w * 3) {}
  __device__ __forceinline__ void px(int x, int& b0, int& b1, int& b2) const { b0 = r[x * 3 + 0], b1 = r[x * 3 + 1], b2 = r[x * 3 + 2]; }
};
template <>
struct SrcRow<kReadBgr> {
  const unsigned char* r;
  __device__ __forceinline__ SrcRow(const unsigned char*, int, int, const FrameSource& f, int n, int y)
      : r(f.planes[n].plane0 + (long)y * f.planes[n].pitch0) {}
  __device__ __forceinline__ void px(int x, int& b0, int& b1, int& b2) const { b0 = r[x * 3 + 0], b1 = r[x * 3 + 1], b2 = r[x * 3 + 2]; }
};
template <>
struct SrcRow<kReadNv12> {
  const unsigned char *ry, *rc;
  const FrameSource& f;
  __device__ __forceinline__ SrcRow(const unsigned char*, int, int, const FrameSource& fs, int n, int y)
      : ry(fs.planes[n].plane0 + (long)y * fs.planes[n].pitch0), rc(fs.planes[n].plane1 + (long)(y >> 1) * fs.planes[n].pitch1), f(fs) {}
  // the conversion rule of include/deepcut_hip.h (dc_frame): int32 throughout, |sum| < 2^26, arithmetic shift
  __device__ __forceinline__ void px(int x, int& b0, int& b1, int& b2) const {
    const int c = (int)ry[x] - f.y0, d = (int)rc[(x >> 1) * 2 + 0] - 128, e = (int)rc[(x >> 1) * 2 + 1] - 128;
    const int l = f.ky * c + 32768;
    b0 = clip8((l + f.bu * d) >> 16);
    b1 = clip8((l + f.gu * d + f.gv * e) >> 16);
    b2 = clip8((l + f.rv * e) >> 16);
  }
};

template <int R>
__global__ __launch_bounds__(256) void image_resample_x_kernel(ImagePrepParams p) {
  const long total = (long)p.n * p.rows * p.use_w;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % p.use_w);
  const long t = i / p.use_w;
  const int r = (int)(t % p.rows), n = (int)(t / p.rows);
  const int sy = min(p.row0 + r, p.h - 1);  // rows >= h replicate the last row (estimate_pose.py:89-92)
  const SrcRow<R> row(p.src, p.h, p.w, p.frame, n, sy);
  const int xmin = p.x_bounds[2 * x], cnt = p.x_bounds[2 * x + 1];
  const int* kk = p.x_coeffs + (long)x * p.x_ksize;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int k = 0; k < cnt; ++k) {
    int sx = min(xmin + k, p.w - 1);  // columns >= w replicate the last column (:93-95)
    if (p.mirror) sx = p.w - 1 - sx;  // ... of the mirrored image: column x of it is source column w - 1 - x
    const int c = kk[k];
    int b0, b1, b2;
    row.px(sx, b0, b1, b2);
    a0 += b0 * c;
    a1 += b1 * c;
    a2 += b2 * c;
  }
  reinterpret_cast<uchar4*>(p.tmp)[i] = make_uchar4((unsigned char)clip8_fixed(a0), (unsigned char)clip8_fixed(a1),
                                                    (unsigned char)clip8_fixed(a2), 0);
}

template <typename T, int R>
__global__ __launch_bounds__(256) void image_finish_kernel(ImagePrepParams p) {
  const long total = (long)p.n * p.out_h * p.out_w;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % p.out_w);
  const long t = i / p.out_w;
  const int y = (int)(t % p.out_h), n = (int)(t / p.out_h);
  float v[3] = {0.f, 0.f, 0.f};
  if (y < p.use_h && x < p.use_w) {
    auto fetch = [&](int row, int& b0, int& b1, int& b2) {
      if (p.x_bounds) {
        const uchar4 q = reinterpret_cast<const uchar4*>(p.tmp)[((long)n * p.rows + (row - p.row0)) * p.use_w + x];
        b0 = q.x, b1 = q.y, b2 = q.z;
      } else {
        const int sx = min(x, p.w - 1);
        SrcRow<R>(p.src, p.h, p.w, p.frame, n, min(row, p.h - 1)).px(p.mirror ? p.w - 1 - sx : sx, b0, b1, b2);
      }
    };
    int o0, o1, o2;
    if (p.y_bounds) {
      const int ymin = p.y_bounds[2 * y], cnt = p.y_bounds[2 * y + 1];
      const int* kk = p.y_coeffs + (long)y * p.y_ksize;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int k = 0; k < cnt; ++k) {
        int b0, b1, b2;
        fetch(ymin + k, b0, b1, b2);
        const int c = kk[k];
        a0 += b0 * c, a1 += b1 * c, a2 += b2 * c;
      }
      o0 = clip8_fixed(a0), o1 = clip8_fixed(a1), o2 = clip8_fixed(a2);
    } else {
      fetch(y, o0, o1, o2);
    }
    v[0] = (float)o0 - p.mean[0], v[1] = (float)o1 - p.mean[1], v[2] = (float)o2 - p.mean[2];
  }
  T* d = reinterpret_cast<T*>(p.dst) + i * p.dst_cp;
  for (int c = 0; c < p.dst_cp; ++c) d[c] = (T)(c < 3 ? v[c] : 0.f);
}

// One thread per canvas pixel of every box.  The vertical taps of a pixel read rows of the horizontally resampled crop that
// are computed here, per tap row, with Pillow's rounding and 8-bit clip: the same integers as the two-pass route.
template <typename T, int R>
__global__ __launch_bounds__(256) void box_prep_kernel(BoxPrepParams p) {
  const long total = (long)p.n * p.out_h * p.out_w;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % p.out_w);
  const long t = i / p.out_w;
  const int y = (int)(t % p.out_h), n = (int)(t / p.out_h);
  const BoxPrepItem it = p.items[n];
  float v[3] = {0.f, 0.f, 0.f};
  if (y < it.use_h && x < it.use_w) {
    // row r of the replicate-padded crop after the horizontal pass (rows / columns past the crop repeat its last one)
    auto hrow = [&](int r, int& b0, int& b1, int& b2) {
      // (image coordinates: an NV12 pixel pairs with the chroma sample of its place in the IMAGE, whatever the window's origin)
      const SrcRow<R> row(p.src, p.img_h, p.img_w, p.frame, 0, it.y0 + min(r, it.h - 1));
      if (it.x_bounds) {
        const int xmin = it.x_bounds[2 * x], cnt = it.x_bounds[2 * x + 1];
        const int* kk = it.x_coeffs + (long)x * it.x_ksize;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int k = 0; k < cnt; ++k) {
          int sx = min(xmin + k, it.w - 1);
          if (p.mirror) sx = it.w - 1 - sx;  // the mirrored crop: column x of it is crop column w - 1 - x (after the clamp, as image_resample_x_kernel)
          const int c = kk[k];
          int s0, s1, s2;
          row.px(it.x0 + sx, s0, s1, s2);
          a0 += s0 * c;
          a1 += s1 * c;
          a2 += s2 * c;
        }
        b0 = clip8_fixed(a0), b1 = clip8_fixed(a1), b2 = clip8_fixed(a2);
      } else {
        int sx = min(x, it.w - 1);
        if (p.mirror) sx = it.w - 1 - sx;
        row.px(it.x0 + sx, b0, b1, b2);
      }
    };
    int o0, o1, o2;
    if (it.y_bounds) {
      const int ymin = it.y_bounds[2 * y], cnt = it.y_bounds[2 * y + 1];
      const int* kk = it.y_coeffs + (long)y * it.y_ksize;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int k = 0; k < cnt; ++k) {
        int b0, b1, b2;
        hrow(ymin + k, b0, b1, b2);
        const int c = kk[k];
        a0 += b0 * c, a1 += b1 * c, a2 += b2 * c;
      }
      o0 = clip8_fixed(a0), o1 = clip8_fixed(a1), o2 = clip8_fixed(a2);
    } else {
      hrow(y, o0, o1, o2);
    }
    v[0] = (float)o0 - p.mean[0], v[1] = (float)o1 - p.mean[1], v[2] = (float)o2 - p.mean[2];
  }
  T* d = reinterpret_cast<T*>(p.dst) + i * p.dst_cp;
  for (int c = 0; c < p.dst_cp; ++c) d[c] = (T)(c < 3 ? v[c] : 0.f);
}

// the reader as a compile-time constant; the packed one is what the entries without a dc_frame launch
template <typename F>
static int by_reader(int reader, F&& f) {
  switch (reader) {
    case kReadPacked: return f(std::integral_constant<int, kReadPacked>{});
    case kReadBgr: return f(std::integral_constant<int, kReadBgr>{});
    case kReadNv12: return f(std::integral_constant<int, kReadNv12>{});
  }
  return (int)hipErrorInvalidValue;
}
static bool source_ok(const unsigned char* src, const FrameSource& f) { return f.reader == kReadPacked ? src != nullptr : f.planes != nullptr; }

int launch_box_prep(const BoxPrepParams& p, void* stream) {
  if (p.dst_ekind != kElemF32 && p.dst_ekind != kElemF16 && p.dst_ekind != kElemBF16) return (int)hipErrorInvalidValue;
  if (p.dst_cp < 3 || !p.items || !source_ok(p.src, p.frame)) return (int)hipErrorInvalidValue;
  const long total = (long)p.n * p.out_h * p.out_w;
  if (total <= 0) return 0;
  return dc_by_kind(p.dst_ekind, [&](auto* tag) {
    return by_reader(p.frame.reader, [&](auto reader) {
      hipLaunchKernelGGL((box_prep_kernel<std::remove_pointer_t<decltype(tag)>, decltype(reader)::value>), dim3((unsigned)((total + 255) / 256)),
                         dim3(256), 0, (hipStream_t)stream, p);
      return (int)hipGetLastError();
    });
  });
}

int launch_image_prep(const ImagePrepParams& p, void* stream) {
  if (p.dst_ekind != kElemF32 && p.dst_ekind != kElemF16 && p.dst_ekind != kElemBF16) return (int)hipErrorInvalidValue;
  if (p.dst_cp < 3 || p.use_h > p.out_h || p.use_w > p.out_w) return (int)hipErrorInvalidValue;
  if (p.frame.reader != kReadPacked && !p.frame.planes) return (int)hipErrorInvalidValue;
  return by_reader(p.frame.reader, [&](auto reader) {
    constexpr int R = decltype(reader)::value;
    if (p.x_bounds) {
      const long total = (long)p.n * p.rows * p.use_w;
      if (total > 0)
        hipLaunchKernelGGL(image_resample_x_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    }
    const long total = (long)p.n * p.out_h * p.out_w;
    if (total <= 0) return 0;
    return dc_by_kind(p.dst_ekind, [&](auto* tag) {
      hipLaunchKernelGGL((image_finish_kernel<std::remove_pointer_t<decltype(tag)>, R>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                         (hipStream_t)stream, p);
      return (int)hipGetLastError();
    });
  });
}


}  // namespace dc
