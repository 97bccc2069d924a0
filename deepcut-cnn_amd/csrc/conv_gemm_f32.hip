// conv_gemm_f32.hip — the float32 instantiations of the gather-GEMM kernel (conv_gemm.h): those of the DC_ROW_F32 rows of conv_gemm_variants.h.
#include "conv_gemm.h"

namespace dc {
#define DC_ROW_F32(...) DC_CONV_GEMM_ROW(float, __VA_ARGS__)
#define DC_ROW_F16(...)
#define DC_ROW_BF16(...)
#include "conv_gemm_variants.h"
}  // namespace dc
