// conv_gemm_f16.hip — the float16 instantiations of the gather-GEMM kernel (conv_gemm.h): those of the DC_ROW_F16 rows of conv_gemm_variants.h.
#include "conv_gemm.h"

namespace dc {
#define DC_ROW_F32(...)
#define DC_ROW_F16(...) DC_CONV_GEMM_ROW(_Float16, __VA_ARGS__)
#define DC_ROW_BF16(...)
#include "conv_gemm_variants.h"
}  // namespace dc
