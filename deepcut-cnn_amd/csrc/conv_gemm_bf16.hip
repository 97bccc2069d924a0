// conv_gemm_bf16.hip — the bfloat16 instantiations of the gather-GEMM kernel (conv_gemm.h): those of the DC_ROW_BF16 rows of conv_gemm_variants.h.
#include "conv_gemm.h"

namespace dc {
#define DC_ROW_F32(...)
#define DC_ROW_F16(...)
#define DC_ROW_BF16(...) DC_CONV_GEMM_ROW(__bf16, __VA_ARGS__)
#include "conv_gemm_variants.h"
}  // namespace dc
