// forms.cpp — the forms table: the kernels beside the gather-GEMM tiles that a convolution can run as (Winograd, streaming 1x1, stem),
// one row each, and the variant_* dispatch over tiles and forms.
#include <cstring>
#include <string>

#include "kernels.h"

namespace dc {

// DC_DEBUG_TIMING phase slots 1..7 of the forms: the Winograd kernels' (stem7x7 reports under these names too) and the streaming ones'
// (stream1x1.hip: 0 start, 1 every prologue request issued, 2 first stage + filters + constants landed, 3 the peeled first D steps done,
// 4 the other steps (and the late half's last epilogue) done, 5 requests drained)
static const char* const kWinoSlots[7] = {"index setup", "first loads issued", "two stages in LDS", "K loop", "partials to LDS + barrier",
                                          "inverse transform + epilogue constants", "shortcut + stores"};
static const char* const kStreamSlots[7] = {"prologue requests issued", "first stage + filters landed", "the first D steps", "the other steps",
                                            "drain", "-", "exit"};
static constexpr ConvForm kForms[kNumForms] = {
    // variant, name, label, ekind, geometry, waves, slots, eligible, grid, launch, own_scale, merges, prepare_multi, launch_multi, sibling, env, offered, env_default, load_only
    {kWinoVariant, "wino_f23", "wino_f23<4x8x16>", kElemF32, kForm3x3, 8, kWinoSlots, wino_eligible, wino_grid, launch_wino_f23,
     false, false, nullptr, nullptr, kWinoVariant16, "DC_WINOGRAD"},
    {kWinoVariant16, "wino_f23_w16", "wino_f23<4x8x16_w16>", kElemF32, kForm3x3, 16, kWinoSlots, wino_eligible, wino_grid, launch_wino_f23_w16,
     false, false, nullptr, nullptr, kWinoVariant, "DC_WINOGRAD"},
    {kWinoHalf, "wino_h23", "wino_h23<2x4x8x64>", kElemF16, kForm3x3, 8, kWinoSlots, wino_half_eligible, wino_half_grid, launch_wino_half,
     true, true, nullptr, nullptr, -1, "DC_WINOGRAD"},
    {kStreamHalf, "ws1x1", "ws1x1<32xN>", kElemF16, kForm1x1, 4, kStreamSlots, stream1x1_eligible, stream1x1_grid, launch_stream1x1,
     false, true, stream1x1_prepare_multi, launch_stream1x1_multi, -1, "DC_STREAM1X1"},
    {kStemHalf, "stem7x7", "stem7x7<8x64>", kElemF16, kFormStem, 4, kWinoSlots, stem7x7_eligible, stem7x7_grid, launch_stem7x7,
     false, false, nullptr, nullptr, -1, "DC_STEM"},
    {kStreamFloat, "ws1x1f", "ws1x1f<16xN>", kElemF32, kForm1x1, 4, kStreamSlots, stream1x1f_eligible, stream1x1f_grid, launch_stream1x1f,
     false, true, nullptr, nullptr, -1, "DC_STREAM1X1"},
    {kStemFloat, "ws7x7f", "ws7x7f<16x64>", kElemF32, kFormStem, 4, kStreamSlots, stem_ws_eligible, stem_ws_grid, launch_stem_ws,
     false, true, nullptr, nullptr, -1, "DC_STEM"},
    {kWinoVariant56, "wino_f23_5x6", "wino_f23<5x6x16>", kElemF32, kForm3x3, 8, kWinoSlots, wino_eligible, wino_grid_5x6, launch_wino_f23_5x6,
     false, false, nullptr, nullptr, kWinoVariant56x16, "DC_WINOGRAD", wino_fewer_blocks},
    {kWinoVariant56x16, "wino_f23_5x6_w16", "wino_f23<5x6x16_w16>", kElemF32, kForm3x3, 16, kWinoSlots, wino_eligible, wino_grid_5x6, launch_wino_f23_5x6_w16,
     false, false, nullptr, nullptr, kWinoVariant56, "DC_WINOGRAD", wino_fewer_blocks},
    // the bfloat16 forms are opt-in: switches of their own, 0 while unset
    {kStreamBf16, "bs1x1", "bs1x1<32xN>", kElemBF16, kForm1x1, 4, kStreamSlots, stream1x1_bf16_eligible, stream1x1_grid, launch_stream1x1_bf16,
     false, true, stream1x1_bf16_prepare_multi, launch_stream1x1_bf16_multi, -1, "DC_STREAM1X1_BF16", nullptr, 0},
    {kStemBf16, "bs7x7", "bs7x7<8x64>", kElemBF16, kFormStem, 4, kWinoSlots, stem7x7_bf16_eligible, stem7x7_grid, launch_stem7x7_bf16,
     false, false, nullptr, nullptr, -1, "DC_STEM_BF16", nullptr, 0},
    {kWinoVariantMix, "wino_f23_mix", "wino_f23<4x8+5x6x16>", kElemF32, kForm3x3, 8, kWinoSlots, wino_eligible, wino_grid_mix, launch_wino_f23_mix,
     false, false, nullptr, nullptr, kWinoVariantMix16, "DC_WINOGRAD", wino_mix_fewer_blocks},
    {kWinoVariantMix16, "wino_f23_mix_w16", "wino_f23<4x8+5x6x16_w16>", kElemF32, kForm3x3, 16, kWinoSlots, wino_eligible, wino_grid_mix, launch_wino_f23_mix_w16,
     false, false, nullptr, nullptr, kWinoVariantMix, "DC_WINOGRAD", wino_mix_fewer_blocks},
    // three launches (wino43_f32.hip): the label names the multiply, whose batched instantiation does the matrix work (launch counts read "ws1x1f<")
    {kWinoF43, "wino_f43", "wino_f43+ws1x1f<16xN>", kElemF32, kForm3x3, 4, kStreamSlots, wino43_eligible, wino43_grid, launch_wino_f43,
     false, false, nullptr, nullptr, -1, "DC_WINOGRAD43", wino43_offered, -1, true},
};

static constexpr bool forms_in_variant_order() {
  for (int i = 0; i < kNumForms; ++i)
    if (kForms[i].variant != kFormVariant0 + i) return false;
  return true;
}
static_assert(forms_in_variant_order(), "row i of kForms is variant kFormVariant0 + i");

const ConvForm* conv_form(int variant) {
  return variant >= kFormVariant0 && variant < kFormVariant0 + kNumForms ? &kForms[variant - kFormVariant0] : nullptr;
}

const char* variant_name(int v) {
  const ConvForm* f = conv_form(v);
  return f ? f->name : conv_variant(v).name;
}
int variant_by_name(const char* name) {
  for (const ConvForm& f : kForms)
    if (std::strcmp(name, f.name) == 0) return f.variant;
  return conv_variant_by_name(name);
}
std::string variant_kernel_label(int v) {
  const ConvForm* f = conv_form(v);
  return f ? std::string(f->label) : std::string("conv_gemm<") + conv_variant(v).name + ">";
}
long variant_grid(const ConvGemmParams& p, int v) {
  const ConvForm* f = conv_form(v);
  return f ? f->grid(p) : conv_grid(p, v);
}
int launch_conv(const ConvGemmParams& p, int v, void* stream) {
  const ConvForm* f = conv_form(v);
  return f ? f->launch(p, stream) : launch_conv_gemm(p, v, stream);
}

}  // namespace dc
