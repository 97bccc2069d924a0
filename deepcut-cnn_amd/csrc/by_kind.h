// by_kind.h — from an ElemKind (kernels.h) to the element type, for the launchers of layers.hip, pose.hip and image_prep.hip.
#pragma once
#include "kernels.h"

namespace dc {

// the element type of an ElemKind: f(tag) with tag a null T* (float, _Float16 or __bf16)
template <typename F>
static int dc_by_kind(int ekind, F&& f) {
  if (ekind == kElemF16) return f((_Float16*)nullptr);
  if (ekind == kElemBF16) return f((__bf16*)nullptr);
  return f((float*)nullptr);
}

}  // namespace dc
