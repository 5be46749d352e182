// sfm_desc.h — the resident descriptor set (sfm_desc_create ... sfm_desc_destroy) as the translation units that read it
// see it: the matcher (sfm_match.hip), which owns it, and the view retrieval (sfm_retrieve.hip).
#pragma once

#include <cstdint>

#include "sfm_common.h"

// `kind` of a set: the image the kernels read.  Exact L2: integer rows in [0, 255] as bf16 [n_pad][dp] (dp = 128 or 256,
// zero padded; n_pad a multiple of 128, at least 128) with their int32 squared norms [n_pad].
namespace sfm {
constexpr int kDescKindExact = 0, kDescKindHamming = 1, kDescKindFloat = 2;
}

struct sfm_desc_set {
  int metric, n, dim, dtype, kind, n_pad, dp;
  uint16_t* bf = nullptr;
  int* norm = nullptr;
  float* f32 = nullptr;
  uint32_t* words = nullptr;
  int64_t upload_bytes = 0;
};
