// What the raster units (raster.hip, raster_tone.hip) share: how a band's nodata value is held and compared, the size of a
// sample of each GDL_RAW_* kind, and the checks of a source's kind and extent.  A sample is read as S(src[i]) with S the C type
// of its kind and compared as a double.
#pragma once
#include "gdl_common.h"

namespace {

constexpr int64_t PIXEL_LIMIT = (int64_t)1 << 31;

struct NoData {
  double value;
  int has, is_nan;
  __device__ __forceinline__ bool masks(double v) const { return has && (is_nan ? v != v : v == value); }
};

// nodata, has_nodata: the HOST arrays of the C-ABI (either may be NULL)
inline NoData band_nodata(const double* nodata, const uint8_t* has_nodata, int c) {
  const bool has = nodata && (!has_nodata || has_nodata[c]);
  return NoData{has ? nodata[c] : 0.0, has, has && nodata[c] != nodata[c]};
}

inline size_t kind_size(int kind) { return kind == GDL_RAW_U8 ? 1 : kind == GDL_RAW_F32 ? 4 : 2; }

inline int check_source(const char* fn, int kind, int C, int H, int W) {
  GDL_CHECK_ARG(kind >= GDL_RAW_U8 && kind <= GDL_RAW_F32, "%s: bad sample kind %d", fn, kind);
  GDL_CHECK_ARG(C > 0 && C <= 65535 && H > 0 && W > 0 && (int64_t)H * W < PIXEL_LIMIT, "%s: source [%d, %d, %d]: sizes must be positive, C <= 65535 and H * W < 2^31", fn, C, H, W);
  return GDL_OK;
}

}  // namespace
