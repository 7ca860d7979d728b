// Shared by the pooling kernels of pool.hip (LDS-resident) and pool_wide.hip (tiled).
#pragma once
#include "sgg_common.h"

namespace sgg {

// column tiling of the 512 -> bn layer on the 16x16x4 fp32 MFMA
template <int BN>
struct PoolCfg {
  static constexpr int NT = (BN + 15) / 16;                      // 16-wide column tiles
  static constexpr int BNP = NT * 16 + ((NT % 2 == 0) ? 16 : 0); // odd multiple of 16: conflict-free B reads
};

// compute units of the current device (256 when the query fails)
static inline int device_cus() {
  static int ncu = 0;
  if (ncu == 0) {
    int d = 0, v = 0;
    if (hipGetDevice(&d) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess)
      ncu = v > 0 ? v : 256;
    else
      ncu = 256;
  }
  return ncu;
}

// the row-chunk planner of the tiled forwards (pool_wide.hip), shared by
// sgg_pool_plan_wide and sgg_pool_plan_bn; `name` prefixes its error messages
int pool_plan_rows(const char* name, const int32_t* host_scene_off, int S, int gpw, int target_chunks,
                   int32_t* chunks, int cap, int* max_rows, int* gpw_out);

}  // namespace sgg
