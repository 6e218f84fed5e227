// kernels_expect.hip -- filter_expect, a lane per record (expect_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "expect.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "canon_walk.inc"
#include "ra_lds.inc"
#include "expect_kernels.inc"

}  // namespace flbgpu
