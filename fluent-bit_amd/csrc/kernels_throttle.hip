// kernels_throttle.hip -- filter_throttle_size: extraction a lane per record, the order by window, the admission, the ticker's trip
// (throttle_kernels.inc; shares kdev.inc with the other kernel units).  Compiled without contraction: the admission evaluates the
// reference's binary64 comparison as it is written.
#include <cstring>
#include <string.h>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "throttle.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "ra_lds.inc"
#include "l2m_dev.inc"
#include "throttle_kernels.inc"

}  // namespace flbgpu
