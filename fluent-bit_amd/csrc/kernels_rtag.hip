// kernels_rtag.hip -- filter_rewrite_tag, a lane per record (rtag_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "rtag.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "ra_lds.inc"
#include "fmt_dev.inc"
#include "rtag_kernels.inc"

}  // namespace flbgpu
