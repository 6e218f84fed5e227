// kernels_mlfilter.hip -- filter_multiline (mode parser, buffer off), a lane per record around the multiline core
// (mlfilter_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "mlfilter_kernels.inc"

}  // namespace flbgpu
