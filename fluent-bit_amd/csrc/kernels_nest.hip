// kernels_nest.hip -- filter_nest, a lane per record (nest_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "nest.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "canon_walk.inc"
#include "nest_kernels.inc"

}  // namespace flbgpu
