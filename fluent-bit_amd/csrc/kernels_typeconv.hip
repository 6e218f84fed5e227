// kernels_typeconv.hip -- filter_type_converter, a lane per record (typeconv_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "typeconv.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "canon_walk.inc"
#include "ra_lds.inc"
#include "typeconv_kernels.inc"

}  // namespace flbgpu
