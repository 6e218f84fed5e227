// kernels_modify.hip -- filter_modify, a lane per record (modify_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "mod.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "modify_kernels.inc"

}  // namespace flbgpu
