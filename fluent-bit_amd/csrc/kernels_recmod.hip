// kernels_recmod.hip -- filter_record_modifier, a lane per record (recmod_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "recmod.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "canon_walk.inc"
#include "recmod_kernels.inc"

}  // namespace flbgpu
