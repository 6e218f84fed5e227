// kernels_kube.hip -- filter_kubernetes' per-record half, a lane per record (kube_kernels.inc; shares kdev.inc with the other kernel units)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <type_traits>
#include "dev.hpp"
#include "numconv.hpp"
#include "typeconv.hpp"
#include "kube.hpp"

namespace flbgpu {

#include "kdev.inc"
#include "lane_rows.inc"
#include "canon_walk.inc"
#include "kube_kernels.inc"

}  // namespace flbgpu
