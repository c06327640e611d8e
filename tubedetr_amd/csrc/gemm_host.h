// Process-wide host state the two GEMM-shaped files share, defined once in gemm_conv.hip.
#pragma once
#include "gemm_route.h"

namespace td {

const GemmKnobs& gemm_knobs();       // the dispatch knobs, read from the environment once per process
unsigned long long* stamp_buffer();  // the calling thread's td_debug_set_stamp_buffer pointer (tools/stamp_*.py), or null

}  // namespace td
