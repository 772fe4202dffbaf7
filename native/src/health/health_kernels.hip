// The one gfx950 code object of the health checks: the kept executable is
// loaded once per device and every check borrows its kernel by symbol name, so
// the kernels of all source files are compiled as one translation unit.
#include "liveness_kernel.hip"
#include "datapath_kernel.hip"
#include "datapath_i8_kernel.hip"
#include "datapath_bf16_kernel.hip"
#include "datapath_fp8_kernel.hip"
#include "datapath_f16_kernel.hip"
