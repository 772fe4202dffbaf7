// The one gfx950 code object of the health checks: the kept executable is
// loaded once per device and every check borrows its kernel by symbol name, so
// the kernels of all source files are compiled as one translation unit.
#include "liveness_kernel.hip"
#include "datapath_kernel.hip"
#include "datapath_i8_kernel.hip"
#include "datapath_bf16_kernel.hip"
#include "datapath_fp8_kernel.hip"
#include "datapath_f16_kernel.hip"
#include "datapath_f64_kernel.hip"
#include "datapath_f6f4_kernel.hip"
#include "datapath_sparse_kernel.hip"
#include "datapath_gemm_kernel.hip"
#include "datapath_splitk_kernel.hip"
#include "datapath_attn_kernel.hip"
#include "datapath_mxgemm_kernel.hip"
#include "datapath_mxquant_kernel.hip"
