// kernels_fast.hip -- throughput flavour: compiled with FMA contraction, restructured models
// (models_fast.hpp).  Results agree with the reference order to rounding level, not bitwise;
// the tolerance is stated and tested in tests/test_gpu_parity.py.  Holds the throughput launch tables of the in-tree
// Goddard, double-integrator and covid19 models (builtin_tables.hpp), adaptive Dormand-Prince on the restructured
// right-hand sides included; capi.cpp uses them when the context's variant is SOCP_VARIANT_LANE_FAST.
#include "models_fast.hpp"
#include "builtin_tables.hpp"

namespace socp {

const ModelLaunchers *builtin_launchers_fast(int model_id)
{
    return builtin_tables<GoddardFast, GoddardFastSmooth, CovidFast, DIntFast>(model_id);
}

}  // namespace socp
