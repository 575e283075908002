// kernels_exact.hip -- reference-operation-order kernels.  MUST be compiled with
// -ffp-contract=off (see socp_amd/csrc/Makefile): the parity tests compare these against the
// CPU oracle at the few-ulp level.  Holds the launch tables of the in-tree Goddard, double-integrator and covid19
// models (builtin_tables.hpp; adaptive Dormand-Prince instantiations included) and the model-independent launchers.
#define SOCP_DEFINE_COMMON 1   // fd_diff, cost_total and regrid_pack live in the no-contraction TU
#include "models_exact.hpp"
#include "builtin_tables.hpp"
#include "models_variational.hpp"

namespace socp {

const ModelLaunchers *builtin_launchers(int model_id)
{
    constexpr auto tables = &builtin_tables<GoddardExact, GoddardExactSmooth, CovidExact, DIntExact>;
    // variational (hybrj) path: the double integrator only; DIntVar is a struct of its own, so the entries are set by hand
    static const ModelLaunchers dint = [] {
        ModelLaunchers t = *tables(SOCP_MODEL_DOUBLE_INTEGRATOR);
        t.var_traj = &varimpl::traj<DIntVar>; t.var_jacobian = &varimpl::jacobian<DIntVar>; t.var_eval = &varimpl::eval<DIntVar>;
        return t;
    }();
    return model_id == SOCP_MODEL_DOUBLE_INTEGRATOR ? &dint : tables(model_id);
}

hipError_t regrid_pack(hipStream_t st, int B, int S, int M2, int n2, const unsigned long long (&free_bits)[4], const double *Xm,
                       const double *T2, double *Z2)
{
    if (B <= 0 || n2 <= 0) return hipSuccess;
    RegridFree fr;
    for (int k = 0; k < 4; k++) fr.w[k] = free_bits[k];
    hipLaunchKernelGGL(regrid_pack_kernel, dim3(blocks_for((long)B * n2)), dim3(64), 0, st, B, S, M2, n2, fr, Xm, T2, Z2);
    return hipGetLastError();
}

hipError_t cost_total(hipStream_t st, int B, int M, const double *cost, double *total)
{
    if (B <= 0 || M <= 0) return hipSuccess;
    hipLaunchKernelGGL(cost_total_kernel, dim3(blocks_for(B)), dim3(64), 0, st, B, M, cost, total);
    return hipGetLastError();
}

hipError_t fd_diff(hipStream_t st, int n, int np, const double *z, double eps, const double *rows, double *fjac)
{
    if (np <= 0) return hipSuccess;
    const long total = (long)np * n * n;
    hipLaunchKernelGGL(fd_diff_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n, np, z, eps, rows, fjac);
    return hipGetLastError();
}

}  // namespace socp
