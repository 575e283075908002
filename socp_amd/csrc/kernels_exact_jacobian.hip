// kernels_exact_jacobian.hip -- socp_exact_jacobian_batch of the in-tree Goddard, double-integrator and covid19 models
// (exact_jacobian.hpp, dual.hpp).  MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every dual-number rule is
// a fixed sequence of IEEE roundings and tests/exact_jacobian_reference.py restates them bit for bit.  ONE object for both flavours:
// the tables of kernels_exact.hip and of kernels_fast.hip point to the launchers below, so a throughput-flavour context returns the
// same bits.  The value trajectories are the reference-order ones, not the fast residual's.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t exact_jacobian_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F)
{
    return (goddard_smooth(P, pb) ? &plugin::exact_jacobian<GoddardExactSmooth> : &plugin::exact_jacobian<GoddardExact>)(st, P, pb, B, Z, Fjac, F);
}

hipError_t exact_jacobian_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F)
{
    return plugin::exact_jacobian<DIntExact>(st, P, pb, B, Z, Fjac, F);
}

hipError_t exact_jacobian_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F)
{
    return plugin::exact_jacobian<CovidExact>(st, P, pb, B, Z, Fjac, F);
}

}  // namespace socp
