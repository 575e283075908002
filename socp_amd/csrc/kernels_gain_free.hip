// kernels_gain_free.hip -- socp_gain_free_batch of the in-tree Goddard, double-integrator and covid19 models (gain_free.hpp,
// exact_jacobian.hpp, dual.hpp).  MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every dual-number rule and every
// product of the bordered backward sweep is a fixed sequence of IEEE roundings and tests/gain_free_reference.py restates them bit for
// bit.  ONE object for both flavours: the tables of kernels_exact.hip and of kernels_fast.hip point to the launchers below, so a
// throughput-flavour context returns the same bits.  The value trajectories are the reference-order ones, not the fast residual's.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t gain_free_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                             double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke)
{
    return (goddard_smooth(P, pb) ? &plugin::gain_free<GoddardExactSmooth> : &plugin::gain_free<GoddardExact>)(st, P, pb, B, Z, stride, cap, tq, Xq,
                                                                                                             count, Psi, Len, gradH, Wq, A, Ke);
}

hipError_t gain_free_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                          double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke)
{
    return plugin::gain_free<DIntExact>(st, P, pb, B, Z, stride, cap, tq, Xq, count, Psi, Len, gradH, Wq, A, Ke);
}

hipError_t gain_free_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                           double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke)
{
    return plugin::gain_free<CovidExact>(st, P, pb, B, Z, stride, cap, tq, Xq, count, Psi, Len, gradH, Wq, A, Ke);
}

}  // namespace socp
