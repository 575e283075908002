// kernels_gain.hip -- socp_gain_batch of the in-tree Goddard, double-integrator and covid19 models (gain.hpp, fields.hpp, dual.hpp).
// MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every dual-number rule and every product of the backward
// sweep is a fixed sequence of IEEE roundings and tests/gain_reference.py restates them bit for bit.  ONE object for both flavours:
// the tables of kernels_exact.hip and of kernels_fast.hip point to the launchers below, so a throughput-flavour context returns the
// same bits.  The value trajectories are the reference-order ones, not the fast residual's.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t gain_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                        double *Xq, int *count, double *Psi, double *Wq, double *A, double *Kp)
{
    return (goddard_smooth(P, pb) ? &plugin::gain<GoddardExactSmooth> : &plugin::gain<GoddardExact>)(st, P, pb, B, Z, stride, cap, tq, Xq, count,
                                                                                                   Psi, Wq, A, Kp);
}

hipError_t gain_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                     double *Xq, int *count, double *Psi, double *Wq, double *A, double *Kp)
{
    return plugin::gain<DIntExact>(st, P, pb, B, Z, stride, cap, tq, Xq, count, Psi, Wq, A, Kp);
}

hipError_t gain_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                      double *Xq, int *count, double *Psi, double *Wq, double *A, double *Kp)
{
    return plugin::gain<CovidExact>(st, P, pb, B, Z, stride, cap, tq, Xq, count, Psi, Wq, A, Kp);
}

}  // namespace socp
