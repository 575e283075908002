// kernels_fields.hip -- socp_fields_batch of the in-tree Goddard, double-integrator and covid19 models (fields.hpp, dual.hpp).
// MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every dual-number rule is a fixed sequence of IEEE
// roundings and tests/fields_reference.py restates them bit for bit.  ONE object for both flavours: the tables of kernels_exact.hip
// and of kernels_fast.hip point to the launchers below, so a throughput-flavour context returns the same bits.  The value
// trajectories are the reference-order ones, not the fast residual's.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t fields_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                          int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi)
{
    return (goddard_smooth(P, pb) ? &plugin::fields<GoddardExactSmooth> : &plugin::fields<GoddardExact>)(st, P, pb, B, Z, cols, stride, skip,
                                                                                                       cap, tq, det, count, nchange, tconj, Phi);
}

hipError_t fields_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                       int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi)
{
    return plugin::fields<DIntExact>(st, P, pb, B, Z, cols, stride, skip, cap, tq, det, count, nchange, tconj, Phi);
}

hipError_t fields_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                        int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi)
{
    return plugin::fields<CovidExact>(st, P, pb, B, Z, cols, stride, skip, cap, tq, det, count, nchange, tconj, Phi);
}

}  // namespace socp
