// kernels_guide.hip -- socp_guide_batch of the in-tree Goddard, double-integrator and covid19 models in REFERENCE ORDER (guide.hpp).
// MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): the flight is the reference-order residual's RK4 and the
// correction a fixed sequence of IEEE roundings that tests/guide_reference.py restates bit for bit.  The reference-order tables of
// kernels_exact.hip point to the launchers below; the throughput flavour has its own (kernels_guide_fast.hip).
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t guide_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A)
{
    return goddard_by_problem<&plugin::guide<GoddardExactSmooth>, &plugin::guide<GoddardExact>>(st, P, pb, B, Z, free_tf, A);
}

hipError_t guide_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A)
{
    return plugin::guide<DIntExact>(st, P, pb, B, Z, free_tf, A);
}

hipError_t guide_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A)
{
    return plugin::guide<CovidExact>(st, P, pb, B, Z, free_tf, A);
}

}  // namespace socp
