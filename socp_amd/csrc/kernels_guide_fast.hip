// kernels_guide_fast.hip -- socp_guide_batch of the in-tree models in the THROUGHPUT flavour (guide.hpp on models_fast.hpp): compiled
// with FMA contraction like kernels_fast.hip, so that a throughput context flies its Monte-Carlo cases at throughput speed.  The
// throughput tables of kernels_fast.hip point to the launchers below -- Goddard's and covid19's.  The double integrator is ONE struct in
// both flavours (DIntFast = DIntExact): a second instantiation here would be the same symbols built with other flags, so both tables
// point to kernels_guide.hip's guide_dint and the model flies the reference-order arithmetic in a throughput context too.  The counters nupd / nskip are the reference order's whenever
// the tables' info words decide them; the states agree with the reference order to the flavours' own deviation times the gains
// (tests/test_gpu_guide_batch.py states and measures the allowance).
#include "models_fast.hpp"
#include "builtin_tables.hpp"

namespace socp {

hipError_t guide_goddard_fast(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf,
                              const GuideArgs &A)
{
    return goddard_by_problem<&plugin::guide<GoddardFastSmooth>, &plugin::guide<GoddardFast>>(st, P, pb, B, Z, free_tf, A);
}

hipError_t guide_covid_fast(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A)
{
    return plugin::guide<CovidFast>(st, P, pb, B, Z, free_tf, A);
}

}  // namespace socp
