// kernels_hamiltonian.hip -- socp_hamiltonian_gradient_batch of the in-tree Goddard, double-integrator and covid19 models
// (hamiltonian_model.hpp, dualn.hpp).  MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every dual-number rule is
// a fixed sequence of IEEE roundings and tests/hamiltonian_model_reference.py restates them bit for bit.  ONE object for both flavours:
// the tables of kernels_exact.hip and of kernels_fast.hip point to the launchers below, so a throughput-flavour context returns the
// same bits.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

// the law as the evaluation kernel takes it: from the context's mu2
hipError_t hamiltonian_gradient_goddard(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X,
                                        double *G)
{
    return (goddard_smooth(P) ? &plugin::hamiltonian_gradient<GoddardExactSmooth> : &plugin::hamiltonian_gradient<GoddardExact>)(st, P, B, t, sw,
                                                                                                                               X, G);
}

hipError_t hamiltonian_gradient_dint(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *G)
{
    return plugin::hamiltonian_gradient<DIntExact>(st, P, B, t, sw, X, G);
}

hipError_t hamiltonian_gradient_covid(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *G)
{
    return plugin::hamiltonian_gradient<CovidExact>(st, P, B, t, sw, X, G);
}

}  // namespace socp
