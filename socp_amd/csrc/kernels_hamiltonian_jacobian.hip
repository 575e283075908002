// kernels_hamiltonian_jacobian.hip -- socp_hamiltonian_jacobian_batch of the in-tree Goddard, double-integrator and covid19 models
// (hamiltonian_model.hpp, dualn.hpp on the carrier Dual).  MUST be compiled with -ffp-contract=off (see socp_amd/csrc/Makefile): every
// nested rule is a fixed sequence of IEEE roundings and tests/hamiltonian_exact_reference.py restates them bit for bit.  ONE object for
// both flavours, like kernels_hamiltonian.hip: a throughput-flavour context returns the same bits.
#include "models_exact.hpp"
#include "builtin_tables.hpp"

namespace socp {

// the derivative parts of an inner pass, per model: a nested number is 2 (1 + W) doubles, every pass recomputes the value part, and the
// width is chosen for registers (profiles/hamiltonian_exact_kernel_meta.txt).  The width changes no bit.  Goddard's smooth law, the double
// integrator and covid19 have no private segment at W = 2.  Goddard's GENERAL law has one even at W = 1, the narrowest pass there is:
// its closed-form singular control on numbers of four doubles does not fit 512 registers (298 spilled, 1196 bytes per lane; W = 2: 612
// spilled, 2444 bytes)
constexpr int kGoddardSmoothJacobianWidth = 2, kGoddardJacobianWidth = 1, kDIntJacobianWidth = 2, kCovidJacobianWidth = 2;

// the law as the evaluation kernel takes it: from the context's mu2
hipError_t hamiltonian_jacobian_goddard(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X,
                                        double *A, double *G)
{
    return (goddard_smooth(P) ? &plugin::hamiltonian_jacobian<GoddardExactSmooth, kGoddardSmoothJacobianWidth>
                              : &plugin::hamiltonian_jacobian<GoddardExact, kGoddardJacobianWidth>)(st, P, B, t, sw, X, A, G);
}

hipError_t hamiltonian_jacobian_dint(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *A,
                                     double *G)
{
    return plugin::hamiltonian_jacobian<DIntExact, kDIntJacobianWidth>(st, P, B, t, sw, X, A, G);
}

hipError_t hamiltonian_jacobian_covid(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *A,
                                      double *G)
{
    return plugin::hamiltonian_jacobian<CovidExact, kCovidJacobianWidth>(st, P, B, t, sw, X, A, G);
}

}  // namespace socp
