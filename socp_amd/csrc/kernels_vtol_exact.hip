// kernels_vtol_exact.hip -- socp_fields_batch and socp_exact_jacobian_batch of the vtolUAV waypoint model (models_vtol.hpp: rhs_t,
// hamiltonian_t, switching_fn_t, final_row_t, switching_state_t; fields.hpp, exact_jacobian.hpp, dual.hpp).  MUST be compiled with
// -ffp-contract=off (see socp_amd/csrc/Makefile): every dual-number rule is a fixed sequence of IEEE roundings and
// tests/vtol_exact_reference.py restates them.  ONE object for both flavours: the tables of kernels_vtol.hip and of
// kernels_vtol_fast.hip point to the launchers below, so a throughput-flavour context returns the same bits.  The value trajectories
// are the reference-order ones (VtolExact), not the fast residual's; tanh is the device library's.
#include "models_vtol.hpp"
#include "plugin_impl.hpp"

namespace socp {

hipError_t fields_vtol(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                       int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi)
{
    return plugin::fields<VtolExact>(st, P, pb, B, Z, cols, stride, skip, cap, tq, det, count, nchange, tconj, Phi);
}

hipError_t exact_jacobian_vtol(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F)
{
    static_assert(plugin::has_exact_jacobian<VtolExact>::value && !plugin::has_sensitivity<VtolExact>::value &&
                      !plugin::has_gain<VtolExact>::value && !plugin::has_gain_free<VtolExact>::value && !plugin::has_guide<VtolExact>::value,
                  "vtolUAV: the exact Jacobian through final_row_t and switching_state_t; no sensitivities, gains or guidance");
    return plugin::exact_jacobian<VtolExact>(st, P, pb, B, Z, Fjac, F);
}

}  // namespace socp
