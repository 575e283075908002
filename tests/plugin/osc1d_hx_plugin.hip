// osc1d_hx_plugin.hip -- osc1d_h_plugin.hip's model with the exact-derivative entries (include/socp_plugin.h, "A MODEL FROM ITS
// HAMILTONIAN", launch-table ABI 17): control_only and hamiltonian_t and no dynamics, the Hamiltonian text generic in the PARAMETER
// view.  plugin::FromHamiltonianExact makes the right-hand side (dH/dp, -dH/dx) by dual numbers, and the right-hand side over dual
// numbers by NESTED ones, so the model has exact fields, the exact shooting Jacobian and exact parameter sensitivities.
//   H = u^2 / 2 - w x^2 / 2 + p u with u = -p.
// State vector [x ; p].  One parameter: w (default 4).  A model id of its own.  Build with -ffp-contract=off.
#include "plugin_impl.hpp"

struct Osc1DHX {
    static constexpr int D = 1;
    static constexpr int S = 2;
    static constexpr int NU = 1;
    static constexpr bool kRefOrder = true;
    // two passes of one derivative part each, as osc1d_h_plugin.hip: the pass loop runs on the device
    static constexpr int kGradientWidth = 1;

    __device__ static void control_only(const socp::ModelParams &, double, double, double, const double (&X)[S], double (&u)[3])
    {
        u[0] = -X[1]; u[1] = 0; u[2] = 0;
    }
    // PV is socp::ModelParams everywhere but in socp_sensitivity_batch, where it is the dual view of the parameter block
    template <class T, class PV>
    __device__ static T hamiltonian_t(const PV &P, double, double, double, const T (&X)[S])
    {
        const auto w = P.p[0];
        const T u = -X[1];
        return u * u / 2 - w * X[0] * X[0] / 2 + X[1] * u;
    }
};

SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT(1010, Osc1DHX, 1, 20, {4.0})
