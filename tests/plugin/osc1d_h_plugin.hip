// osc1d_h_plugin.hip -- the osc1d example written from its Hamiltonian ALONE (include/socp_plugin.h, "A MODEL FROM ITS HAMILTONIAN",
// launch-table ABI 16): the smallest such model.  It brings control_only and hamiltonian_t and no dynamics;
// plugin::FromHamiltonian makes the right-hand side (dH/dp, -dH/dx) by dual numbers.
//   H = u^2 / 2 - w x^2 / 2 + p u with u = -p, so x' = dH/dp = -p and p' = -dH/dx = w x up to the roundings of the dual-number rules.
// State vector [x ; p].  One parameter: w (default 4).  A model id of its own.  Build with -ffp-contract=off.
#include "plugin_impl.hpp"

struct Osc1DH {
    static constexpr int D = 1;
    static constexpr int S = 2;
    static constexpr int NU = 1;
    static constexpr bool kRefOrder = true;
    // two passes of one derivative part each, not one pass of two: the bits are the same (dualn.hpp), and the tests that compare this
    // plugin with the one-pass restatement run the gradient's pass loop on the device
    static constexpr int kGradientWidth = 1;

    __device__ static void control_only(const socp::ModelParams &, double, double, double, const double (&X)[S], double (&u)[3])
    {
        u[0] = -X[1]; u[1] = 0; u[2] = 0;
    }
    template <class T>
    __device__ static T hamiltonian_t(const socp::ModelParams &P, double, double, double, const T (&X)[S])
    {
        const T u = -X[1];
        return u * u / 2 - P.p[0] * X[0] * X[0] / 2 + X[1] * u;
    }
};

SOCP_DEFINE_HAMILTONIAN_PLUGIN(1008, Osc1DH, 1, 20, {4.0})
