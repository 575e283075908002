// dint_hx_plugin.hip -- dint_h_plugin.hip's model with the exact-derivative entries (include/socp_plugin.h, "A MODEL FROM ITS
// HAMILTONIAN", launch-table ABI 17): the in-tree double integrator's control_only and hamiltonian_t texts
// (doubleIntegrator.cpp:218-300), the Hamiltonian generic in the PARAMETER view, and NO hand-written dynamics.
// plugin::FromHamiltonianExact makes the right-hand side (dH/dp, -dH/dx) by dual numbers and the right-hand side over dual numbers by
// NESTED ones: exact fields, the exact shooting Jacobian, the Newton polish that consumes it and exact parameter sensitivities run
// through the unchanged launch-table kernels.  State vector [x(3) v(3) ; p_x(3) p_v(3)], S = 12; the in-tree model's three parameters
// and defaults: u_max, a_max, muT.  Build with -ffp-contract=off.
#include "plugin_impl.hpp"

struct DIntHX {
    static constexpr int D = 6;
    static constexpr int S = 12;
    static constexpr int NU = 3;
    static constexpr bool kRefOrder = true;
    // derivative parts per pass of the gradient ON DUAL NUMBERS: a nested number is 2 (1 + W) doubles, and the exact kernels keep an RK4
    // step's dual states beside the gradient's working set.  Chosen for registers; the width changes no bit.  The plain right-hand side
    // keeps one pass of S parts, as dint_h_plugin.hip
    static constexpr int kNestedGradientWidth = 2;

    __device__ static void control_only(const socp::ModelParams &P, double, double, double, const double (&X)[S], double (&u)[3])
    {
        const double a_max = P.p[1], u_max = P.p[0];
        u[0] = -X[9] / a_max;
        u[1] = -X[10] / a_max;
        u[2] = -X[11] / a_max;
        const double norm_u = sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        if (norm_u > u_max) {
            u[0] = u[0] / norm_u*u_max;
            u[1] = u[1] / norm_u*u_max;
            u[2] = u[2] / norm_u*u_max;
        }
    }
    // H(X, u(X)) over a number type T and a parameter view PV (socp::ModelParams, or the dual view of socp_sensitivity_batch: a local
    // that holds a parameter is `auto`, a comparison reads d_val)
    template <class T, class PV>
    __device__ static T hamiltonian_t(const PV &P, double, double, double, const T (&X)[S])
    {
        using socp::d_sqrt;
        using socp::d_val;
        const auto a_max = P.p[1], u_max = P.p[0];
        T u[3];
        u[0] = -X[9] / a_max;
        u[1] = -X[10] / a_max;
        u[2] = -X[11] / a_max;
        const T norm_c = d_sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        if (d_val(norm_c) > d_val(u_max)) {
            u[0] = u[0] / norm_c*u_max;
            u[1] = u[1] / norm_c*u_max;
            u[2] = u[2] / norm_c*u_max;
        }
        const T norm_u = d_sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        return P.p[2] + a_max * a_max*norm_u*norm_u / 2 + X[6] * X[3] + X[7] * X[4] + X[8] * X[5]
             + a_max * (X[9]*u[0] + X[10] * u[1] + X[11] * u[2]);
    }
};

SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT(1011, DIntHX, 3, 30, {1.0, 1.0, 0.01})
