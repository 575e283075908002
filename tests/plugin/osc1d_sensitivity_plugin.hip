// osc1d_sensitivity_plugin.hip -- osc1d_exact_jacobian_plugin.hip's model with its three traits generic in the PARAMETER view as well
// (include/socp_plugin.h, launch-table ABI 15): the smallest out-of-tree model with exact parameter sensitivities (tests of
// socp_sensitivity_batch).
//   x' = -p,  p' = w x,  H = u^2 / 2 - w x^2 / 2 + p u with u = -p;  the free-interior-time row is H(t, X-) - H(t, X+).
// State vector [x ; p].  One parameter: w (default 4).  A model id of its own: the other osc1d plugins stay as they are.
// PV is socp::ModelParams for the residual, the fields and the exact Jacobian -- the texts are then what they were -- and the dual
// view of the parameter block for socp_sensitivity_batch: a local that holds a parameter is `auto`.
#include "plugin_impl.hpp"

struct Osc1DSensitivity {
    static constexpr int D = 1;
    static constexpr int S = 2;
    static constexpr int NU = 1;
    static constexpr bool kRefOrder = true;

    __device__ static void control_only(const socp::ModelParams &, double, double, double, const double (&X)[S], double (&u)[3])
    {
        u[0] = -X[1]; u[1] = 0; u[2] = 0;
    }
    template <class T, class PV>
    __device__ static void rhs_t(const PV &P, double, double, double, const T (&X)[S], T (&dX)[S])
    {
        const auto w = P.p[0];
        dX[0] = -X[1];
        dX[1] = w * X[0];
    }
    template <class T, class PV>
    __device__ static T hamiltonian_t(const PV &P, double, double, double, const T (&X)[S])
    {
        const auto w = P.p[0];
        const T u = -X[1];
        return u * u / 2 - w * X[0] * X[0] / 2 + X[1] * u;
    }
    static constexpr bool kSwitchingReadsXp = true;
    template <class T, class PV>
    __device__ static T switching_fn_t(const PV &P, double a, double b, double t, const T (&X)[S], const T (&Xp)[S])
    {
        return hamiltonian_t<T>(P, a, b, t, X) - hamiltonian_t<T>(P, a, b, t, Xp);
    }
    __device__ static void rhs(const socp::ModelParams &P, double a, double b, double t, const double (&X)[S], double (&dX)[S])
    {
        rhs_t<double>(P, a, b, t, X, dX);
    }
    __device__ static double hamiltonian(const socp::ModelParams &P, double a, double b, double t, const double (&X)[S])
    {
        return hamiltonian_t<double>(P, a, b, t, X);
    }
    __device__ static double switching_fn(const socp::ModelParams &P, double a, double b, double t, const double (&X)[S], const double (&Xp)[S])
    {
        return switching_fn_t<double>(P, a, b, t, X, Xp);
    }
};

SOCP_DEFINE_MODEL_PLUGIN(1007, Osc1DSensitivity, 1, 20, {4.0})
