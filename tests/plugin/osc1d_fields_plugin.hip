// osc1d_fields_plugin.hip -- osc1d_plugin.hip's dynamics plus the rhs_t trait (include/socp_plugin.h, launch-table ABI 11): the
// smallest out-of-tree model with exact fields (tests of socp_fields_batch).
//   x' = -p,  p' = w x:   dx(t)/dp(0) = -sin(sqrt(w) t) / sqrt(w), conjugate times k pi / sqrt(w); with w = 0 there are none.
// State vector [x ; p].  One parameter: w (default 4).  A model id of its own: osc1d_plugin.hip stays without the trait.
#include "plugin_impl.hpp"

struct Osc1DFields {
    static constexpr int D = 1;
    static constexpr int S = 2;
    static constexpr int NU = 1;
    static constexpr bool kRefOrder = true;

    __device__ static void control_only(const socp::ModelParams &, double, double, double, const double (&X)[S], double (&u)[3])
    {
        u[0] = -X[1]; u[1] = 0; u[2] = 0;
    }
    // the right-hand side over a number type: T = double for rhs, T = socp::Dual for socp_fields_batch
    template <class T>
    __device__ static void rhs_t(const socp::ModelParams &P, double, double, double, const T (&X)[S], T (&dX)[S])
    {
        dX[0] = -X[1];
        dX[1] = P.p[0] * X[0];
    }
    __device__ static void rhs(const socp::ModelParams &P, double a, double b, double t, const double (&X)[S], double (&dX)[S])
    {
        rhs_t<double>(P, a, b, t, X, dX);
    }
    __device__ static double hamiltonian(const socp::ModelParams &P, double, double, double, const double (&X)[S])
    {
        const double u = -X[1];
        return u * u / 2 - P.p[0] * X[0] * X[0] / 2 + X[1] * u;
    }
    __device__ static double switching_fn(const socp::ModelParams &P, double a, double b, double t, const double (&X)[S], const double (&Xp)[S])
    {
        return hamiltonian(P, a, b, t, X) - hamiltonian(P, a, b, t, Xp);
    }
};

SOCP_DEFINE_MODEL_PLUGIN(1004, Osc1DFields, 1, 20, {4.0})
