// osc1d_plugin.hip -- the smallest out-of-tree model with a KNOWN conjugate time (include/socp_plugin.h; tests of socp_jacobi_batch):
//   x' = u,  cost = int (u^2/2 - w x^2/2),  H = u^2/2 - w x^2/2 + p u  with  u = -p:   x' = -p,  p' = w x.
// The Jacobi field dx(t)/dp(0) = -sin(sqrt(w) t) / sqrt(w): conjugate times k pi / sqrt(w); with w = 0 there are none.
// State vector [x ; p].  One parameter: w (default 4).
#include "plugin_impl.hpp"

struct Osc1D {
    static constexpr int D = 1;
    static constexpr int S = 2;
    static constexpr int NU = 1;
    static constexpr bool kRefOrder = true;

    __device__ static void control_only(const socp::ModelParams &, double, double, double, const double (&X)[S], double (&u)[3])
    {
        u[0] = -X[1]; u[1] = 0; u[2] = 0;
    }
    __device__ static void rhs(const socp::ModelParams &P, double, double, double, const double (&X)[S], double (&dX)[S])
    {
        dX[0] = -X[1];
        dX[1] = P.p[0] * X[0];
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

SOCP_DEFINE_MODEL_PLUGIN(1002, Osc1D, 1, 20, {4.0})
