// fold1d_plugin.hip -- the smallest out-of-tree model with a KNOWN fold of its solution branch (include/socp_plugin.h; tests of
// socp_branch_batch):
//   x' = p^2 + a,  p' = 0,  u = p,  H = p (p^2 + a).
// Single shooting over [0, 1] with x(0) = 0 and x(1) = 1 fixed: F = [x0 - 0 ; x0 + p0^2 + a - 1] (RK4 is exact on a constant
// right-hand side, up to rounding).  The branch is a = 1 - p0^2: it turns back in a at the fold a = 1, p0 = 0.
// State vector [x ; p].  One parameter: a (default 0).
#include "plugin_impl.hpp"

struct Fold1D {
    static constexpr int D = 1;
    static constexpr int S = 2;
    static constexpr int NU = 1;
    static constexpr bool kRefOrder = true;

    __device__ static void control_only(const socp::ModelParams &, double, double, double, const double (&X)[S], double (&u)[3])
    {
        u[0] = X[1]; u[1] = 0; u[2] = 0;
    }
    __device__ static void rhs(const socp::ModelParams &P, double, double, double, const double (&X)[S], double (&dX)[S])
    {
        dX[0] = X[1] * X[1] + P.p[0];
        dX[1] = 0;
    }
    __device__ static double hamiltonian(const socp::ModelParams &P, double, double, double, const double (&X)[S])
    {
        return X[1] * (X[1] * X[1] + P.p[0]);
    }
    __device__ static double switching_fn(const socp::ModelParams &P, double a, double b, double t, const double (&X)[S], const double (&Xp)[S])
    {
        return hamiltonian(P, a, b, t, X) - hamiltonian(P, a, b, t, Xp);
    }
};

SOCP_DEFINE_MODEL_PLUGIN(1003, Fold1D, 1, 20, {0.0})
