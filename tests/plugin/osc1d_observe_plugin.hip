// osc1d_observe_plugin.hip -- osc1d_plugin.hip's dynamics plus the observables trait (include/socp_plugin.h, launch-table ABI 14): the
// smallest out-of-tree model with an observe entry (tests of socp_observe_batch).
//   x' = -p,  p' = w x;  observables: the energy (x^2 + p^2) / 2 and |u| = |p|.
// State vector [x ; p].  One parameter: w (default 4).  A model id of its own: the other osc1d plugins stay without the trait.
#include "plugin_impl.hpp"

struct Osc1DObserve {
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
    // the observables, each operation rounding once in the order written (tests/observe_reference.py restates them)
    static constexpr int kObservables = 2;
    static constexpr const char *kObservableNames[kObservables] = {"energy", "abs_u"};
    __device__ static void observe(const socp::ModelParams &, double, double, double, const double (&X)[S], const double (&u)[NU],
                                   double (&y)[kObservables])
    {
        y[0] = (X[0] * X[0] + X[1] * X[1]) / 2;
        y[1] = fabs(u[0]);
    }
};

SOCP_DEFINE_MODEL_PLUGIN(1006, Osc1DObserve, 1, 20, {4.0})
