// builtin_tables.hpp -- launch tables of the in-tree Goddard, double-integrator and covid19 models: the tables of
// plugin_impl.hpp, plus the one thing an out-of-tree model has no use for -- the choice between Goddard's two control laws.
// Instantiated once per arithmetic flavour (kernels_exact.hip, kernels_fast.hip).
#pragma once
#include "plugin_impl.hpp"
#include "../../include/socp_hip.h"

namespace socp {

// Goddard launches the smooth-law specialisation (GoddardExactSmooth / GoddardFastSmooth) when mu2 > 0.  Kernels that read a
// shooting problem may get per-problem parameter blocks, whose law may differ between the problems of one launch: the
// specialisation is then taken only when the caller vouches for every block (ProblemDev::pp_smooth).
inline bool goddard_smooth(const ModelParams &P) { return P.p[GP_MU2] > 0; }
inline bool goddard_smooth(const ModelParams &P, const ProblemDev &pb) { return pb.pp_params ? pb.pp_smooth != 0 : goddard_smooth(P); }

// one table entry: the launcher of the smooth or of the general law, by the context's parameters / by the shooting problem
template <auto Smooth, auto General, class... Args>
hipError_t goddard_by_params(hipStream_t st, const ModelParams &P, Args... args)
{
    return (goddard_smooth(P) ? Smooth : General)(st, P, args...);
}
template <auto Smooth, auto General, class... Args>
hipError_t goddard_by_problem(hipStream_t st, const ModelParams &P, const ProblemDev &pb, Args... args)
{
    return (goddard_smooth(P, pb) ? Smooth : General)(st, P, pb, args...);
}
// the trace's fill takes the law the way the evaluation kernel does (from the context's mu2), and the general law when every
// problem brings its own parameters
template <class God, class GodSmooth>
hipError_t goddard_trace_fill(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, int cap, double *rows, const int *count)
{
    if (pb.pp_params) return plugin::trace_fill_pp<God, true>(st, P, pb, B, cap, rows, count);
    if (goddard_smooth(P)) return plugin::trace_fill_pp<GodSmooth, false>(st, P, pb, B, cap, rows, count);
    return plugin::trace_fill_pp<God, false>(st, P, pb, B, cap, rows, count);
}

// the table of SOCP_MODEL_GODDARD, SOCP_MODEL_DOUBLE_INTEGRATOR or SOCP_MODEL_COVID19; null for any other id
template <class God, class GodSmooth, class Covid, class DInt>
const ModelLaunchers *builtin_tables(int model_id)
{
    // the flavour this translation unit is built for: Goddard's and covid19's guide entries differ by it
    constexpr bool kRef = God::kRefOrder;
    // goddard.cpp:23-40 defaults.  Dense output always takes the general law.
    static const ModelLaunchers goddard = [] {
        ModelLaunchers t = plugin::table<God, false>(SOCP_GODDARD_NPARAMS, 10, {3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 0.0, -1.0});
        t.fields = &fields_goddard;                  // kernels_fields.hip: the same reference-order object in both flavours
        t.exact_jacobian = &exact_jacobian_goddard;  // kernels_exact_jacobian.hip: likewise
        t.sensitivity = &sensitivity_goddard;        // kernels_sensitivity.hip: likewise
        t.hamiltonian_gradient = &hamiltonian_gradient_goddard;      // kernels_hamiltonian.hip: likewise
        t.hamiltonian_jacobian = &hamiltonian_jacobian_goddard;      // kernels_hamiltonian_jacobian.hip: likewise
        t.gain = &gain_goddard;                      // kernels_gain.hip: likewise
        t.gain_free = &gain_free_goddard;            // kernels_gain_free.hip: likewise
        t.guide = kRef ? &guide_goddard : &guide_goddard_fast;   // kernels_guide.hip / kernels_guide_fast.hip: each flavour its own
        t.traj = &goddard_by_params<&plugin::traj<GodSmooth>, &plugin::traj<God>>;
        t.eval = &goddard_by_params<&plugin::eval<GodSmooth>, &plugin::eval<God>>;
        t.residual = &goddard_by_problem<&plugin::residual<GodSmooth>, &plugin::residual<God>>;
        t.fdjac = &goddard_by_problem<&plugin::fdjac<GodSmooth>, &plugin::fdjac<God>>;
        t.fdrows = &goddard_by_problem<&plugin::fdrows<GodSmooth>, &plugin::fdrows<God>>;
        t.trace = &goddard_by_problem<&plugin::trace<GodSmooth>, &plugin::trace<God>>;
        t.cost = &goddard_by_problem<&plugin::cost<GodSmooth>, &plugin::cost<God>>;
        t.move = &goddard_by_problem<&plugin::move<GodSmooth>, &plugin::move<God>>;
        t.extrema = &goddard_by_problem<&plugin::extrema<GodSmooth>, &plugin::extrema<God>>;
        t.observe = &goddard_by_problem<&plugin::observe<GodSmooth>, &plugin::observe<God>>;
        t.events = &goddard_by_problem<&plugin::events<GodSmooth>, &plugin::events<God>>;
        t.jacobi = &goddard_by_problem<&plugin::jacobi<GodSmooth>, &plugin::jacobi<God>>;
        t.trace_fill = &goddard_trace_fill<God, GodSmooth>;
        return t;
    }();
    // doubleIntegrator.cpp:26-34 defaults
    static const ModelLaunchers dint = [] {
        ModelLaunchers t = plugin::table<DInt, false>(SOCP_DINT_NPARAMS, 30, {1.0, 1.0, 0.01});
        t.fields = &fields_dint;
        t.exact_jacobian = &exact_jacobian_dint;
        t.sensitivity = &sensitivity_dint;
        t.hamiltonian_gradient = &hamiltonian_gradient_dint;
        t.hamiltonian_jacobian = &hamiltonian_jacobian_dint;
        t.gain = &gain_dint;
        t.gain_free = &gain_free_dint;
        t.guide = &guide_dint;                       // DIntFast = DIntExact: one struct, one launcher, reference order in both flavours
        return t;
    }();
    // covid19.cpp:25-38 defaults; its ModelInt integrates with its own stepNbr = 1000
    static const ModelLaunchers covid = [] {
        ModelLaunchers t = plugin::table<Covid, false>(SOCP_COVID_NPARAMS, 1000, {4, 10, 5, 1, 0.1, 1, -10, 20});
        t.fields = &fields_covid;
        t.exact_jacobian = &exact_jacobian_covid;
        t.sensitivity = &sensitivity_covid;
        t.hamiltonian_gradient = &hamiltonian_gradient_covid;
        t.hamiltonian_jacobian = &hamiltonian_jacobian_covid;
        t.gain = &gain_covid;
        t.gain_free = &gain_free_covid;
        t.guide = kRef ? &guide_covid : &guide_covid_fast;
        return t;
    }();
    switch (model_id) {
    case SOCP_MODEL_GODDARD: return &goddard;
    case SOCP_MODEL_DOUBLE_INTEGRATOR: return &dint;
    case SOCP_MODEL_COVID19: return &covid;
    default: return nullptr;
    }
}

}  // namespace socp
