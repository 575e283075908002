// plugin_impl.hpp -- the launch table of a device model (every in-tree model's is built here too: kernels_*.hip,
// builtin_tables.hpp), and how to build an OUT-OF-TREE device model into a loadable plugin.
//
// A model is one struct with the static interface the in-tree models have (models_exact.hpp):
//
//   struct MyModel {
//       static constexpr int D = ...;            // state dimension d; S = 2 d (state + costate)
//       static constexpr int S = 2 * D;
//       static constexpr int NU = ...;           // control dimension (<= 3)
//       static constexpr bool kRefOrder = true;  // true: RK4 in the reference's association order
//       __device__ static void rhs(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                  const double (&X)[S], double (&dX)[S]);              // model::Model
//       __device__ static void control_only(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                           const double (&X)[S], double (&u)[3]);      // model::Control
//       __device__ static double hamiltonian(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                            const double (&X)[S]);                     // model::Hamiltonian
//       __device__ static double switching_fn(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                             const double (&X)[S], const double (&Xp)[S]);  // SwitchingTimesFunction
//       // OPTIONAL -- model::SwitchingStateFunction (model.hpp:339-341; shooting.cpp:1535-1538): the two residual rows of state
//       // component j of an interior node whose mode is FREE; X: end of the arriving segment, Xp: the node's unknowns, Xd: the
//       // node's desired state.  Without it those rows are zero (the reference's default hook is a no-op).
//       __device__ static void switching_state(const socp::ModelParams &P, double t, int j, const double (&X)[S], const double (&Xp)[S],
//                                              const double *Xd, double &f_state, double &f_costate);
//       // OPTIONAL -- the same hook with isJac = 1 (hybrj path, shooting.cpp:1524-1538): partial derivatives of those two rows with
//       // respect to X and Xp (arrays arrive zeroed; fill the nonzeros).  The library chains them through the sensitivity block and
//       // forms the free-time column like MultipleShootingFunction does for its own rows.  Without it: zero rows.
//       __device__ static void switching_state_jac(const socp::ModelParams &P, double t, int j, const double (&X)[S], const double (&Xp)[S],
//                                                  const double *Xd, double (&dfs_dX)[S], double (&dfs_dXp)[S],
//                                                  double (&dfc_dX)[S], double (&dfc_dXp)[S]);
//       // OPTIONAL -- event channels (socp_events_batch): scalars a caller may watch along the trajectories, typically the
//       // switching function of the control law.  Plain IEEE operations if a CPU restatement is to match bit for bit.
//       static constexpr int kEventChannels = ...;                                        // 1 .. 16
//       __device__ static double event_fn(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                         const double (&X)[S], int chan);
//       // OPTIONAL -- observables (socp_observe_batch): scalars of a row whose extrema and integrals the library reduces along the
//       // trajectories -- drag, clearance, a norm.  u is control_only at the row, evaluated once by the kernel with the row's aux
//       // pair.  Plain IEEE operations if a CPU restatement is to match bit for bit.  A model with its own ComputeTraj does not
//       // get the entry.
//       static constexpr int kObservables = ...;                                          // 1 .. 16
//       static constexpr const char *kObservableNames[kObservables] = {...};
//       __device__ static void observe(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                      const double (&X)[S], const double (&u)[NU], double (&y)[kObservables]);
//       // OPTIONAL -- variational equations, for classes with modelOrder = 1 (hybrj; model.hpp:104-120,149-183):
//       __device__ static double aug_rhs(const socp::ModelParams &P, double t, int e, const double *Y);
//                 // element e of Model(t, Y, isJac = 1), Y = [X(S) ; R(S x S)], R[k][i] at Y[S (k+1) + i]  
//       __device__ static void dhamiltonian(const socp::ModelParams &P, double t, const double *X, double (&dH)[S + 1]);
//                 // Hamiltonian(t, X, isJac = 1): dH/dX (S entries), then dH/dt
//       // OPTIONAL -- the right-hand side over a number type (socp_fields_batch: exact Jacobi fields and transition matrices on
//       // dual numbers, dual.hpp).  The text of rhs on plain IEEE operations, d_sqrt / d_abs / d_exp for the functions and d_val
//       // where a comparison reads a value; a quantity that is a constant stays a plain double.  With T = double: the bits of rhs.
//       template <class T> __device__ static void rhs_t(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                                       const T (&X)[S], T (&dX)[S]);
//       // OPTIONAL -- with rhs_t, the Hamiltonian and the free-interior-time row over a number type (socp_exact_jacobian_batch: the
//       // exact Jacobian of the shooting function).  With T = double: the bits of hamiltonian / switching_fn.  kSwitchingReadsXp says
//       // whether the row is H(t, X) - H(t, Xp) (true: the library then takes -grad H(Xp) from hamiltonian_t) or does not read Xp
//       // (false, the default).  A model with its own ComputeTraj does not get the entry; one with custom final rows or a
//       // switching_state hook gets it through the two traits below.
//       template <class T> __device__ static T hamiltonian_t(const socp::ModelParams &P, double sw0, double sw1, double t, const T (&X)[S]);
//       template <class T> __device__ static T switching_fn_t(const socp::ModelParams &P, double sw0, double sw1, double t,
//                                                             const T (&X)[S], const T (&Xp)[S]);
//       static constexpr bool kSwitchingReadsXp = ...;
//       // OPTIONAL -- for a model with custom final rows (kCustomFinal): the text of final_row over a number type; final_h_offset
//       // stays plain.  With it the exact Jacobian covers the model's final rows.
//       template <class T> __device__ static T final_row_t(const socp::ModelParams &P, int j, int mode, const T (&X)[S], const double *xd);
//       // OPTIONAL -- for a model with a switching_state hook: the hook with X over a number type and Xp as the plain doubles they
//       // are.  The lanes of the segment that ENDS at the node differentiate the two rows; kSwitchingStateXpContinuous = true is the
//       // model's promise that the hook reads Xp only as -Xp[j] in f_state and -Xp[j + D] in f_costate, so that the next segment's
//       // lanes store the -1 entries of a CONTINUOUS row.  Both are required for the exact Jacobian of such a model.
//       template <class T> __device__ static void switching_state_t(const socp::ModelParams &P, double t, int j, const T (&X)[S],
//                                                                   const double (&Xp)[S], const double *Xd, T &f_state, T &f_costate);
//       static constexpr bool kSwitchingStateXpContinuous = true;
//       // OPTIONAL -- the same three texts generic in the PARAMETER view as well (socp_sensitivity_batch: exact dF/dtheta): a second
//       // template argument for anything with p[i], locals that hold a parameter `auto`, comparisons through d_val.  With
//       // socp::ModelParams the texts are what they were (tests/plugin/osc1d_sensitivity_plugin.hip):
//       template <class T, class PV> __device__ static void rhs_t(const PV &P, double sw0, double sw1, double t, const T (&X)[S], T (&dX)[S]);
//       // hamiltonian_t ALONE already gives the model socp_hamiltonian_gradient_batch: (dH/dp, -dH/dx) of that text by dual numbers,
//       // the check of rhs against it (hamiltonian_model.hpp).  And a struct with control_only and hamiltonian_t and NO rhs at all is
//       // a whole model through SOCP_DEFINE_HAMILTONIAN_PLUGIN below (tests/plugin/dint_h_plugin.hip).  A hamiltonian_t that also
//       // instantiates on the nested number socp::DualN<W, socp::Dual> gives the model socp_hamiltonian_jacobian_batch, and through
//       // SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT the exact fields, Jacobian and sensitivities (tests/plugin/dint_hx_plugin.hip).
//   };
//   SOCP_DEFINE_MODEL_PLUGIN(1001, MyModel, 3 /*nparams*/, 30 /*stepNbr*/, {1.0, 2.0, 3.0})
//
// compiled with   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared -I<repo>/socp_amd/csrc
//                       -I<repo>/include my_model.hip -o libmy_model.so
// and loaded with socp_plugin_load("libmy_model.so"); afterwards socp_ctx_create(&ctx, 1001, dev) gives a
// context on which every entry point of socp_hip.h works (trajectories, residual, FD Jacobian, dense output,
// evaluation, batched trace, batched cost, batched Move(tf) / re-grid, batched events when the model has the trait, batched Jacobi fields, batched exact fields when the model has rhs_t, batched exact shooting Jacobian when it has hamiltonian_t and switching_fn_t too, batched extrema, batched observables when the model has the trait, batched exact sensitivities when the traits are generic in the parameter view, adaptive integrator, lock-step multi-start).
#pragma once
#include "integrator.hpp"
#include "fields.hpp"
#include "exact_jacobian.hpp"
#include "sensitivity.hpp"
#include "gain.hpp"
#include "gain_free.hpp"
#include "guide.hpp"
#include "hamiltonian_model.hpp"
#include "jacobi.hpp"
#include "launch.hpp"
#include "variational.hpp"
#include "../../include/socp_plugin.h"

namespace socp {
namespace plugin {

// optional model hint kOneWavePerSimd: build and launch only the one-wave-per-SIMD instantiations (heavy
// right-hand sides whose batches never fill the chip three deep)
template <class M, class = void> struct one_wave_per_simd : std::false_type {};
template <class M> struct one_wave_per_simd<M, std::void_t<decltype(M::kOneWavePerSimd)>> : std::bool_constant<M::kOneWavePerSimd> {};

// one launch of a hot kernel: adaptive integrator -> one wave per SIMD; otherwise occupancy cap from the grid.
// ADAPTIVE: false for a kernel that has no adaptive instantiation (that arm is then not compiled)
// PP: the PERPROB template argument (always false for the trajectory kernel)
#define SOCP_PLUGIN_LAUNCH_T(KERNEL, ADAPTIVE, PP, GRID, LDS, ST, ...)                                                \
    do {                                                                                                               \
        if constexpr (ADAPTIVE) {                                                                                      \
            if (P.integrator == 1) { hipLaunchKernelGGL((KERNEL<Mdl, 1, 1, PP>), dim3(GRID), dim3(64), LDS, ST, __VA_ARGS__); break; } \
        }                                                                                                              \
        if constexpr (one_wave_per_simd<Mdl>::value)                                                                   \
            hipLaunchKernelGGL((KERNEL<Mdl, 1, 0, PP>), dim3(GRID), dim3(64), LDS, ST, __VA_ARGS__);                 \
        else switch (wpe_for(GRID)) {                                                                                  \
        case 1: hipLaunchKernelGGL((KERNEL<Mdl, 1, 0, PP>), dim3(GRID), dim3(64), LDS, ST, __VA_ARGS__); break;       \
        case 2: hipLaunchKernelGGL((KERNEL<Mdl, 2, 0, PP>), dim3(GRID), dim3(64), LDS, ST, __VA_ARGS__); break;       \
        default: hipLaunchKernelGGL((KERNEL<Mdl, 3, 0, PP>), dim3(GRID), dim3(64), LDS, ST, __VA_ARGS__); break;      \
        }                                                                                                              \
    } while (0)
#define SOCP_PLUGIN_LAUNCH(KERNEL, GRID, ST, ...) SOCP_PLUGIN_LAUNCH_T(KERNEL, true, false, GRID, 0, ST, __VA_ARGS__)
// kernels that read a shooting problem `pb`: per-problem blocks (dev_common.hpp) select the PERPROB instantiation
inline bool has_blocks(const ProblemDev &pb) { return pb.pp_params || pb.pp_time || pb.pp_xnode; }
#define SOCP_PLUGIN_LAUNCH_PB_LDS(KERNEL, ADAPTIVE, GRID, LDS, ST, ...)                                                 \
    do {                                                                                                               \
        if (has_blocks(pb)) SOCP_PLUGIN_LAUNCH_T(KERNEL, ADAPTIVE, true, GRID, LDS, ST, __VA_ARGS__);                  \
        else SOCP_PLUGIN_LAUNCH_T(KERNEL, ADAPTIVE, false, GRID, LDS, ST, __VA_ARGS__);                               \
    } while (0)
#define SOCP_PLUGIN_LAUNCH_PB(KERNEL, GRID, ST, ...) SOCP_PLUGIN_LAUNCH_PB_LDS(KERNEL, true, GRID, 0, ST, __VA_ARGS__)
// the same choice for a group kernel, which has ONE instantiation per PERPROB value (always one wave per SIMD): `shared` is its
// <..., false>, `perprob` its <..., true>; one group of `lanes` neighbouring lanes per (row, segment), 64 / lanes groups per
// single-wave workgroup (segment_views.hpp group_lane)
template <class Kernel, class... Args>
hipError_t launch_groups(hipStream_t st, const ProblemDev &pb, int B, int lanes, Kernel shared, Kernel perprob, Args... args)
{
    const int gpw = 64 / lanes;
    const long slabs = (long)B * pb.M;
    hipLaunchKernelGGL((has_blocks(pb) ? perprob : shared), dim3((unsigned)((slabs + gpw - 1) / gpw)), dim3(64), 0, st, args...);
    return hipGetLastError();
}

template <class Mdl>
hipError_t traj(hipStream_t st, const ModelParams &P, int B, const double *t0, const double *tf, const double *sw,
                const double *X0, double *Xf)
{
    if (B <= 0) return hipSuccess;
    SOCP_PLUGIN_LAUNCH(traj_lane_kernel, blocks_for(B), st, P, B, t0, tf, sw, X0, Xf);
    return hipGetLastError();
}
template <class Mdl>
hipError_t residual(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *F)
{
    if (B <= 0) return hipSuccess;
    const int R = rows_per_block(pb.M, pb.n);
    const unsigned grid = R ? (unsigned)((B + R - 1) / R) : blocks_for((long)B * pb.M);
    SOCP_PLUGIN_LAUNCH_PB_LDS(residual_lane_kernel, true, grid, (unsigned)((long)R * pb.n * 8), st, P, pb, B, Z, F, R);
    return hipGetLastError();
}
template <class Mdl>
hipError_t fdjac(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int np, int T, const int2 *pairs,
                 const double *z, const double *fvec, double eps, double *fjac)
{
    if (np <= 0 || T <= 0) return hipSuccess;
    SOCP_PLUGIN_LAUNCH_PB(fdjac_lane_kernel, blocks_for((long)np * T), st, P, pb, np, T, pairs, z, fvec, eps, fjac);
    return hipGetLastError();
}
template <class Mdl>
hipError_t fdrows(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int np, const double *z, double eps, double *rows)
{
    if (np <= 0) return hipSuccess;
    const long vrows = (long)np * (pb.n + 1);
    const int R = rows_per_block(pb.M, pb.n);
    const unsigned grid = R ? (unsigned)((vrows + R - 1) / R) : blocks_for(vrows * pb.M);
    SOCP_PLUGIN_LAUNCH_PB_LDS(fdrows_lane_kernel, true, grid, (unsigned)((long)R * pb.n * 8), st, P, pb, np, z, eps, rows, R);
    return hipGetLastError();
}
template <class Mdl>
hipError_t dense(hipStream_t st, const ModelParams &P, double t0, double tf, double sw0, double sw1, const double *X0,
                 double *out, double *times, int cap, int *rows, double *aux)
{
    if (P.integrator == 1) hipLaunchKernelGGL((traj_dense_kernel<Mdl, 1>), dim3(1), dim3(64), 0, st, P, t0, tf, sw0, sw1, X0, out, times, cap, rows, aux);
    else hipLaunchKernelGGL((traj_dense_kernel<Mdl, 0>), dim3(1), dim3(64), 0, st, P, t0, tf, sw0, sw1, X0, out, times, cap, rows, aux);
    return hipGetLastError();
}
template <class Mdl>
hipError_t eval(hipStream_t st, const ModelParams &P, int what, int B, const double *t, const double *sw, const double *X, double *out)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(eval_lane_kernel<Mdl>, dim3(blocks_for(B)), dim3(64), 0, st, P, what, B, t, sw, X, out);
    return hipGetLastError();
}

template <class Mdl>
hipError_t trace(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *rows,
                 int *count)
{
    if (B <= 0) return hipSuccess;
    SOCP_PLUGIN_LAUNCH_PB(trace_lane_kernel, blocks_for((long)B * pb.M), st, P, pb, B, Z, stride, cap, rows, count);
    return hipGetLastError();
}
// PP: the kernel's PERPROB argument -- every problem brings its own parameter block
template <class Mdl, bool PP>
hipError_t trace_fill_pp(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, int cap, double *rows, const int *count)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL((trace_fill_kernel<Mdl, PP>), dim3(blocks_for((long)B * pb.M * cap)), dim3(64), 0, st, P, pb, B, cap, rows, count);
    return hipGetLastError();
}
template <class Mdl>
hipError_t trace_fill(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, int cap, double *rows, const int *count)
{
    return pb.pp_params ? trace_fill_pp<Mdl, true>(st, P, pb, B, cap, rows, count) : trace_fill_pp<Mdl, false>(st, P, pb, B, cap, rows, count);
}

// batched extrema: one lane per (row, segment) like the trace, both integrators; what == 0 launches the state-only kernel, which
// carries neither u, H, the event channels nor their running pairs
template <class Mdl>
hipError_t extrema(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int what, double *vmin, double *vmax,
                   double *tmin, double *tmax, int *count, int *nbad)
{
    if (B <= 0) return hipSuccess;
    if (what < 0 || what > 7) return hipErrorInvalidValue;
    if (what == 0) SOCP_PLUGIN_LAUNCH_PB(extrema_state_lane_kernel, blocks_for((long)B * pb.M), st, P, pb, B, Z, vmin, vmax, tmin, tmax, count, nbad);
    else SOCP_PLUGIN_LAUNCH_PB(extrema_lane_kernel, blocks_for((long)B * pb.M), st, P, pb, B, Z, what, vmin, vmax, tmin, tmax, count, nbad);
    return hipGetLastError();
}

// batched observables: one lane per (row, segment) like the extrema, both integrators
template <class Mdl>
hipError_t observe(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *ymin, double *ymax,
                   double *tmin, double *tmax, double *integral, int *count, int *nbad)
{
    if (B <= 0) return hipSuccess;
    SOCP_PLUGIN_LAUNCH_PB(observe_lane_kernel, blocks_for((long)B * pb.M), st, P, pb, B, Z, ymin, ymax, tmin, tmax, integral, count, nbad);
    return hipGetLastError();
}

// batched cost: fixed-step integrator only, so no adaptive instantiation (the C-ABI layer refuses the adaptive integrator)
template <class Mdl>
hipError_t cost(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *out, double *Xend)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0) return hipErrorInvalidValue;
    SOCP_PLUGIN_LAUNCH_PB_LDS(cost_lane_kernel, false, blocks_for((long)B * pb.M), 0, st, P, pb, B, Z, out, Xend);
    return hipGetLastError();
}

// batched Move(tf): one lane per (row, query), both integrators
template <class Mdl>
hipError_t move(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int K, const double *tq, double *Xq,
                double *tout)
{
    if (B <= 0 || K <= 0) return hipSuccess;
    SOCP_PLUGIN_LAUNCH_PB(move_lane_kernel, blocks_for((long)B * K), st, P, pb, B, Z, K, tq, Xq, tout);
    return hipGetLastError();
}

// batched events: fixed-step integrator only, like the cost.  The state before the step stays alive beside rk4()'s working set,
// so the Goddard instantiations take more registers than the residual's and run one or two waves per SIMD whatever WPE allows;
// no instantiation has a private segment ("Batched events")
template <class Mdl>
hipError_t events(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int E, unsigned chans,
                  const double *levels, int refine, int cap, double *tev, int *id, int *count, double *Xev)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || E < 1 || E > kMaxEventWatches || refine < 0 || refine > kMaxEventRefine || cap < 1) return hipErrorInvalidValue;
    SOCP_PLUGIN_LAUNCH_PB_LDS(events_lane_kernel, false, blocks_for((long)B * pb.M), 0, st, P, pb, B, Z, E, chans, levels, refine, cap, tev, id,
                              count, Xev);
    return hipGetLastError();
}

// optional model hint kNoJacobi: leave the jacobi entry of the table empty (and its kernels unbuilt) although the model could have one
template <class M, class = void> struct no_jacobi : std::false_type {};
template <class M> struct no_jacobi<M, std::void_t<decltype(M::kNoJacobi)>> : std::bool_constant<M::kNoJacobi> {};

// batched Jacobi fields: fixed-step integrator only.  One group of D + 1 neighbouring lanes per (row, segment), 64 / (D + 1) groups
// per single-wave workgroup (jacobi.hpp); the occupancy cap follows the number of waves like every other hot kernel
template <class Mdl>
hipError_t jacobi(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double eps, int stride, int skip, int cap,
                  double *tq, double *det, int *count, int *nchange, double *tconj, double *Jend)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || stride < 1 || skip < 0 || cap < 1) return hipErrorInvalidValue;
    constexpr int gpw = 64 / (Mdl::D + 1);
    const long slabs = (long)B * pb.M;
    SOCP_PLUGIN_LAUNCH_PB_LDS(jacobi_group_kernel, false, (unsigned)((slabs + gpw - 1) / gpw), 0, st, P, pb, B, Z, eps, stride, skip, cap, tq, det,
                              count, nchange, tconj, Jend);
    return hipGetLastError();
}

// optional trait rhs_t: the right-hand side over a number type -> the model has exact fields (socp_fields_batch)
template <class M, class = void> struct has_fields : std::false_type {};
template <class M>
struct has_fields<M, std::void_t<decltype(M::template rhs_t<Dual>(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                   std::declval<const Dual (&)[M::S]>(), std::declval<Dual (&)[M::S]>()))>>
    : std::true_type {};

// batched exact fields: fixed-step integrator only.  One group of C neighbouring lanes per (row, segment), 64 / C groups per
// single-wave workgroup (fields.hpp); always one wave per SIMD.  The translation unit must be built without contraction
template <class Mdl, bool ALL>
hipError_t fields_cols(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int skip, int cap,
                       double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi)
{
    return launch_groups(st, pb, B, ALL ? Mdl::S : Mdl::D, &fields_group_kernel<Mdl, ALL, false>, &fields_group_kernel<Mdl, ALL, true>, P, pb, B, Z,
                         stride, skip, cap, tq, det, count, nchange, tconj, Phi);
}
template <class Mdl>
hipError_t fields(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip, int cap,
                  double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || cols < 0 || cols > 1 || stride < 1 || skip < 0 || cap < 1) return hipErrorInvalidValue;
    return cols ? fields_cols<Mdl, true>(st, P, pb, B, Z, stride, skip, cap, tq, det, count, nchange, tconj, Phi)
                : fields_cols<Mdl, false>(st, P, pb, B, Z, stride, skip, cap, tq, det, count, nchange, tconj, Phi);
}

// optional traits hamiltonian_t and switching_fn_t beside rhs_t, and none of the hooks the definition does not cover -> the model has
// the exact shooting Jacobian (socp_exact_jacobian_batch).  Custom final rows are covered iff the model has final_row_t, a
// switching_state hook iff it has switching_state_t and declares kSwitchingStateXpContinuous (exact_jacobian.hpp)
template <class M, class = void> struct has_exact_jacobian : std::false_type {};
template <class M>
struct has_exact_jacobian<M, std::void_t<decltype(M::template hamiltonian_t<Dual>(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                                   std::declval<const Dual (&)[M::S]>())),
                                         decltype(M::template switching_fn_t<Dual>(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                                    std::declval<const Dual (&)[M::S]>(),
                                                                                    std::declval<const Dual (&)[M::S]>()))>>
    : std::bool_constant<has_fields<M>::value && !has_custom_traj<M>::value && exact_jacobian_covers_hooks<M>::value> {};

// batched exact shooting Jacobian: fixed-step integrator only.  The matrices are zero-filled on the stream, then ONE launch: one group of
// S + 1 neighbouring lanes per (row, segment) (exact_jacobian.hpp).  The translation unit must be built without contraction
template <class Mdl>
hipError_t exact_jacobian(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(Fjac, 0, sizeof(double) * (size_t)B * pb.n * pb.n, st);
    if (e != hipSuccess) return e;
    return launch_groups(st, pb, B, Mdl::S + 1, &exact_jacobian_kernel<Mdl, false>, &exact_jacobian_kernel<Mdl, true>, P, pb, B, Z, Fjac, F);
}

// optional: rhs_t, hamiltonian_t and switching_fn_t are generic in the parameter view too (they take SeededParams, sensitivity.hpp)
// beside everything the exact Jacobian asks for, and neither custom final rows nor a switching_state hook (the sensitivities of those
// rows need a definition of their own) -> the model has exact parameter sensitivities (socp_sensitivity_batch)
template <class M, class = void> struct has_sensitivity : std::false_type {};
template <class M>
struct has_sensitivity<M, std::void_t<decltype(M::template rhs_t<Dual>(std::declval<const SeededParams &>(), 0.0, 0.0, 0.0,
                                                                        std::declval<const Dual (&)[M::S]>(), std::declval<Dual (&)[M::S]>())),
                                      decltype(M::template hamiltonian_t<Dual>(std::declval<const SeededParams &>(), 0.0, 0.0, 0.0,
                                                                                std::declval<const Dual (&)[M::S]>())),
                                      decltype(M::template switching_fn_t<Dual>(std::declval<const SeededParams &>(), 0.0, 0.0, 0.0,
                                                                                 std::declval<const Dual (&)[M::S]>(),
                                                                                 std::declval<const Dual (&)[M::S]>()))>>
    : std::bool_constant<has_exact_jacobian<M>::value && !has_custom_final<M>::value && !has_switching_state<M>::value> {};

// the integrating directions of ONE kind of socp_sensitivity_batch: fixed-step integrator only.  G is zero-filled by the caller; one
// group of dirs.n neighbouring lanes per (row, segment), 64 / dirs.n groups per single-wave workgroup (sensitivity.hpp); always one wave
// per SIMD.  The translation unit must be built without contraction
template <class Mdl, int KIND>
hipError_t sensitivity_kind(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                            double *G)
{
    return launch_groups(st, pb, B, dirs.n, &sensitivity_kernel<Mdl, KIND, false>, &sensitivity_kernel<Mdl, KIND, true>, P, pb, B, Z, dirs, K, G);
}
template <class Mdl>
hipError_t sensitivity(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                       double *G)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || dirs.n < 1 || dirs.n > kMaxTangentDirs || K < dirs.n || K > kMaxTangentDirs) return hipErrorInvalidValue;
    if (dirs.kind == kSensParam) return sensitivity_kind<Mdl, kSensParam>(st, P, pb, B, Z, dirs, K, G);
    if (dirs.kind == kSensTime) return sensitivity_kind<Mdl, kSensTime>(st, P, pb, B, Z, dirs, K, G);
    return hipErrorInvalidValue;
}

// rhs_t and none of the hooks the definition does not cover -> the model has the neighbouring-extremal gains (socp_gain_batch):
// has_exact_jacobian's condition without the Hamiltonian traits
template <class M>
struct has_gain : std::bool_constant<has_fields<M>::value && !has_custom_traj<M>::value && !has_custom_final<M>::value &&
                                     !has_switching_state<M>::value> {};

// batched neighbouring-extremal gains: fixed-step integrator only.  Launch 1: the blocks, one group of S neighbouring lanes per (row,
// segment), always one wave per SIMD; launch 2: the backward sweep, one group of D neighbouring lanes per row (gain.hpp).  The
// translation unit must be built without contraction
template <class Mdl>
hipError_t gain(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq, double *Xq,
                int *count, double *Psi, double *Wq, double *A, double *Kp)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || stride < 1 || cap < 1 || !Psi || !A) return hipErrorInvalidValue;
    const hipError_t e = launch_groups(st, pb, B, Mdl::S, &gain_blocks_kernel<Mdl, false>, &gain_blocks_kernel<Mdl, true>, P, pb, B, Z, stride,
                                       cap, tq, Xq, count, Psi);
    if (e != hipSuccess) return e;
    constexpr int gpw = 64 / Mdl::D;
    hipLaunchKernelGGL(gain_sweep_kernel<Mdl>, dim3((unsigned)(((long)B + gpw - 1) / gpw)), dim3(64), 0, st, pb, B, cap, count, Psi, Wq, A, Kp);
    return hipGetLastError();
}

// has_gain's condition and the hamiltonian_t trait -> the model has the gains with a free final time (socp_gain_free_batch): the H row
// of the bordered sweep is the gradient of the model's own Hamiltonian text
template <class M, class = void> struct has_gain_free : std::false_type {};
template <class M>
struct has_gain_free<M, std::void_t<decltype(M::template hamiltonian_t<Dual>(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                              std::declval<const Dual (&)[M::S]>()))>>
    : std::bool_constant<has_gain<M>::value> {};

// batched neighbouring-extremal gains with a free final time: fixed-step integrator only.  Launch 1: the blocks, one group of S + 1
// neighbouring lanes per (row, segment), always one wave per SIMD; launch 2: the bordered backward sweep, one group of D + 1
// neighbouring lanes per row (gain_free.hpp).  The translation unit must be built without contraction
template <class Mdl>
hipError_t gain_free(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                     double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || stride < 1 || cap < 1 || !Psi || !Len || !gradH || !A) return hipErrorInvalidValue;
    const hipError_t e = launch_groups(st, pb, B, Mdl::S + 1, &gain_free_blocks_kernel<Mdl, false>, &gain_free_blocks_kernel<Mdl, true>, P, pb, B,
                                       Z, stride, cap, tq, Xq, count, Psi, Len, gradH);
    if (e != hipSuccess) return e;
    constexpr int gpw = 64 / (Mdl::D + 1);
    hipLaunchKernelGGL(gain_free_sweep_kernel<Mdl>, dim3((unsigned)(((long)B + gpw - 1) / gpw)), dim3(64), 0, st, pb, B, cap, count, Psi, Len,
                       gradH, Wq, A, Ke);
    return hipGetLastError();
}

// rhs and none of the hooks has_gain excludes -> the model has the closed-loop flight (socp_guide_batch).  rhs_t is NOT needed: the
// flight is a plain trajectory; the entry points ask for the gain entry of the structure at hand, so that the tables can exist
template <class M>
struct has_guide : std::bool_constant<!has_custom_traj<M>::value && !has_custom_final<M>::value && !has_switching_state<M>::value> {};

// closed-loop flight of K cases per row: fixed-step integrator only.  ONE launch, one lane per (row, case) (guide.hpp); the occupancy
// cap follows the number of waves like every other hot kernel.  Reference order: the translation unit must be built without contraction
template <class Mdl>
hipError_t guide(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A)
{
    if (B <= 0) return hipSuccess;
    if (P.integrator != 0 || A.K < 1 || A.stride < 1 || A.cap < 1 || A.every < 0 || !A.Xq || !A.Kg || !A.dX0 || !A.info || !A.count || !A.Xf ||
        !A.miss || !A.nupd || !A.nskip)
        return hipErrorInvalidValue;
    if (free_tf) SOCP_PLUGIN_LAUNCH_PB_LDS(guide_free_kernel, false, blocks_for((long)B * A.K), 0, st, P, pb, B, Z, A);
    else SOCP_PLUGIN_LAUNCH_PB_LDS(guide_kernel, false, blocks_for((long)B * A.K), 0, st, P, pb, B, Z, A);
    return hipGetLastError();
}

// optional trait hamiltonian_t alone -> the model has the Hamiltonian gradient (socp_hamiltonian_gradient_batch): the check of a
// hand-written rhs against its Hamiltonian text (hamiltonian_model.hpp)
template <class M, class = void> struct has_hamiltonian_gradient : std::false_type {};
template <class M>
struct has_hamiltonian_gradient<M, std::void_t<decltype(M::template hamiltonian_t<DualN<1>>(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                                            std::declval<const DualN<1> (&)[M::S]>()))>>
    : std::true_type {};

// one lane per point, one launch, like eval.  The translation unit must be built without contraction
template <class Mdl>
hipError_t hamiltonian_gradient(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *G)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(hamiltonian_gradient_kernel<Mdl>, dim3(blocks_for(B)), dim3(64), 0, st, P, B, t, sw, X, G);
    return hipGetLastError();
}

// hamiltonian_t instantiates on the nested number too -> the model has the Jacobian of the Hamiltonian vector field
// (socp_hamiltonian_jacobian_batch)
template <class M, class = void> struct has_hamiltonian_jacobian : std::false_type {};
template <class M>
struct has_hamiltonian_jacobian<M, std::void_t<decltype(M::template hamiltonian_t<DualN<1, Dual>>(std::declval<const ModelParams &>(), 0.0, 0.0, 0.0,
                                                                                                  std::declval<const DualN<1, Dual> (&)[M::S]>()))>>
    : std::true_type {};

// one lane per point, one launch, like hamiltonian_gradient.  W: the inner pass width (the model's kNestedGradientWidth, else its
// kGradientWidth, unless the caller chooses one for registers).  The translation unit must be built without contraction
template <class Mdl, int W = nested_gradient_width<Mdl>::value>
hipError_t hamiltonian_jacobian(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *A,
                                double *G)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL((hamiltonian_jacobian_kernel<Mdl, W>), dim3(blocks_for(B)), dim3(64), 0, st, P, B, t, sw, X, A, G);
    return hipGetLastError();
}

// optional trait: the model integrates its variational equations (aug_rhs + dhamiltonian) -> the hybrj path works for it
template <class M, class = void> struct has_variational : std::false_type {};
template <class M>
struct has_variational<M, std::void_t<decltype(M::aug_rhs(std::declval<const ModelParams &>(), 0.0, 0, (const double *)nullptr)),
                                      decltype(M::dhamiltonian(std::declval<const ModelParams &>(), 0.0, (const double *)nullptr,
                                                               std::declval<double (&)[M::S + 1]>()))>> : std::true_type {};

// FIELDS = false: leave the fields, exact_jacobian, sensitivity, hamiltonian_gradient, hamiltonian_jacobian, gain, gain_free and guide
// entries to the caller (the in-tree models' entries live in kernels_fields.hip, kernels_exact_jacobian.hip, kernels_sensitivity.hip,
// kernels_hamiltonian.hip, kernels_hamiltonian_jacobian.hip, kernels_gain.hip, kernels_gain_free.hip and kernels_guide[_fast].hip,
// builtin_tables.hpp)
template <class Mdl, bool FIELDS = true>
ModelLaunchers table(int nparams, int step_nbr, std::initializer_list<double> defaults)
{
    static_assert(Mdl::S == 2 * Mdl::D, "state vector is [state ; costate]");
    static_assert(Mdl::NU >= 1 && Mdl::NU <= 3, "control dimension 1..3");
    ModelLaunchers t{};
    t.abi = kPluginAbi; t.dim = Mdl::D; t.control_dim = Mdl::NU; t.nparams = nparams; t.default_step_nbr = step_nbr;
    int i = 0;
    for (double v : defaults) if (i < kMaxParams) t.default_params[i++] = v;
    t.traj = &traj<Mdl>; t.residual = &residual<Mdl>; t.fdjac = &fdjac<Mdl>; t.fdrows = &fdrows<Mdl>;
    t.dense = &dense<Mdl>; t.eval = &eval<Mdl>; t.trace = &trace<Mdl>; t.trace_fill = &trace_fill<Mdl>;
    t.move = &move<Mdl>; t.extrema = &extrema<Mdl>;
    if constexpr (!has_custom_traj<Mdl>::value) t.cost = &cost<Mdl>;     // a model with its own ComputeTraj has no cost kernel
    if constexpr (event_channels<Mdl>::value > 0 && !has_custom_traj<Mdl>::value) {
        static_assert(event_channels<Mdl>::value <= 16, "a watch's channel travels in four bits");
        t.event_channels = event_channels<Mdl>::value; t.events = &events<Mdl>;
    }
    if constexpr (observables<Mdl>::value > 0 && !has_custom_traj<Mdl>::value) {
        static_assert(observables<Mdl>::value <= 16, "at most 16 observables: their running pairs and sums live in registers");
        static_assert(sizeof(Mdl::kObservableNames) / sizeof(Mdl::kObservableNames[0]) == observables<Mdl>::value, "one name per observable");
        t.observables = observables<Mdl>::value; t.observable_names = Mdl::kObservableNames; t.observe = &observe<Mdl>;
    }
    if constexpr (!has_custom_traj<Mdl>::value && !no_jacobi<Mdl>::value) t.jacobi = &jacobi<Mdl>;   // nor Jacobi fields (their chart changes rewrite the costate)
    if constexpr (FIELDS && has_fields<Mdl>::value && !has_custom_traj<Mdl>::value) t.fields = &fields<Mdl>;
    if constexpr (FIELDS && has_exact_jacobian<Mdl>::value) t.exact_jacobian = &exact_jacobian<Mdl>;
    if constexpr (FIELDS && has_sensitivity<Mdl>::value) t.sensitivity = &sensitivity<Mdl>;
    if constexpr (FIELDS && has_hamiltonian_gradient<Mdl>::value) t.hamiltonian_gradient = &hamiltonian_gradient<Mdl>;
    if constexpr (FIELDS && has_hamiltonian_jacobian<Mdl>::value) t.hamiltonian_jacobian = &hamiltonian_jacobian<Mdl>;
    if constexpr (FIELDS && has_gain<Mdl>::value) t.gain = &gain<Mdl>;
    if constexpr (FIELDS && has_gain_free<Mdl>::value) t.gain_free = &gain_free<Mdl>;
    if constexpr (FIELDS && has_guide<Mdl>::value) t.guide = &guide<Mdl>;
    if constexpr (has_variational<Mdl>::value) {
        t.var_traj = &varimpl::traj<Mdl>; t.var_jacobian = &varimpl::jacobian<Mdl>; t.var_eval = &varimpl::eval<Mdl>;
    }
    return t;
}

}  // namespace plugin
}  // namespace socp

// defines the entry point socp_plugin_load() looks for
#define SOCP_DEFINE_MODEL_PLUGIN(MODEL_ID, MDL, NPARAMS, STEP_NBR, ...)                                   \
    extern "C" int socp_plugin_register(void)                                                             \
    {                                                                                                     \
        static const socp::ModelLaunchers t = socp::plugin::table<MDL>(NPARAMS, STEP_NBR, __VA_ARGS__);   \
        return socp_register_model(MODEL_ID, &t, (int)sizeof(t));                                         \
    }

// the same for a model written from its Hamiltonian alone: MDL brings control_only and hamiltonian_t, the right-hand side is
// symplectic_gradient (hamiltonian_model.hpp: plugin::FromHamiltonian).  Build the plugin with -ffp-contract=off
#define SOCP_DEFINE_HAMILTONIAN_PLUGIN(MODEL_ID, MDL, NPARAMS, STEP_NBR, ...)                             \
    SOCP_DEFINE_MODEL_PLUGIN(MODEL_ID, socp::plugin::FromHamiltonian<MDL>, NPARAMS, STEP_NBR, __VA_ARGS__)

// the same with the three texts over a number type as well (plugin::FromHamiltonianExact): exact fields, the exact shooting Jacobian
// and, when MDL's hamiltonian_t is generic in the parameter view, exact sensitivities.  MDL's hamiltonian_t must instantiate on
// socp::DualN<W, socp::Dual>
#define SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT(MODEL_ID, MDL, NPARAMS, STEP_NBR, ...)                       \
    SOCP_DEFINE_MODEL_PLUGIN(MODEL_ID, socp::plugin::FromHamiltonianExact<MDL>, NPARAMS, STEP_NBR, __VA_ARGS__)
