// launch.hpp -- what the C-ABI layer launches through: every model, in-tree or plugin, is a ModelLaunchers table, one per
// arithmetic flavour (translation unit); plus the launch geometry the tables share and the model-independent launchers.
#pragma once
#include <cstdlib>

#include "dev_common.hpp"

namespace socp {

// ---- launch geometry of the tables' launchers (plugin_impl.hpp) ----
constexpr int kNumSIMD = 1024;                       // MI355X: 256 CUs x 4 SIMDs

inline unsigned blocks_for(long n) { return (unsigned)((n + 63) / 64); }

// Fill-the-chip placement.  Workgroups here are single waves that keep their trajectory in registers for
// milliseconds.  The dispatcher packs them as deep as registers allow (3 per SIMD at <= 168 VGPRs) and a CU
// does not balance single-wave workgroups over its 4 SIMDs, so a grid of W < 3072 waves would time-slice
// three waves on some SIMDs while others idle (measured: 960 waves took 2x, 1920 waves 3x the single-wave
// time).  Every hot kernel is therefore instantiated with an occupancy cap WPE in {1,2,3}
// (amdgpu_waves_per_eu) and the launcher picks WPE = ceil(W / 1024 SIMDs): up to 1024 waves run one per
// SIMD, up to 2048 two per SIMD, beyond that three.
inline int wpe_for(long waves)
{
    const long k = (waves + kNumSIMD - 1) / kNumSIMD;
    return k < 1 ? 1 : (k > 3 ? 3 : (int)k);
}

// rows per workgroup of the row-owned-tile kernels (integrator.hpp): whole rows, M lanes each, tile <= 32 KiB;
// 0 = direct stores
inline int rows_per_block(int M, int n)
{
    static const bool off = [] { const char *e = std::getenv("SOCP_ROW_TILES"); return e && e[0] == '0'; }();
    if (off || M > 64) return 0;                      // SOCP_ROW_TILES=0: direct stores (A/B measurements)
    int R = 64 / M;
    const long bytes = (long)R * n * 8;
    if (bytes > 32 * 1024) R = (int)(32 * 1024 / ((long)n * 8));
    return R < 1 ? 0 : R;
}

// Launch table of a model (plugin_impl.hpp): what the C-ABI layer calls.  In-tree models bring theirs below (the Goddard table
// picks the control law per launch, builtin_tables.hpp); an out-of-tree model registers one (include/socp_plugin.h).
constexpr int kPluginAbi = 20;     // 3: ProblemDev carries per-problem blocks; 4: optional variational launchers; 5: ModelParams carries the map table;
                                   // 6: batched trace launchers; 7: batched cost launcher; 8: batched move launcher;
                                   // kPluginAbi = 9: batched events launcher; kPluginAbi = 10: batched Jacobi-field launcher;
                                   // kPluginAbi = 11: batched exact-fields launcher
                                   // kPluginAbi = 12: batched extrema launcher
                                   // kPluginAbi = 13: batched exact shooting-Jacobian launcher
                                   // kPluginAbi = 14: batched observables launcher
                                   // kPluginAbi = 15: batched exact-sensitivities launcher
                                   // kPluginAbi = 16: Hamiltonian-gradient launcher
                                   // kPluginAbi = 17: Hamiltonian-Jacobian launcher
                                   // kPluginAbi = 18: batched neighbouring-extremal gain launcher
                                   // kPluginAbi = 19: the same with a free final time (bordered sweep)
                                   // kPluginAbi = 20: closed-loop guidance launcher (until then `constexpr int kPluginAbi = 19;`)
// the integrating directions of one kind of socp_sensitivity_batch as they travel to the kernel (sensitivity.hpp): 16 bits per
// direction, four to a word.  slot: the direction's place k in the call's table (4 bits each); index: the parameter or the node
constexpr int kSensParam = 0, kSensTime = 1;
struct SensDirs {
    int kind, n;                                     // kSensParam / kSensTime; 1 <= n <= 16
    unsigned long long slot, index[4];
};

// socp_guide_batch as it travels to the kernel (guide.hpp): K cases per row, the tables of the gain call with the same stride and cap
// (Xq[B][M][cap][s], Kg[B][M][cap][ldk d], info[B][M][cap], count[B][M]), the deviations dX0[B][K][d], `every`; the outputs per case,
// tf, dxmax and Xs null when not wanted
struct GuideArgs {
    int K, stride, cap, every;
    const double *Xq, *Kg, *dX0;
    const int *info, *count;
    double *Xf, *miss, *tf, *dxmax, *Xs;
    int *nupd, *nskip;
};

struct ModelLaunchers {
    int abi, dim, control_dim, nparams, default_step_nbr;
    double default_params[kMaxParams];
    hipError_t (*traj)(hipStream_t, const ModelParams &, int, const double *, const double *, const double *, const double *, double *);
    hipError_t (*residual)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double *);
    hipError_t (*fdjac)(hipStream_t, const ModelParams &, const ProblemDev &, int, int, const int2 *, const double *, const double *, double, double *);
    hipError_t (*fdrows)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double, double *);
    hipError_t (*dense)(hipStream_t, const ModelParams &, double, double, double, double, const double *, double *, double *, int, int *, double *);
    hipError_t (*eval)(hipStream_t, const ModelParams &, int, int, const double *, const double *, const double *, double *);
    // variational equations (modelOrder 1, hybrj path): all three null when the model has none
    hipError_t (*var_traj)(hipStream_t, const ModelParams &, int, const double *, const double *, const double *, double *);
    hipError_t (*var_jacobian)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double *, double *, double *, double *, double *);
    hipError_t (*var_eval)(hipStream_t, const ModelParams &, int, int, const double *, const double *, int, double *);
    // batched trace (socp_trace_batch): kept rows' t, X, aux and their number; then u and H of the stored rows in place
    hipError_t (*trace)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, int, double *, int *);
    hipError_t (*trace_fill)(hipStream_t, const ModelParams &, const ProblemDev &, int, int, double *, const int *);
    // batched cost (socp_cost_batch): cost[B][M] and, unless null, Xend[B][M][S]; fixed-step integrator only.  Null: the model has
    // no running-cost kernel (one with its own ComputeTraj)
    hipError_t (*cost)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double *, double *);
    // batched Move(tf) (socp_move_batch): Z[B][n], tq[B][K] -> Xq[B][K][S] and, unless null, tout[B][K]; both integrators
    hipError_t (*move)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, const double *, double *, double *);
    // batched events (socp_events_batch): Z[B][n], E watches (channel of watch e: bits 4e .. 4e+3 of `chans`), levels[B][E],
    // refine, cap -> tev[B][M][cap], id[B][M][cap], count[B][M] and, unless null, Xev[B][M][cap][S]; fixed-step integrator only.
    // event_channels = 0 and a null entry: the model has no event channels (no kEventChannels / event_fn trait)
    int event_channels;
    hipError_t (*events)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, unsigned, const double *, int, int,
                         double *, int *, int *, double *);
    // batched Jacobi fields (socp_jacobi_batch): Z[B][n], eps, stride, skip, cap -> tq[B][M][cap], det[B][M][cap], count[B][M],
    // nchange[B][M], tconj[B][M] and, unless null, Jend[B][M][d][d]; fixed-step integrator only.  Null: the model has its own
    // ComputeTraj, or the entry is not offered for it
    hipError_t (*jacobi)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double, int, int, int, double *, double *,
                         int *, int *, double *, double *);
    // batched exact fields (socp_fields_batch): Z[B][n], cols (0: the d costate columns, 1: all s), stride, skip, cap ->
    // tq[B][M][cap], det[B][M][cap], count[B][M], nchange[B][M], tconj[B][M] and, unless null, Phi[B][M][s][C]; fixed-step integrator
    // only.  Null: the model has its own ComputeTraj, or no rhs_t trait (plugin_impl.hpp).  The in-tree models' entries live in
    // kernels_fields.hip, one object without contraction that both flavours' tables point to
    hipError_t (*fields)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, int, int, int, double *, double *,
                         int *, int *, double *, double *);
    // batched extrema (socp_extrema_batch): Z[B][n], what (bit 0: u, 1: H, 2: the event channels; the state always) -> vmin, vmax,
    // tmin, tmax [B][M][C] (tmin, tmax may be null), count[B][M], nbad[B][M] (may be null), C = 2d + NU + 1 + event_channels; both
    // integrators, one launch.  Every model with a trace entry has it
    hipError_t (*extrema)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, double *, double *, double *,
                          double *, int *, int *);
    // batched exact shooting Jacobian (socp_exact_jacobian_batch): Z[B][n] -> Fjac[B][n*n] column-major (zero-filled on the stream,
    // then ONE launch) and, unless null, F[B][n]; fixed-step integrator only.  Null: the model lacks one of the traits rhs_t,
    // hamiltonian_t, switching_fn_t, or has its own ComputeTraj, custom final rows without final_row_t or a switching_state hook without
    // switching_state_t (plugin_impl.hpp).  The in-tree models' entries live in kernels_exact_jacobian.hip and kernels_vtol_exact.hip,
    // objects without contraction that both flavours' tables point to
    hipError_t (*exact_jacobian)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double *, double *);
    // batched observables (socp_observe_batch): Z[B][n] -> ymin, ymax, tmin, tmax, integral [B][M][NO] (tmin, tmax, integral may be
    // null), count[B][M], nbad[B][M] (may be null), NO = observables; both integrators, one launch.  observables = 0 and null
    // entries: the model has no observables (no kObservables / kObservableNames / observe trait) or its own ComputeTraj
    int observables;
    const char *const *observable_names;
    hipError_t (*observe)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, double *, double *, double *, double *,
                          double *, int *, int *);
    // batched exact sensitivities (socp_sensitivity_batch): Z[B][n], the integrating directions of ONE kind, K -> their rows of
    // G[B][K][n] (zero-filled by the caller; ONE launch); fixed-step integrator only.  Null: the model has no exact_jacobian entry, or
    // its rhs_t / hamiltonian_t / switching_fn_t are not generic in the parameter view (plugin_impl.hpp).  The in-tree models' entries
    // live in kernels_sensitivity.hip, one object without contraction that both flavours' tables point to
    hipError_t (*sensitivity)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, const SensDirs &, int, double *);
    // Hamiltonian gradient (socp_hamiltonian_gradient_batch): t[B], sw[B][2] or null, X[B][S] -> G[B][S] = (dH/dp, -dH/dx) of the
    // model's hamiltonian_t by dual numbers (hamiltonian_model.hpp), the arguments of `eval`; ONE launch.  Null: the model has no
    // hamiltonian_t trait (plugin_impl.hpp).  The in-tree models' entries live in kernels_hamiltonian.hip, one object without
    // contraction that both flavours' tables point to
    hipError_t (*hamiltonian_gradient)(hipStream_t, const ModelParams &, int, const double *, const double *, const double *, double *);
    // Jacobian of the Hamiltonian vector field (socp_hamiltonian_jacobian_batch): t[B], sw[B][2] or null, X[B][S] -> A[B][S * S]
    // column-major, A[S j + i] = dG_i/dX_j of the gradient above by nested dual numbers, and its value parts into G[B][S] unless null;
    // ONE launch.  Null: the model's hamiltonian_t does not instantiate on the nested number (plugin_impl.hpp).  The in-tree models'
    // entries live in kernels_hamiltonian_jacobian.hip, one object without contraction that both flavours' tables point to
    hipError_t (*hamiltonian_jacobian)(hipStream_t, const ModelParams &, int, const double *, const double *, const double *, double *,
                                       double *);
    // batched neighbouring-extremal gains (socp_gain_batch): Z[B][n], stride, cap -> tq[B][M][cap], Xq[B][M][cap][s] (may be null),
    // count[B][M], the blocks Psi[B][M][cap][s][s], then Wq[B][M][cap][d][s] (may be null), the elimination's matrices
    // A[B][M][cap][d*d] column-major and its right-hand sides in Kp[B][M][cap][d*d]; fixed-step integrator only.  TWO launches (the
    // blocks, the backward sweep); the caller runs the elimination.  Null: the model has no rhs_t trait, or has a switching_state hook,
    // custom final rows or its own ComputeTraj (plugin_impl.hpp).  The in-tree models' entries live in kernels_gain.hip, one object
    // without contraction that both flavours' tables point to
    hipError_t (*gain)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, int, double *, double *, int *, double *,
                       double *, double *, double *);
    // the same with a FREE final time (socp_gain_free_batch): Z[B][n], stride, cap -> tq, Xq (may be null), count, the blocks
    // Psi[B][M][cap][s][s] and their length columns Len[B][M][cap][s], grad H at the final state gradH[B][s], then
    // Wq[B][M][cap][(d+1)(s+1)] (may be null), the elimination's bordered matrices A[B][M][cap][(d+1)(d+1)] column-major and its
    // right-hand sides in Ke[B][M][cap][d][d+1]; fixed-step integrator only.  TWO launches; the caller runs the elimination.  Null: the
    // model has no gain entry or no hamiltonian_t trait.  The in-tree models' entries live in kernels_gain_free.hip, one object without
    // contraction that both flavours' tables point to
    hipError_t (*gain_free)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, int, double *, double *, int *,
                            double *, double *, double *, double *, double *, double *);
    // closed-loop flight under the sampled neighbouring-extremal law (socp_guide_batch): Z[B][n], free_tf (0: the tables are
    // socp_gain_batch's, ldk = d; 1: socp_gain_free_batch's, ldk = d + 1, and the final time is re-timed), the tables and the outputs
    // of GuideArgs; fixed-step integrator only.  ONE launch, one lane per (row, case).  Null: the model has a switching_state hook,
    // custom final rows or its own ComputeTraj (plugin_impl.hpp).  UNLIKE the gain entries the two flavours' tables point to their OWN
    // launcher: the in-tree models' entries live in kernels_guide.hip (no contraction) and kernels_guide_fast.hip (contraction on; the
    // double integrator, one struct in both flavours, has the reference-order launcher in both tables)
    hipError_t (*guide)(hipStream_t, const ModelParams &, const ProblemDev &, int, const double *, int, const GuideArgs &);
};

// flavour-independent: Jacobian from the rows of fdrows (differences and one division per entry)
hipError_t fd_diff(hipStream_t st, int n, int np, const double *z, double eps, const double *rows, double *fjac);
// socp_tangent_batch (kernels_tangent.hip, built once per flavour: the plain names are the no-contraction object's, the _fast names
// the contraction-on object's).  The directions travel as a kernel argument.
constexpr int kMaxTangentDirs = 16;
constexpr int kLinsolveLdsBytes = 64 * 1024;         // LDS a linsolve workgroup may take: two such workgroups share a CU's 160 KiB
constexpr int kLinsolveScratch = 16;                  // doubles per team behind its matrix: candidate values, candidate rows, the not-finite flag
// team geometry of the elimination from n: W wavefronts per problem, T problems per workgroup (kernels_tangent.hip)
inline int linsolve_waves(int n) { return n <= 64 ? 1 : (n <= 128 ? 2 : 4); }
inline int linsolve_teams(int n) { return n <= 16 ? 4 : 1; }
// whether a workgroup's teams fit the LDS at least on the HBM path (a pivot row, a multiplier column and the scratch per team)
inline bool linsolve_fits(int n, int K)
{
    return sizeof(double) * linsolve_teams(n) * ((size_t)2 * n + K + kLinsolveScratch) <= (size_t)kLinsolveLdsBytes;
}
struct TangentDirs { int kind[kMaxTangentDirs], index[kMaxTangentDirs]; };
// block rows r = kk B + b (kk = 0: row b's own block or the shared one; kk = k + 1: direction k's entry moved by h[b][k]) into
// wP[R][nparams + 2], wT[R][M+1], wX[R][(M+1) 2d], the replicated unknowns into wZ[R][n], the steps into wH[B][K];  R = B (K + 1)
hipError_t tangent_expand(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int nparams, int B, int K, const TangentDirs &dirs,
                          double e, const double *Z, double *wP, double *wT, double *wX, double *wZ, double *wH);
hipError_t tangent_expand_fast(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int nparams, int B, int K, const TangentDirs &dirs,
                               double e, const double *Z, double *wP, double *wT, double *wX, double *wZ, double *wH);
// G = (F[(k+1) B + b] - F[b]) / h[b][k] from the residual rows F[R][n]: -G into rhs[B][K][n], G into Fp[B][K][n] unless null
hipError_t tangent_diff(hipStream_t st, int B, int K, int n, const double *F, const double *H, double *rhs, double *Fp);
hipError_t tangent_diff_fast(hipStream_t st, int B, int K, int n, const double *F, const double *H, double *rhs, double *Fp);
// A[B][n*n] column-major, Y[B][K][n] -> the solutions in Y, info[B]; hipErrorInvalidValue unless linsolve_fits(n, K)
hipError_t linsolve(hipStream_t st, int B, int n, int K, double *A, double *Y, int *info);
hipError_t linsolve_fast(hipStream_t st, int B, int n, int K, double *A, double *Y, int *info);
// the same elimination over the slots [B][cap] of which only the first min(count[b], cap) of each b hold a problem: the others are
// neither read nor written (socp_gain_batch).  Reference order only
hipError_t linsolve_slots(hipStream_t st, int B, int cap, const int *count, int n, int K, double *A, double *Y, int *info);
// socp_branch_batch (kernels_branch.hip: one object without contraction, for both flavours).  The direction and the options travel as
// a kernel argument; the row state lives in the caller's workspace.
struct BranchArgs {
    int kind, index, dir, kfast, max_corr, have_goal, cap;
    double e, wtheta, h0, hmin, hmax, grow, ftol, goal;          // e = sqrt(max(epsfcn, DBL_EPSILON))
};
// per row: the evaluation point v, the last accepted point y and the unit tangent t there ([B][n+1]: z then lambda), the step
// length h, the parameter step h_theta and ||F0||inf of this round, the corrector count k, this round's case and the elimination's
// info; live: the number of unfinished rows after the last update
struct BranchState {
    double *v, *y, *t, *h, *hth, *rn;
    int *k, *kase, *info, *live;
};
struct BranchOut {
    double *Y, *ttheta, *rnorm;
    int *count, *nfold, *ifold, *status, *nreject;
    double *hlast, *zgoal;                                       // zgoal may be null
};
// block rows r = kk B + b (kk = 0: theta = fl(lambda wtheta) of row b's evaluation point, kk = 1: theta + h_theta) into wP / wT / wX
// [2B][..], the evaluation point's z into wZ[2B][n], h_theta into the state, live = 0; first: the state and the outputs are set
// from Z and the row's blocks first
hipError_t branch_expand(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int nparams, int B, const BranchArgs &A, int first,
                         const double *Z, const BranchState &S, const BranchOut &O, double *wP, double *wT, double *wX, double *wZ);
// from the residual rows F[2B][n] and J[B][n*n]: ||F0||inf and the row's case into the state, the bordered matrix Mx[B][(n+1)^2]
// column-major, the right-hand side rhs[B][n+1]
hipError_t branch_assemble(hipStream_t st, int B, int n, const BranchArgs &A, int first, const double *F, const double *J,
                           const BranchState &S, const int *status, double *Mx, double *rhs);
// the transitions of every unfinished row from the solutions X[B][n+1]
hipError_t branch_update(hipStream_t st, int B, int n, const BranchArgs &A, const BranchState &S, const BranchOut &O, const double *X);
// socp_newton_batch (kernels_newton.hip: one object without contraction, for both flavours).  The options travel as a kernel argument;
// the row state is the caller's outputs (y = Zout, rn = rnorm, the counters, status) plus F0 in the workspace.
struct NewtonArgs {
    int trials, rounds;
    double ftol, xtol;
};
struct NewtonOut {
    double *Zout, *Fout, *rnorm, *dnorm;                          // Fout may be null
    int *iters, *nhalf, *status;
    double *rhist;                                                // may be null
};
// F0[B][n] by row.  By compact slot s: the accepted point cZ, its residual cF, the right-hand side and then the step cR ([B][n] each),
// the slot's block rows cP / cT / cX, the elimination's info.  By trial row r = s trials + k: tZ, tF ([B trials][n]) and the block
// rows tP / tT / tX.  list[s]: the row of slot s; bcount: the compaction's per-workgroup counts; live: the number of unfinished rows
struct NewtonWork {
    double *F0, *cZ, *cF, *cR, *cP, *cT, *cX, *tZ, *tF, *tP, *tT, *tX;
    int *list, *info, *bcount, *live;
};
inline int newton_scan_blocks(int B) { return (B + 255) / 256; }  // workgroups of the compaction: 256 rows each
// from F0 = F(Z): every output and the state of every row (BAD_START, CONVERGED with iters = 0, or unfinished); slot b <- row b
hipError_t newton_start(hipStream_t st, const ProblemDev &pb, int B, int n, const NewtonArgs &A, const double *Z, const NewtonWork &W,
                        const NewtonOut &O);
// the unfinished rows (status == 0) in ascending order into list[0 .. live): three launches (count, scan, scatter), none waits on another
hipError_t newton_compact(hipStream_t st, int B, const int *status, const NewtonWork &W);
// slots 0 .. min(slots, live) - 1: y, F0, -F0 and the row's own block rows (those pb has) into the compact buffers
hipError_t newton_gather(hipStream_t st, const ProblemDev &pb, int slots, int n, const NewtonWork &W, const NewtonOut &O);
// every slot: tZ[s trials + k] = cZ[s] + fl(2^-k cR[s]) and the slot's block rows replicated
hipError_t newton_trials(hipStream_t st, const ProblemDev &pb, int slots, int n, int trials, const NewtonWork &W);
// slots 0 .. min(slots, live) - 1: the step's norm, the first trial that passes its bar, the accepted row scattered back, the end tests
hipError_t newton_update(hipStream_t st, int slots, int n, const NewtonArgs &A, const NewtonWork &W, const NewtonOut &O);
// socp_svd_batch_dev / socp_singular_batch (kernels_svd.hip, built once per flavour like kernels_tangent.hip).  One matrix per team
// of L lanes, a lane per pair of rows; T teams per workgroup; the matrix, its n row norms and kSvdFlags doubles of flags in LDS
constexpr int kSvdLdsBytes = 160 * 1024;             // the LDS of a CU: the most one workgroup can take
constexpr int kSvdFlags = 4;                          // doubles per team behind its row norms: eight int flags
constexpr int kSvdMaxN = 142;                         // the largest n whose matrix (row stride n | 1), norms and flags fit kSvdLdsBytes
inline size_t svd_team_bytes(int n) { return sizeof(double) * ((size_t)n * (n | 1) + n + kSvdFlags); }
inline bool svd_fits(int n) { return n >= 1 && svd_team_bytes(n) <= (size_t)kSvdLdsBytes; }
// L: the power of two that holds the (n + (n & 1)) / 2 pairs of a step (so a lane owns at most two rows in the finish)
inline int svd_lanes(int n)
{
    int L = 1;
    while (L < (n + (n & 1)) / 2) L *= 2;
    return L;
}
// T: the teams that fill a wavefront, halved while they take more than half a CU's LDS (two workgroups then share a CU)
inline int svd_teams(int n)
{
    int T = svd_lanes(n) >= 64 ? 1 : 64 / svd_lanes(n);
    while (T > 1 && T * svd_team_bytes(n) > (size_t)kSvdLdsBytes / 2) T /= 2;
    return T;
}
inline size_t svd_lds_bytes(int n) { return svd_teams(n) * svd_team_bytes(n); }
// A[B][n*n] column-major (left as it was) -> sigma[B][n], sweeps[B], info[B] and, by vt_mode, 0: nothing, 1: Vt[B][n][n], 2: only
// the row of the smallest singular value, Vt[B][n]; hipErrorInvalidValue unless svd_fits(n)
hipError_t svd(hipStream_t st, int B, int n, const double *A, int max_sweeps, int vt_mode, double *sigma, double *Vt, int *sweeps, int *info);
hipError_t svd_fast(hipStream_t st, int B, int n, const double *A, int max_sweeps, int vt_mode, double *sigma, double *Vt, int *sweeps,
                    int *info);
// J[B][n*n] column-major: scale != 0: colnorm[b][j] = the norm of column j (a zero: 1) and the column divided by it, in place;
// scale == 0: colnorm = 1.  colnorm may be null
hipError_t svd_colscale(hipStream_t st, int B, int n, int scale, double *J, double *colnorm);
hipError_t svd_colscale_fast(hipStream_t st, int B, int n, int scale, double *J, double *colnorm);
// socp_group_batch (kernels_group.hip; flavour- and model-independent, built without contraction).  next[max_groups + 1]: the
// "next leader" words -- next[g] is the leader of round g (INT_MAX: no row is left), written by group_begin (g = 0) and by round g - 1
// group_begin: leader / count / radius / summary / next filled, label = MASKED or unassigned (= OVERFLOW), next[0] = the first leader
hipError_t group_begin(hipStream_t st, int B, int n, int ld, const double *V, const int *mask, int max_groups, int *label, int *leader,
                       int *count, double *radius, int *summary, int *next);
// round g: unassigned rows near row next[g] take label g; leader[g], count[g], radius[g], summary[0] = g + 1, next[g + 1].  Returns
// at once on the device when next[g] holds no row
hipError_t group_round(hipStream_t st, int B, int n, int ld, const double *V, double atol, double rtol, int g, int *label, int *leader,
                       int *count, double *radius, int *summary, int *next);
// the numbers of overflow, not-finite and masked rows into summary[1 .. 3]
hipError_t group_end(hipStream_t st, int B, const int *label, int *summary);
// flavour- and model-independent: total[b] = sum of cost[b][0 .. M), left to right
hipError_t cost_total(hipStream_t st, int B, int M, const double *cost, double *total);
// flavour- and model-independent: the unknown vectors Z2[B][n2] of a re-grid's target structure from the moved node states
// Xm[B][M2+1][S] and the target times T2[B][M2+1]; free_bits: bit j of word j / 64 = node j of the target is FREE (M2 <= 255)
hipError_t regrid_pack(hipStream_t st, int B, int S, int M2, int n2, const unsigned long long (&free_bits)[4], const double *Xm,
                       const double *T2, double *Z2);

// socp_fields_batch of the in-tree models (kernels_fields.hip: one object without contraction, for both flavours -- a throughput
// context returns the same bits); Goddard's picks the law per launch like its other entries
hipError_t fields_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                          int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi);
hipError_t fields_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                       int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi);
hipError_t fields_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                        int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi);

// socp_gain_batch of the in-tree models (kernels_gain.hip: one object without contraction, for both flavours)
hipError_t gain_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                        double *Xq, int *count, double *Psi, double *Wq, double *A, double *Kp);
hipError_t gain_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                     double *Xq, int *count, double *Psi, double *Wq, double *A, double *Kp);
hipError_t gain_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                      double *Xq, int *count, double *Psi, double *Wq, double *A, double *Kp);

// socp_gain_free_batch of the in-tree models (kernels_gain_free.hip: one object without contraction, for both flavours)
hipError_t gain_free_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                             double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke);
hipError_t gain_free_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                          double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke);
hipError_t gain_free_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int stride, int cap, double *tq,
                           double *Xq, int *count, double *Psi, double *Len, double *gradH, double *Wq, double *A, double *Ke);

// socp_guide_batch of the in-tree models (kernels_guide.hip: the reference-order models without contraction; kernels_guide_fast.hip:
// the throughput flavour's models with contraction on -- a throughput context flies at throughput speed); Goddard's pick the law per
// launch as its trace entry does.  The double integrator is one struct in both flavours (DIntFast = DIntExact): ONE launcher, guide_dint,
// for both tables
hipError_t guide_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A);
hipError_t guide_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A);
hipError_t guide_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A);
hipError_t guide_goddard_fast(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf,
                              const GuideArgs &A);
hipError_t guide_covid_fast(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int free_tf, const GuideArgs &A);

// socp_exact_jacobian_batch of the in-tree models (kernels_exact_jacobian.hip: one object without contraction, for both flavours)
hipError_t exact_jacobian_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F);
hipError_t exact_jacobian_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F);
hipError_t exact_jacobian_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F);

// socp_fields_batch and socp_exact_jacobian_batch of the vtolUAV model (kernels_vtol_exact.hip: one object without contraction, for
// both flavours; instantiated on VtolExact)
hipError_t fields_vtol(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, int cols, int stride, int skip,
                       int cap, double *tq, double *det, int *count, int *nchange, double *tconj, double *Phi);
hipError_t exact_jacobian_vtol(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, double *Fjac, double *F);

// socp_sensitivity_batch of the in-tree models (kernels_sensitivity.hip: one object without contraction, for both flavours), and its
// model-independent finish: the XNODE directions' -1.0 into G[B][K][n] (kind / index: 2 and 16 bits per direction, the index
// (node << 5) | component), then rhs = -G
hipError_t sensitivity_goddard(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                               double *G);
hipError_t sensitivity_dint(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                            double *G);
hipError_t sensitivity_covid(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int B, const double *Z, const SensDirs &dirs, int K,
                             double *G);
hipError_t sensitivity_finish(hipStream_t st, const ProblemDev &pb, int B, int K, unsigned xnode_mask, const unsigned long long (&index)[4],
                              double *G, double *rhs);

// socp_hamiltonian_gradient_batch of the in-tree models (kernels_hamiltonian.hip: one object without contraction, for both flavours);
// Goddard's picks the law from the context's mu2 like its eval entry
hipError_t hamiltonian_gradient_goddard(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X,
                                        double *G);
hipError_t hamiltonian_gradient_dint(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *G);
hipError_t hamiltonian_gradient_covid(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *G);

// socp_hamiltonian_jacobian_batch of the in-tree models (kernels_hamiltonian_jacobian.hip: one object without contraction, for both
// flavours); Goddard's picks the law from the context's mu2 like its eval entry
hipError_t hamiltonian_jacobian_goddard(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X,
                                        double *A, double *G);
hipError_t hamiltonian_jacobian_dint(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *A,
                                     double *G);
hipError_t hamiltonian_jacobian_covid(hipStream_t st, const ModelParams &P, int B, const double *t, const double *sw, const double *X, double *A,
                                      double *G);

// the in-tree models' tables, one translation unit each
// Goddard, double integrator, covid19 by SOCP_MODEL_* id (builtin_tables.hpp); null for any other id
const ModelLaunchers *builtin_launchers(int model_id);      // kernels_exact.hip            (reference operation order)
const ModelLaunchers *builtin_launchers_fast(int model_id); // kernels_fast.hip             (restructured, contraction on)
const ModelLaunchers *interceptor_launchers();      // kernels_interceptor.hip      (reference operation order)
const ModelLaunchers *interceptor_launchers_fast(); // kernels_interceptor_fast.hip (restructured, contraction on)
const ModelLaunchers *vtol_launchers();             // kernels_vtol.hip             (reference operation order)
const ModelLaunchers *vtol_launchers_fast();        // kernels_vtol_fast.hip        (restructured, contraction on)

}  // namespace socp
