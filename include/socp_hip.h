/*
 * socp_hip.h -- C-ABI of the MI355X (gfx950) hot path of SOCP.
 *
 * Plain C types only (pointers, sizes, int status); no C++ or torch types cross this line.
 * Each entry point names the reference interface it replaces (file:line into bherisse/socp).
 * Host programs reach it either directly (ctypes / dlopen) or through the C++ mirror of the
 * reference's own classes in socp_amd/host/ (model, goddard, doubleIntegrator, shooting).
 *
 * Conventions
 *   - every function returns SOCP_OK (0) or a negative SOCP_ERR_*; socp_last_error() gives text.
 *     No exceptions cross the boundary.  There is NO CPU fallback: without a HIP device
 *     socp_ctx_create fails with SOCP_ERR_NO_DEVICE.
 *   - "_dev" variants take DEVICE pointers and only enqueue work on the context's stream
 *     (inputs already resident in HBM); the plain variants take HOST pointers, copy in,
 *     run, copy out and synchronise.
 *   - all reals are IEEE double (commonType.hpp:16, real = double).
 *   - state vectors are [state(d) ; costate(d)], s = 2d doubles (Appendix B of SURVEY.md);
 *     batches are row-major, one trajectory / unknown vector per row.
 */
#ifndef SOCP_HIP_H_
#define SOCP_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOCP_OK               0
#define SOCP_ERR_ARG         -1   /* bad argument / inconsistent problem description */
#define SOCP_ERR_HIP         -2   /* a HIP runtime call failed */
#define SOCP_ERR_NO_DEVICE   -3   /* no gfx950 device visible: the product does not run on CPU */
#define SOCP_ERR_UNSUPPORTED -4   /* model / mode combination without a device implementation */

/* in-tree device dynamics (twins of src/models/goddard, src/models/doubleIntegrator) */
#define SOCP_MODEL_GODDARD            1   /* dim 7, goddard.cpp:48-295 */
#define SOCP_MODEL_DOUBLE_INTEGRATOR  2   /* dim 6, doubleIntegrator.cpp:49-300 */
#define SOCP_MODEL_COVID19            3   /* dim 4, covid19.cpp:53-165 (control dimension 1) */
#define SOCP_MODEL_INTERCEPTOR        4   /* dim 6, interceptor.cpp:69-998: two charts, two stages, own ComputeTraj and
                                             final rows (control dimension 2: u, beta) */
#define SOCP_MODEL_VTOLUAV            5   /* dim 6, vtolUAV.cpp:58-278 + obstacle.cpp:155-319: the right-hand side reads a
                                             device-resident obstacle table (socp_ctx_set_map); state-only (modelOrder 0).
                                             LANE_EXACT follows the reference's operation order but uses the device library's
                                             tanh: NOT bit-identical to the CPU path (rows 6-8 of the RHS, the Hamiltonian) */

/* packed parameter block, refreshed before every Newton solve (parameters are mutated by the
 * continuation loop through a raw real&, shooting.cpp:695-707) */
#define SOCP_GODDARD_NPARAMS 8   /* C, b, KD, kr, u_max, mu1, mu2, singularControl (goddard.hpp:28-37) */
#define SOCP_DINT_NPARAMS    3   /* u_max, a_max, muT (doubleIntegrator.hpp:24-28) */
#define SOCP_COVID_NPARAMS   8   /* R0, Tinf, Tinc, N, Imax, muI, umin, umax (covid19.hpp parameters_struct) */
/* interceptor.hpp:28-46 in declaration order without the never-read r_2p/t_2p, then data->R_Earth, data->mu0,
 * data->chartLimit (interceptor.cpp:52-58):  c0, hr, d0, eta, propellant_mass, empty_mass, q, ve, alpha_max, u_max,
 * a_max, mu_gft, muT, muV, muC, R_Earth, mu0, chartLimit */
#define SOCP_INTERCEPTOR_NPARAMS 18
/* vtolUAV.hpp parameters_struct in declaration order (nWP_tot, nWP as doubles), then the map's obstacle.hpp
 * parameters_struct: u_max, a_max, alphaT, alphaV, invSigmaXwp, Vd, ca, nWP_tot, nWP, phiObs, psiWP, muObs, sigmaWP.
 * The map's scalars are parameters, not table entries: continuation moves muObs, and chains carry per-problem blocks. */
#define SOCP_VTOL_NPARAMS 13
#define SOCP_MAX_NPARAMS         24   /* capacity of a packed parameter block */
/* obstacle table of SOCP_MODEL_VTOLUAV: SOCP_MAP_STRIDE doubles per obstacle -- type (0 ellipsoid, 1 box, anything else
 * contributes nothing), centre x y z, radii x y z -- at most SOCP_MAX_OBSTACLES rows */
#define SOCP_MAP_STRIDE     7
#define SOCP_MAX_OBSTACLES  256

/* time / state modes, model.hpp:34-38 */
#define SOCP_FIXED      0
#define SOCP_FREE       1
#define SOCP_CONTINUOUS 2

/* kernel variants behind one call */
#define SOCP_VARIANT_AUTO       0   /* default: the reference-order kernels (= LANE_EXACT), the flavour every parity claim is
                                       made on; the environment variable SOCP_VARIANT=fast|exact changes the default */
#define SOCP_VARIANT_LANE_EXACT 1   /* one trajectory per lane, reference operation order, no FMA contraction: bit-identical
                                       to the CPU path for goddard / doubleIntegrator / covid19 */
#define SOCP_VARIANT_LANE_FAST  2   /* one trajectory per lane, reciprocal/FMA-restructured arithmetic (<= 1e-8 after 1e4 steps) */
/* There is no selectable one-trajectory-per-wavefront variant for the state-only path (north_star sketches one): a wave
 * instruction costs the same issue slots with 1 or 64 active lanes (scripts/probes/probe_lanes.hip), and spreading ONE
 * Goddard trajectory over lanes does not shorten its instruction stream (DESIGN.md section 3 has the count), so it would be
 * the same latency at 1/16 of the throughput.  The variational (is_jac = 1) integration, 156 values per trajectory, IS one
 * wavefront per trajectory with its stage vectors in LDS -- always, not as a variant. */

/* what socp_eval_batch computes */
#define SOCP_EVAL_RHS         0   /* odeTools.hpp:82  Model(t, X, isJac)      -> len(X) values  */
#define SOCP_EVAL_CONTROL     1   /* model.hpp:375    Control(t, X)           -> control dim (3, 3, 1) */
#define SOCP_EVAL_HAMILTONIAN 2   /* model.hpp:384    Hamiltonian(t, X, 0)    -> 1 value        */

typedef struct socp_ctx socp_ctx;

/* ---- context ---------------------------------------------------------------------------- */
/* replaces: construction of a model object + its parameters (goddard.cpp:23-40,
 * doubleIntegrator.cpp:26-34).  device < 0 selects the current HIP device. */
int socp_ctx_create(socp_ctx **ctx, int model_id, int device);
int socp_ctx_destroy(socp_ctx *ctx);
const char *socp_last_error(const socp_ctx *ctx);   /* ctx may be NULL: last creation error */

int socp_ctx_set_params(socp_ctx *ctx, const double *params, int nparams);
int socp_ctx_get_params(const socp_ctx *ctx, double *params, int nparams);
int socp_ctx_num_params(const socp_ctx *ctx);        /* length of the model's packed parameter block (< 0: error) */
int socp_ctx_set_step_number(socp_ctx *ctx, int step_nbr);      /* model::stepNbr, model.hpp:367 */
/* replaces: the obstacle arrays an `obstacle` map reads from its file (obstacle.cpp:69-109) and every later
 * map::Gradient / map::Function call of the model (vtolUAV.cpp:84-90, :172-177).  table[n_obs][SOCP_MAP_STRIDE] is copied to a
 * device buffer the context owns; every kernel of the model reads it from there.  n_obs = 0 is free space; more than
 * SOCP_MAX_OBSTACLES is SOCP_ERR_ARG (the context keeps its previous table); a context of another model: SOCP_ERR_UNSUPPORTED.
 * A fresh context has no obstacles.  socp_ctx_clone copies the table to the clone's device. */
int socp_ctx_set_map(socp_ctx *ctx, int n_obs, const double *table);
/* *n_obs = rows in force; table (may be NULL) receives them, read back from the device; cap_obs = rows `table` can hold */
int socp_ctx_get_map(const socp_ctx *ctx, int *n_obs, double *table, int cap_obs);
/* integrator of every later call: SOCP_INT_RK4 = the reference's default fixed-step loop
 * (odeTools.cpp:135-145); SOCP_INT_DOPRI5 = what it runs when built with -D_USE_BOOST (odeTools.cpp:129-134),
 * abs = rel tolerance `tol` = odeTools::odeIntTol (set from the solver's xtol by shooting::SetPrecision,
 * shooting.cpp:447-450); initial step (tf - t0)/stepNbr.  Per-lane step control; reference-order RHS. */
#define SOCP_INT_RK4    0
#define SOCP_INT_DOPRI5 1
int socp_ctx_set_integrator(socp_ctx *ctx, int kind, double tol);
/* the step number, integrator and tolerance in force (any pointer may be NULL): what sizes the rows of a trace */
int socp_ctx_get_integrator(const socp_ctx *ctx, int *step_nbr, int *kind, double *tol);
int socp_ctx_set_switching_times(socp_ctx *ctx, const double *sw, int nsw);  /* goddard.cpp:373-377 */
int socp_ctx_get_switching_times(const socp_ctx *ctx, double *sw2);          /* the two values the control law reads */
int socp_ctx_set_variant(socp_ctx *ctx, int variant);
/* vtolUAV's entries of the exact-derivative stack (socp_fields_batch, socp_exact_jacobian_batch, socp_newton_batch with jac = 2) are
 * switched per context and are OFF in a new one: until socp_ctx_set_exact_hooks(ctx, 1) the context answers as it did before the model
 * had them -- socp_ctx_has_fields and socp_ctx_has_exact_jacobian 0, the calls SOCP_ERR_UNSUPPORTED ("no fields entry", "no
 * exact_jacobian entry").  on = 0 switches them off again; socp_ctx_clone copies the setting.  SOCP_ERR_UNSUPPORTED for any other
 * model: theirs are not switched. */
int socp_ctx_set_exact_hooks(socp_ctx *ctx, int on);
int socp_ctx_get_variant(const socp_ctx *ctx);      /* SOCP_VARIANT_* as set (AUTO = reference order) */
/* enqueue on the caller's hipStream_t (NULL is the device's default stream); use_own != 0 switches
 * back to the context's private non-blocking stream */
int socp_ctx_set_stream(socp_ctx *ctx, void *hip_stream, int use_own);
/* the stream launches currently go to (the context's own stream or the one given to socp_ctx_set_stream) */
int socp_ctx_get_stream(const socp_ctx *ctx, void **hip_stream);
/* a second stream owned by the context (non-blocking, highest priority where the device has priorities: its own hardware
 * queue, so that work on it overlaps work on the context's stream).  Created on the first call -- that takes ~6 ms, which is
 * why the lock-step engines keep it instead of creating one per call -- and destroyed with the context.  Nothing is ever
 * enqueued on it by the context itself: the engines (socp_chains_solve, socp_multistart_solve) use it while they run. */
int socp_ctx_aux_stream(socp_ctx *ctx, void **hip_stream);
/* Pay now what a process otherwise pays inside its first large call: the context's second stream (above) and the start-up of the
 * copy engines -- the first copy of more than 16 KB between pinned host memory and the device takes ~8 ms, once per process
 * (measured: scripts/probes/first_copy.hip).  Optional; for callers whose first solve is latency-critical. */
int socp_ctx_warm_up(socp_ctx *ctx);
int socp_ctx_synchronize(socp_ctx *ctx);
int socp_ctx_dims(const socp_ctx *ctx, int *dim, int *state_len, int *state_len_jac);
int socp_ctx_control_dim(const socp_ctx *ctx);
int socp_ctx_device(const socp_ctx *ctx);            /* HIP device index the context lives on (< 0: error) */
int socp_ctx_model_id(const socp_ctx *ctx);          /* SOCP_MODEL_* / plugin id the context was created with */
/* 1 when the model integrates its variational equations on the device (modelOrder 1: is_jac = 1 trajectories,
 * socp_var_jacobian, hybrj chains) -- the in-tree double integrator, or a plugin with the aug_rhs / dhamiltonian trait
 * (socp_amd/csrc/plugin_impl.hpp); 0 otherwise (model.hpp:104-120,149-183 need Model(t, X, 1) and Hamiltonian(t, X, 1)) */
int socp_ctx_has_variational(const socp_ctx *ctx);

/* counters since creation: trajectories integrated, kernel launches */
int socp_ctx_counters(const socp_ctx *ctx, long long *trajectories, long long *launches);
/* adds to them: what a clone of `ctx` (socp_ctx_clone) integrated on its behalf -- the second group of chains of a large
 * socp_chains_solve call runs on one -- counts as ctx's */
void socp_ctx_add_counters(socp_ctx *ctx, long long trajectories, long long launches);

/* ---- batched trajectory integration ------------------------------------------------------ */
/* replaces: shooting::Move -> model::ComputeTraj -> ModelInt -> odeTools::integrate -> RK4
 * (shooting.cpp:365-372, model.hpp:77-79,395-414, goddard.cpp:298-317, odeTools.cpp:89-98,128-146),
 * once per row.  t0,tf: [B]; sw: NULL (use the context's switching times) or [B][2];
 * X0,Xf: [B][len], len = s (is_jac = 0) or (s+1)*s (is_jac = 1, variational state, identity
 * block supplied by the caller exactly as shooting.cpp:1003-1005 builds it).  Xf may alias X0. */
int socp_integrate_batch(socp_ctx *ctx, int B, const double *t0, const double *tf,
                         const double *sw, const double *X0, double *Xf, int is_jac);
int socp_integrate_batch_dev(socp_ctx *ctx, int B, const double *d_t0, const double *d_tf,
                             const double *d_sw, const double *d_X0, double *d_Xf, int is_jac);

/* replaces: the observer form of odeTools::integrate (odeTools.cpp:103-123) used by the trace replay
 * (shooting.cpp:496-544, model.hpp:401-407): one trajectory, the state after every step kept.
 * dense: [cap][len], times: [cap]; row 0 = (t0, X0), row k = accumulated time and state after k
 * steps; *rows = steps + 1 (rows beyond cap are counted, not stored).  sw: NULL or 2 values.
 * Under SOCP_INT_DOPRI5 (the reference built with -D_USE_BOOST: odeTools.cpp:108, integrate_adaptive with the observer) the rows
 * are the adaptive integrator's own accepted steps -- their number is only known afterwards: call again with cap >= *rows
 * when *rows > cap. */
int socp_integrate_dense(socp_ctx *ctx, double t0, double tf, const double *sw, const double *X0,
                         double *dense, double *times, int cap, int *rows);
/* Same, also returning each row's two per-trajectory auxiliary scalars in aux[cap][2] (NULL: not wanted).  They
 * are the Goddard switching times (constant) or, for the interceptor, (stageMode, currentChart) -- what
 * interceptor::Trace prints beside the state (interceptor.cpp:131-151).  A model with its own ComputeTraj
 * (interceptor.cpp:162-218) reports the rows that function traces -- the start of each stage and every step --
 * followed by ONE extra row: the state ComputeTraj returns (chart 1) with the flags it leaves behind. */
int socp_integrate_dense_aux(socp_ctx *ctx, double t0, double tf, const double *sw, const double *X0,
                             double *dense, double *times, double *aux, int cap, int *rows);

/* replaces: model::Model / Control / Hamiltonian called outside the integrator (trace,
 * free-time rows).  t: [B]; X: [B][len]; out: [B][out_len]. */
int socp_eval_batch(socp_ctx *ctx, int what, int B, const double *t, const double *sw,
                    const double *X, int len, double *out, int is_jac);

/* ---- shooting problem --------------------------------------------------------------------- */
/* replaces: the part of shooting::data_struct the residual reads (shooting.cpp:21-35):
 * numMulti M, mode_t[M+1], mode_X[M+1][d], current node times time[M+1] and node states
 * X[M+1][2d] (only the first d of each row is read).  Must be re-sent when the continuation
 * loop blends the boundary data (shooting.cpp:609-611). */
int socp_problem_set(socp_ctx *ctx, int num_multi, const int *mode_t, const int *mode_x,
                     const double *time, const double *xnode);
int socp_problem_num_param(const socp_ctx *ctx);   /* n = 2 d M + #FREE times (shooting.cpp:179,196) */
int socp_problem_num_nodes(const socp_ctx *ctx);   /* M + 1 of the problem set (< 0: none) */

/* Per-problem blocks for the batch entry points below (batched continuation chains: shooting.cpp:598-692 blends the
 * boundary data of ONE problem per Newton solve, :695-778 moves ONE model parameter through a real&; with many chains in
 * one launch every row needs its own).  Device pointers, or NULL for "shared" (the context's parameters / the tables of
 * socp_problem_set); they stay in force for every later *_dev batch call until replaced:
 *   d_params[q][stride]   stride = nparams + 2: the packed parameters of problem q, then its two default switching times
 *   d_time[q][M+1], d_xnode[q][(M+1)*2d]   current node times / node states of problem q (what socp_problem_set takes)
 * Row q of socp_residual_batch_dev, problem q of socp_fd_jacobian_multi_dev / socp_fd_rows_dev read block q.  Modes, M and n
 * are those of socp_problem_set.  With d_params the Goddard control law is chosen per problem from its own mu2. */
int socp_problem_set_blocks_dev(socp_ctx *ctx, const double *d_params, int stride, const double *d_time,
                                const double *d_xnode);
/* Goddard with d_params: a promise that EVERY parameter block has mu2 > 0 (the smooth control law of goddard.cpp:137-145), which
 * lets the batch launches take the kernel specialised on that law (three waves per SIMD instead of two; with shared parameters
 * the library sees mu2 itself).  Stays in force until socp_problem_set or a call with all_smooth = 0.  A wrong promise computes
 * the smooth law for blocks that asked for the bang / singular / off law. */
int socp_problem_blocks_all_smooth(socp_ctx *ctx, int all_smooth);
/* host-pointer form of socp_residual_batch with per-row blocks (any of params / time / xnode may be NULL) */
int socp_residual_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int stride,
                               const double *time, const double *xnode, double *F);

/* replaces: shooting::ComputeTimeLine (shooting.cpp:1579-1617) for one unknown vector */
int socp_timeline(socp_ctx *ctx, const double *z, double *timeline);

/* replaces: shooting::StaticShootingFunction -> ShootingFunction[Parallel]
 * (shooting.cpp:859-874,918-993,1133-1158,1215-1307), for B unknown vectors at once:
 * Z[B][n] -> F[B][n].  One trajectory per (row, segment); every trajectory writes its own
 * residual slots, as the reference's threads do. */
int socp_residual_batch(socp_ctx *ctx, int B, const double *Z, double *F);
int socp_residual_batch_dev(socp_ctx *ctx, int B, const double *d_Z, double *d_F);

/* replaces: MINPACK fdjac1 as hybrd drives it (call site shooting.cpp:803-826):
 * J[:,j] = (F(z + h_j e_j) - fvec) / h_j, h_j = sqrt(max(epsfcn, eps_mach)) * |z_j| (or that
 * factor itself when z_j == 0).  fjac is column-major with leading dimension n.  The n
 * perturbed residuals are one batch.  dedup != 0 integrates only the segments a column can
 * change (bit-identical result, fewer trajectories; SURVEY 7 "free win"). */
int socp_fd_jacobian(socp_ctx *ctx, const double *z, const double *fvec, double epsfcn,
                     double *fjac, int dedup);
int socp_fd_jacobian_dev(socp_ctx *ctx, const double *d_z, const double *d_fvec, double epsfcn,
                         double *d_fjac, int dedup);

/* The same for `np` independent unknown vectors of ONE problem structure (multi-start /
 * continuation sweeps): Z[np][n], Fvec[np][n] -> Fjac[np][n*n]; one launch. */
int socp_fd_jacobian_multi_dev(socp_ctx *ctx, int np, const double *d_Z, const double *d_Fvec,
                               double epsfcn, double *d_Fjac, int dedup);

/* The (n+1) residual rows of a forward-difference Jacobian in ONE launch: Rows[np][n+1][n], row 0
 * = F(z), row j+1 = F(z + h_j e_j); base and perturbed trajectories are independent, so nothing
 * waits on the base evaluation.  This is "one Newton step's batch": (n+1)*M trajectories per
 * problem (15 rows).  socp_fd_diff_dev turns rows into the Jacobian. */
int socp_fd_rows_dev(socp_ctx *ctx, int np, const double *d_Z, double epsfcn, double *d_Rows);
int socp_fd_rows(socp_ctx *ctx, int np, const double *Z, double epsfcn, double *Rows);
int socp_fd_diff_dev(socp_ctx *ctx, int np, const double *d_Z, double epsfcn, const double *d_Rows,
                     double *d_Fjac);

/* replaces: shooting::Trace (shooting.cpp:496-544; model.hpp:422-462) for a whole batch of unknown vectors: the sampled rows
 * t, X, u, H of every segment, device-resident.
 * width of a trace row of this context's model: W = 1 + 2d + NU + 1 + 2  (t, X[2d], u[NU], H, aux0, aux1) */
int socp_trace_width(const socp_ctx *ctx);
/* Z[B][n] -> rows[B][M][cap][W], count[B][M].  Segment i of row b is integrated exactly as the residual integrates it
 * (same timeline, switching times, start state z[s i .. s i + s), integrator, per-problem blocks of
 * socp_problem_set_blocks_dev: row b reads block b).  Let R be the number of rows socp_integrate_dense_aux reports for
 * that segment and k = 0 .. R-1 their indices: row k is KEPT iff k % stride == 0 or k == R-1.  Kept rows are stored in
 * order; count[b][i] = number of kept rows (kept rows beyond cap are counted, not stored, nothing is written past
 * slab [b][i]; rows at or beyond min(count, cap) keep what the buffer held).  stride >= 1, cap >= 1.
 * t, X, aux0, aux1 of a row are what socp_integrate_dense_aux gives for (t1, t2, switching times, X_start) of the segment
 * (a model with its own ComputeTraj: its traced rows and the extra final row, which is row R-1; a zero-length or backward
 * segment: R = 1); u and H are what socp_eval_batch(SOCP_EVAL_CONTROL / SOCP_EVAL_HAMILTONIAN) returns at the row's (t, X)
 * with the row's aux pair as sw.  The variational state is not traced (neither does the reference: odeTools.cpp:242).
 * Under SOCP_INT_DOPRI5 a trajectory whose integration fails (NaN result) shows the NaN state in its last row unless the
 * stride kept the last accepted step.
 * SOCP_ERR_ARG: stride < 1, cap < 1, B < 0, no problem set; B == 0: SOCP_OK without a launch; a model whose launch table
 * has no trace entry: SOCP_ERR_UNSUPPORTED.  Two launches (integration; u and H of the stored rows); socp_ctx_counters
 * advances by B M trajectories.  The _dev form takes device pointers, enqueues on the context's stream and neither copies nor
 * synchronises; the host form stages through that stream (rows travels both ways).  When count exceeds cap, call again
 * with cap >= the largest count. */
int socp_trace_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int stride, int cap, double *d_rows, int *d_count);
int socp_trace_batch(socp_ctx *ctx, int B, const double *Z, int stride, int cap, double *rows, int *count);
/* host-pointer form with per-row blocks, like socp_residual_batch_blocks (any of params / time / xnode may be NULL) */
int socp_trace_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                            const double *time, const double *xnode, int stride, int cap, double *rows, int *count);

/* Integrated running cost of a whole batch of unknown vectors: what ranks the extremals a multi-start sweep ends in.  [ext] The
 * reference never computes it.  Every in-tree Hamiltonian (and the example plugin's) has the form H = L + <p, f_x>, so the running
 * cost is L(t, X) = H(t, X) - sum_k p_k f_k(t, X), from the model's Hamiltonian and right-hand side; the sum runs over the d
 * state components, left to right.  H - p.f carries an absolute rounding error of the order of eps |p.f| per evaluation.
 * Z[B][n] -> cost[B][M]: segment i of row b is integrated exactly as the residual integrates it (same timeline, switching times,
 * start state z[s i .. s i + s), per-problem blocks of socp_problem_set_blocks_dev: row b reads block b) with the fixed-step RK4
 * steps of the residual, and q' = L is carried through those steps as a quadrature variable: q = 0.0 at the segment's start,
 * q <- q + (step/6)(L1 + (L4 + 2 (L2 + L3))) with L1..L4 at the four stage points (t, X) of the step; cost[b][i] = q at the
 * segment's end.  A zero-length or backward segment takes no step: cost = 0.0 (+0.0) and Xend = the start state.
 * total[b] (may be NULL) = cost[b][0] + cost[b][1] + ... + cost[b][M-1], summed in that order; Xend[b][i][s] (may be NULL) = the
 * state at the end of segment i, what socp_integrate_batch gives for the segment.  Terminal cost terms are not included.
 * socp_ctx_has_cost: 1 when the context's model has a cost kernel, 0 when not (a model with its own ComputeTraj -- the
 * interceptor: its chart changes rewrite the costate in mid-trajectory).
 * SOCP_ERR_ARG: no problem set, B < 0, B > 0 with Z or cost NULL, _blocks with params and param_stride != nparams + 2;
 * B == 0: SOCP_OK without a launch; SOCP_ERR_UNSUPPORTED: the context's integrator is SOCP_INT_DOPRI5 (the message says so), or
 * the model's launch table has no cost entry.  An error leaves the context unchanged.
 * One launch, one more with total; socp_ctx_counters advances by B M trajectories.  The _dev form takes device pointers,
 * enqueues on the context's stream and neither copies nor synchronises; the host forms stage through that stream and return
 * when the results are in the caller's arrays.  _blocks: per-row blocks like socp_residual_batch_blocks (any of params / time /
 * xnode may be NULL); the context's own blocks are restored afterwards. */
int socp_ctx_has_cost(const socp_ctx *ctx);   /* 1 / 0 */
int socp_cost_batch_dev(socp_ctx *ctx, int B, const double *d_Z, double *d_cost, double *d_total, double *d_Xend);
int socp_cost_batch(socp_ctx *ctx, int B, const double *Z, double *cost, double *total, double *Xend);
int socp_cost_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                           const double *time, const double *xnode, double *cost, double *total, double *Xend);

/* Control-structure events of a whole batch of unknown vectors: on which arcs the control of an extremal is saturated, interior or
 * off, and when it changes branch.  [ext] The reference reads this off a plot (testGoddard.cpp:117-118: "estimated from observation
 * of the previous solution").  A model offers event CHANNELS, scalars of (t, X) -- typically the switching function of its control
 * law; the caller gives E watches (chan[e], level[b][e]) and gets every crossing of channel chan[e] through that level:
 *   goddard            1 channel:  Switch = mu1 - b p_mass - C / mass |p_v|  (goddard.cpp:135), for every mu2; with mu2 > 0 the thrust
 *                                  is on below 0 and saturated below -2 mu2 u_max
 *   doubleIntegrator   1 channel:  the norm of the unsaturated control -p_v / a_max (doubleIntegrator.cpp:218-259); saturated above u_max
 *   covid19            2 channels: 0 the unclamped control (covid19.cpp:97-126; levels umin, umax), 1 the state I = X[2] (level Imax:
 *                                  the contact times of the penalised state constraint)
 *   interceptor, vtolUAV, a plugin without the trait (include/socp_plugin.h): none
 * Z[B][n], chan[E] (HOST array, read before the call returns: the channels travel as a kernel argument), levels[B][E] ->
 * tev[B][M][cap], id[B][M][cap], count[B][M], Xev[B][M][cap][s] (may be NULL).  Segment i of row b is integrated exactly as the
 * residual integrates it (same timeline, switching times, start state z[s i .. s i + s), fixed RK4 steps, per-problem blocks of
 * socp_problem_set_blocks_dev: row b reads block b).  With g the channel values at the two ends of a step that starts at the
 * accumulated time tk from the state Xk and has the length `step` (the clamped last step included), neg(v) = (v < 0.0):
 *   a0 = g(tk, Xk) - level, a1 = g(tk + step, X) - level;   an event iff neither is NaN and neg(a0) != neg(a1)
 *   a = 0.0, c = step, ga = a0, gc = a1
 *   `refine` times:  th = a + (c - a) * (ga / (ga - gc));  Y = one RK4 step of length th from (tk, Xk);  gt = g(tk + th, Y) - level
 *                    neg(gt) == neg(ga) ? (a = th, ga = gt) : (c = th, gc = gt)
 *   th = a + (c - a) * (ga / (ga - gc));  tev = tk + th;  id = neg(a0) ? +(e + 1) : -(e + 1)     (rising / falling through the level)
 *   Xev = one RK4 step of length th from (tk, Xk)
 * in this operation order (refine = 0: linear interpolation over the step).  The events of a segment are stored in (step, e) order;
 * count[b][i] = their number (events beyond cap are counted, not stored, nothing is written past slab [b][i]; rows at or beyond
 * min(count, cap) keep what the buffer held).  A zero-length or backward segment takes no step: count 0.
 * NOT SEEN: a crossing that falls in the gap between a segment's end state and the next node's unknowns (an unconverged row), and
 * a level touched without a sign change at the ends of a step.
 * The times are a measuring instrument for structure and a source of candidate node times for socp_regrid_batch; a stage started
 * from them need not converge to the root a hand-picked structure converges to.
 * socp_ctx_event_channels: the number of channels of the context's model, 0 when it has none.
 * SOCP_ERR_ARG: no problem set, B < 0, E outside 1 .. 8, refine outside 0 .. 8, cap < 1, a channel outside 0 .. channels-1, a NULL
 * required pointer (chan; with B > 0: Z, levels, tev, id, count), _blocks with params and param_stride != nparams + 2; B == 0: SOCP_OK
 * without a launch; SOCP_ERR_UNSUPPORTED (the message says which): the context's integrator is SOCP_INT_DOPRI5, or the model's launch
 * table has no events entry.  An error leaves the context unchanged.
 * One launch; socp_ctx_counters advances by B M trajectories.  The _dev form takes device pointers (chan stays a host array),
 * enqueues on the context's stream and neither copies nor synchronises; the host forms stage through that stream (tev, id and Xev
 * travel both ways) and return when the results are in the caller's arrays.  _blocks: per-row blocks like
 * socp_residual_batch_blocks (any of params / time / xnode may be NULL); the context's own blocks are restored afterwards.  When a
 * count exceeds cap, call again with cap >= the largest count. */
int socp_ctx_event_channels(const socp_ctx *ctx);      /* number of channels; 0: the model has none */
int socp_events_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int E, const int *chan, const double *d_levels,
                          int refine, int cap, double *d_tev, int *d_id, int *d_count, double *d_Xev);
int socp_events_batch(socp_ctx *ctx, int B, const double *Z, int E, const int *chan, const double *levels,
                      int refine, int cap, double *tev, int *id, int *count, double *Xev);
int socp_events_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                             const double *xnode, int E, const int *chan, const double *levels, int refine, int cap, double *tev,
                             int *id, int *count, double *Xev);

/* Per-segment extrema along a whole batch of unknown vectors: how constant the Hamiltonian is, how large states and controls get,
 * how close the switching function comes to a switch -- without the rows of a trace ever being stored.  [ext] The reference
 * plots its trace files.
 * Z[B][n] -> vmin, vmax, tmin, tmax [B][M][C], count[B][M], nbad[B][M];  tmin, tmax and nbad may be NULL.
 * CHANNELS, in this order (C = socp_extrema_width = 2d + NU + 1 + EC):  X[0 .. 2d), u[0 .. NU), H, g[0 .. EC) -- g the model's event
 * channels, the channels of socp_events_batch, EC = socp_ctx_event_channels (0 when the model has none).
 * WHAT.  The state channels are always reduced; SOCP_EXTREMA_CONTROL, SOCP_EXTREMA_HAMILTONIAN and SOCP_EXTREMA_EVENTS select u, H
 * and g.  Columns of a group that is not selected keep what the buffer held; the events bit on a model with EC = 0 selects nothing.
 * ROWS.  Segment i of row b is integrated exactly as socp_trace_batch integrates it (same timeline, switching times, start state
 * z[s i .. s i + s), integrator -- the fixed-step RK4 loop or the adaptive Dormand-Prince one --, per-problem blocks of
 * socp_problem_set_blocks_dev: row b reads block b), and the rows k = 0 .. R-1 reduced are exactly the rows socp_trace_batch keeps
 * with stride = 1: t, X and the aux pair of row k.  count[b][i] = R.  A model with its own ComputeTraj (the interceptor) reports its
 * traced rows and the extra final row, each in the RAW coordinates of the chart the row is in: an extremum of such a state channel
 * mixes charts, as the trace's column does.  A zero-length or backward segment has R = 1.
 * VALUES.  u and H of a row are what socp_eval_batch(SOCP_EVAL_CONTROL / SOCP_EVAL_HAMILTONIAN) returns at the row's (t, X) with the
 * row's aux pair as sw; g_c = event_fn(P, aux0, aux1, t, X, c), the channel value socp_events_batch watches.
 * REDUCTION, per selected channel, sequential in row order, v the channel's value and t the time of the row:
 *   row 0:            vmin = vmax = v;  tmin = tmax = t
 *   every later row:  if (v < vmin) { vmin = v; tmin = t; }   if (v > vmax) { vmax = v; tmax = t; }
 * The comparisons are strict, so: the FIRST attainment of an extremum wins; -0.0 never displaces +0.0 (nor +0.0 -0.0); a NaN never
 * displaces anything, and a NaN in row 0 stays (no later row compares below or above it).
 * nbad[b][i] = the number of rows in which at least one selected channel is not finite (the state is always selected).
 * The result is over the ROWS, like the trace: an extremum inside a step is not interpolated.
 * SOCP_ERR_ARG: no problem set, B < 0, what outside 0 .. 7, B > 0 with Z, vmin, vmax or count NULL, _blocks with params and
 * param_stride != nparams + 2; B == 0: SOCP_OK without a launch; SOCP_ERR_UNSUPPORTED: the model's launch table has no extrema
 * entry (socp_ctx_has_extrema says 0).  An error writes nothing and leaves the context unchanged.
 * One launch, which writes nothing but these arrays; socp_ctx_counters advances by B M trajectories and one launch.  The _dev form
 * takes device pointers, enqueues on the context's stream and neither copies nor synchronises; the host forms stage through that
 * stream (vmin, vmax, tmin and tmax travel both ways) and return when the results are in the caller's arrays.  _blocks: per-row
 * blocks like socp_trace_batch_blocks (any of params / time / xnode may be NULL); the context's own blocks are restored afterwards. */
#define SOCP_EXTREMA_CONTROL      1
#define SOCP_EXTREMA_HAMILTONIAN  2
#define SOCP_EXTREMA_EVENTS       4
int socp_extrema_width(const socp_ctx *ctx);                 /* C = 2d + NU + 1 + EC  (< 0: error) */
int socp_ctx_has_extrema(const socp_ctx *ctx);               /* 1 / 0 */
int socp_extrema_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int what,
                           double *d_vmin, double *d_vmax, double *d_tmin, double *d_tmax, int *d_count, int *d_nbad);
int socp_extrema_batch(socp_ctx *ctx, int B, const double *Z, int what,
                       double *vmin, double *vmax, double *tmin, double *tmax, int *count, int *nbad);
int socp_extrema_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                              const double *time, const double *xnode, int what,
                              double *vmin, double *vmax, double *tmin, double *tmax, int *count, int *nbad);

/* Model-defined observables along a whole batch of unknown vectors: peak drag and when, burnt fuel, the clearance of an obstacle map,
 * total intervention -- quantities that are neither a state, a control nor H -- reduced to their extrema and their integrals without
 * the rows of a trace ever being stored.  [ext] The reference plots its trace files.
 * Z[B][n] -> ymin, ymax, tmin, tmax, integral [B][M][NO], count[B][M], nbad[B][M];  tmin, tmax, integral and nbad may be NULL.
 * NO = socp_ctx_observables, the names socp_ctx_observable_name(ctx, k), k = 0 .. NO-1 (NULL outside).
 * ROWS.  Exactly those of socp_extrema_batch, that is the rows socp_trace_batch keeps with stride = 1 (same timeline, switching times,
 * start state, per-problem blocks, integrator -- the fixed-step RK4 loop or the adaptive Dormand-Prince one): t, X and the aux pair of
 * row k = 0 .. R-1;  count[b][i] = R.  A zero-length or backward segment has R = 1.
 * VALUES.  y[0 .. NO) = the model's observe(P, aux0, aux1, t, X, u) with u what socp_eval_batch(SOCP_EVAL_CONTROL) returns at the row's
 * (t, X) with the row's aux pair as sw, evaluated once per row.
 * REDUCTION, per observable, sequential in row order, y the value and t the time of row k:
 *   row 0:            ymin = ymax = y;  tmin = tmax = t;  I = +0.0
 *   every later row:  if (y < ymin) { ymin = y; tmin = t; }   if (y > ymax) { ymax = y; tmax = t; }
 *                     w = t_k - t_{k-1};  s = y_k + y_{k-1};  I = I + (0.5 w) s
 * The comparisons are strict, as in socp_extrema_batch: the FIRST attainment wins; -0.0 never displaces +0.0; a NaN never displaces
 * anything and a NaN in row 0 stays.  The integral is the composite trapezoid on the rows: 0.5 w is exact, every other operation
 * rounds once (the throughput flavour may contract the last two); a value that is not finite ENTERS the sum -- the integral is then
 * not finite, and nbad says so; a segment with one row has I = +0.0.  nbad[b][i] = the number of rows in which some observable is
 * not finite.  An extremum inside a step is not interpolated.
 * THE IN-TREE OBSERVABLES.  Plain IEEE operations, each rounding once, in the order written, products and sums left to right; sqrt
 * and / correctly rounded; exp is exp_glibc.  X, u as above, p the packed parameters.
 *   Goddard (both laws), NO = 6:
 *     r         = sqrt(X0 X0 + X1 X1 + X2 X2)                 v = sqrt(X3 X3 + X4 X4 + X5 X5)          (the model's own r and v)
 *     norm_u    = sqrt(u0 u0 + u1 u1 + u2 u2)
 *     drag      = KD v v E,   E = exp(-kr (r - 1))            (the density factor as the right-hand side forms it)
 *     drag_acc  = drag / X6
 *     fuel_rate = b norm_u                                    (its integral is the burnt mass: row 6 of the right-hand side)
 *   vtolUAV, NO = 3:
 *     speed     = sqrt(X3 X3 + X4 X4 + X5 X5)                 norm_u as above
 *     clearance = the smallest level of any obstacle of the context's map (socp_ctx_set_map), negative inside one:
 *       cl = +inf;  for each obstacle in table order:  level -> if (level < cl) cl = level;
 *       box (type 1):        m = |X0 - x| - radx;  b = |X1 - y| - rady;  c = |X2 - z| - radz;  if (b > m) m = b;  if (c > m) m = c;  level = m
 *       ellipsoid (type 0):  hx = X0 - x, hy = X1 - y, hz = X2 - z;  d = sqrt(hx hx + hy hy + hz hz);
 *                            level = d - d / sqrt(hx hx / radx / radx + hy hy / rady / rady + hz hz / radz / radz)
 *     (the three-term radius of the map's value, not the two-term one of its gradient).  A NaN level -- the centre of an ellipsoid --
 *     never displaces anything; an empty map gives +inf (which is not finite: every row then counts in nbad); any other type is skipped.  Never contracted: both flavours give the same bits.
 *   doubleIntegrator, NO = 1:  norm_u.        covid19, NO = 1:  u = u0  (its integral is the total intervention).
 * The throughput flavour evaluates the same texts with contraction on (clearance excepted).
 * SOCP_ERR_ARG: no problem set, B < 0, B > 0 with Z, ymin, ymax or count NULL, _blocks with params and param_stride != nparams + 2;
 * B == 0: SOCP_OK without a launch; SOCP_ERR_UNSUPPORTED ("no observe entry"): the model's launch table has no observe entry
 * (socp_ctx_has_observe says 0): a model without the trait, or with its own ComputeTraj (the interceptor).  An error writes nothing
 * and leaves the context unchanged.
 * One launch, which writes nothing but these arrays; socp_ctx_counters advances by B M trajectories and one launch.  The _dev form
 * takes device pointers, enqueues on the context's stream and neither copies nor synchronises; the host forms stage through that
 * stream and return when the results are in the caller's arrays.  _blocks: per-row blocks like socp_extrema_batch_blocks (any of
 * params / time / xnode may be NULL); the context's own blocks are restored afterwards. */
int socp_ctx_has_observe(const socp_ctx *ctx);               /* 1 / 0 */
int socp_ctx_observables(const socp_ctx *ctx);               /* NO; 0: no observe entry  (< 0: error) */
const char *socp_ctx_observable_name(const socp_ctx *ctx, int k);
int socp_observe_batch_dev(socp_ctx *ctx, int B, const double *d_Z, double *d_ymin, double *d_ymax, double *d_tmin, double *d_tmax,
                           double *d_integral, int *d_count, int *d_nbad);
int socp_observe_batch(socp_ctx *ctx, int B, const double *Z, double *ymin, double *ymax, double *tmin, double *tmax,
                       double *integral, int *count, int *nbad);
int socp_observe_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                              const double *time, const double *xnode, double *ymin, double *ymax, double *tmin, double *tmax,
                              double *integral, int *count, int *nbad);

/* Conjugate-time test of a whole batch of unknown vectors: the Jacobi fields along every extremal.  [ext] The reference never
 * computes this; indirect shooting finds extremals, not minima, and the standard instrument for telling them apart (cotcot, HamPath)
 * is J(t) = dx(t)/dp(t0), a d x d matrix with J(t0) = 0: the first time det J(t) changes sign is the first conjugate time, and a
 * fixed-endpoint extremal stops being locally optimal beyond it.
 * Z[B][n] -> tq[B][M][cap], det[B][M][cap], count[B][M], nchange[B][M], tconj[B][M], Jend[B][M][d][d] (may be NULL).
 * SETUP.  For row b and segment i: the start state X0 = z[s i .. s i + s) = [x (d) ; p (d)]; timeline, switching times and
 * per-problem blocks as the residual takes them (socp_problem_set_blocks_dev: row b reads block b);
 * eps = sqrt(max(epsfcn, DBL_EPSILON)), formed as socp_fd_jacobian forms it.
 * COLUMNS.  Column 0 is X0; column c = 1 .. d starts from X0 with X[d+c-1] + h_c, h_c = eps |X0[d+c-1]|, or eps when that is zero
 * (MINPACK's rule).
 * STEPS.  All d + 1 trajectories take the residual's fixed RK4 steps: dt = (t2 - t1) / N, accumulated t, clamped last step, no step
 * when t2 <= t1 + dt / 2.  Steps are numbered k = 1 .. K.
 * SAMPLES.  One after step k iff k % stride == 0 or k == K:  tq = tk + step (tk the accumulated time before the step, step its
 * length);  J[r][c-1] = (X^c[r] - X^0[r]) / h_c for r = 0 .. d-1;  det as below.  The samples of slab [b][i] are stored in order up
 * to cap; count[b][i] = their number (samples beyond cap are counted, not stored, nothing is written past the slab; entries at or
 * beyond min(count, cap) keep what the buffer held).
 * DETERMINANT, a fixed sequence of IEEE operations (tests/jacobi_reference.py restates it).  Any entry of J not finite: det = NaN.
 * Otherwise Gaussian elimination with partial pivoting, for k = 0 .. d-1:
 *   the pivot row p is the smallest r >= k with |a[r][k]| maximal (strict >); rows k and p are swapped in the columns >= k, a swap
 *   with p != k flips the sign;  v_k = a[k][k];  v_k == 0.0: det = +0.0 and the elimination stops;
 *   for r > k: l = a[r][k] / v_k (one division), for c > k: a[r][c] = a[r][c] - l * a[k][c] (a product and a subtraction, unfused,
 *   in the reference-order flavour)
 *   det = (((v_0 v_1) v_2) ...), negated at the end when the number of swaps is odd.
 * DETECTION, neg(v) = (v < 0.0).  Consecutive samples j-1, j with j-1 >= skip are compared, those beyond cap included: a change is
 * counted when both determinants are non-NaN and neg(d0) != neg(d1).  nchange[b][i] = the number of changes;
 * tconj[b][i] = t0 + (t1 - t0) * (d0 / (d0 - d1)) at the FIRST change, in this operation order; NaN when there is none.
 * Jend holds the matrix J[r][c] of the LAST sample, row-major: dx(t_{i+1})/dp(t_i), what a rank test other than the plain
 * determinant needs (the free-final-time variant with x' in place of one column).  A zero-length or backward segment takes no
 * step: count = 0, nchange = 0, tconj = NaN, Jend all +0.0.
 * WHAT IT IS AND IS NOT.  A measuring instrument.  The classical statement holds for single shooting with a fixed initial state,
 * M = 1 (socp_regrid_batch moves any solution onto M2 = 1); for M > 1 each segment's determinant is reported for its own start
 * node.  The matrix is a forward difference: near t0 it is rank-deficient to rounding and the sign of its determinant is noise --
 * that is what skip is for.  A non-smooth control law (goddard with mu2 = 0) makes the fields jump.  With a free final time the
 * plain determinant is not the right test: use Jend.
 * socp_ctx_has_jacobi: 1 when the context's model has the entry, else 0.
 * SOCP_ERR_ARG: no problem set, B < 0, stride < 1, skip < 0, cap < 1, a NULL required pointer with B > 0 (all but Jend), _blocks with
 * params and param_stride != nparams + 2; B == 0: SOCP_OK without a launch; SOCP_ERR_UNSUPPORTED (the message says which): the
 * context's integrator is SOCP_INT_DOPRI5, or the model's launch table has no jacobi entry (a model with its own ComputeTraj -- the
 * interceptor -- and vtolUAV, for which it is not offered).  An error leaves the context unchanged.
 * One launch; socp_ctx_counters advances by B M (d + 1) trajectories.  The _dev form takes device pointers, enqueues on the
 * context's stream and neither copies nor synchronises; the host forms stage through that stream (tq and det travel both ways) and
 * return when the results are in the caller's arrays.  _blocks: per-row blocks like socp_residual_batch_blocks (any of params /
 * time / xnode may be NULL); the context's own blocks are restored afterwards. */
int socp_ctx_has_jacobi(const socp_ctx *ctx);          /* 1 / 0 */
int socp_jacobi_batch_dev(socp_ctx *ctx, int B, const double *d_Z, double epsfcn, int stride, int skip, int cap, double *d_tq,
                          double *d_det, int *d_count, int *d_nchange, double *d_tconj, double *d_Jend);
int socp_jacobi_batch(socp_ctx *ctx, int B, const double *Z, double epsfcn, int stride, int skip, int cap, double *tq, double *det,
                      int *count, int *nchange, double *tconj, double *Jend);
int socp_jacobi_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                             const double *xnode, double epsfcn, int stride, int skip, int cap, double *tq, double *det, int *count,
                             int *nchange, double *tconj, double *Jend);

/* The same test with EXACT Jacobi fields: J(t) = dx(t)/dp(t0) by forward-mode differentiation of the residual's own RK4 steps, and
 * the transition matrix Phi = dX(t_{i+1})/dX(t_i) of every segment as a by-product.  [ext] HamPath's expdhvfun provides this; the
 * reference does not.  For an explicit Runge-Kutta method, carrying the derivative through the steps is precisely the derivative
 * of the DISCRETE flow the residual integrates; there is no epsfcn and no step rule.  socp_jacobi_batch's forward difference is
 * wrong in the fourth digit on the nominal Goddard extremal (it starts at |v| = 1.7e-10, where vx / v is violently nonlinear).
 * Measured on the CPU restatement against the same recurrence in 240 bits, nominal Goddard start, one segment [0, 0.2640825],
 * N = 50 (error of Jend / max |J|;  det truth;  det forward difference with epsfcn 0 / 4 DBL_EPSILON;  det by this call):
 *   mu2 = 1                      1.5e-4 -> 3.5e-13    -1.26348e-8    -1.199e-8 / -1.135e-8     -1.26348027522e-8
 *   mu2 = 0.2                    7.7e-5 -> 3.7e-14    0 (singular)   -5.0e-24 / -6.7e-25       -2.4e-43
 *   mu2 = 0, sw = (0.05, 0.15)   3.7e-4 -> 2.5e-13    0              0.0 / 0.0                 0.0
 * Z[B][n] -> tq[B][M][cap], det[B][M][cap], count[B][M], nchange[B][M], tconj[B][M], Phi[B][M][s][C] (may be NULL; row-major: row r of
 * X, column c).  cols = SOCP_FIELDS_COSTATE: C = d columns, the unit vectors of p(t_i);  SOCP_FIELDS_ALL: C = s = 2d columns, the
 * unit vectors of X(t_i), x first.
 * SETUP, timeline, switching times, per-row blocks, STEPS, SAMPLES, the slab / cap rule and DETECTION (with skip) are word for word
 * those of socp_jacobi_batch.  There is no epsfcn.
 * DUAL NUMBERS.  A dual number is (v, d).  Every operation is one IEEE rounding per listed step, never contracted:
 *   a +- b = (a.v +- b.v, a.d +- b.d);   a b = (a.v b.v, (a.d b.v) + (a.v b.d));   a / b: q = a.v / b.v, (q, (a.d - q b.d) / b.v);
 *   -a and |a| act on both parts, |a| flips d when v < 0;
 *   sqrt a: s = sqrt(a.v), (s, a.d / (s + s)), the derivative +0.0 when s == 0 (Goddard's norm_u with the thrust off);
 *   exp a: e = the model's exp (exp_glibc for Goddard), (e, e a.d);
 *   tanh a: th = tanh(a.v), the device library's tanh (vtolUAV's map), (th, (1.0 - th th) a.d) -- the product th th, the difference
 *   from 1.0, the product with a.d, in that order (d_tanh, dual.hpp; dual numbers only, the nested and wide numbers have no such rule);
 *   comparisons read v; a branch's derivative is that of the branch taken;
 *   a plain double c (a parameter, a literal, t, h, and a control or penalty that the law makes a constant: thrust off or full, a
 *   clamped control, an inactive penalty) takes part with its zero derivative terms DROPPED, not computed:
 *   c a = (c v, c d);  a / c = (v / c, d / c);  c / a: q = c / v, (q, (-(q d)) / v);  c +- a = (c +- v, +-d);  a - c = (v - c, d).
 *   A component of the right-hand side that is a constant has the derivative +0.0.
 * The model's right-hand side is its rhs_t trait (plugin_impl.hpp): the reference-order text on plain IEEE operations.
 * COLUMNS.  Column c starts from (X0, e_k): k = d + c (COSTATE), k = c (ALL).  All columns take the residual's RK4 steps in the
 * association order of odeTools.cpp:89-98 on dual numbers, t and the step plain doubles; the value part of every column is the
 * reference-order residual's trajectory, bit for bit.
 * DETERMINANT.  J[r][c'] = the derivative part of component r < d in the column of p_c'(t_i); det by the elimination of
 * socp_jacobi_batch, unchanged.
 * Phi holds the derivative parts of all s components after the last step.  A zero-length or backward segment takes no step:
 * count = 0, nchange = 0, tconj = NaN, Phi = the unit columns it started from.
 * ONE OBJECT, NO CONTRACTION: the kernels are built once, without contraction, and serve both variants -- a throughput-flavour
 * context returns the same bits, and the value trajectories are the reference-order ones, not the fast residual's.
 * WHAT IT IS AND IS NOT.  The caveats of the Jacobi test stand: the classical statement is for M = 1 with a fixed initial state, and
 * with a free final time the plain determinant is not the right test (use Phi).  The result is exact for the DISCRETE flow, to
 * rounding -- not for the differential equation.  A determinant that is zero to rounding (table above) has no sign to read.  A
 * state-dependent kink (Switch < 0, a saturation) differentiates the branch taken.  vtolUAV: rhs_t is the reference-order text of
 * both flavours' contexts (control_t, map_exact_t on T: the table read as the residual reads it, the NaN reset testing the VALUE
 * part and zeroing the whole number, the upstream quirks kept); tanh is the device library's, so wherever the map is live the bits
 * are the kernel's own and the test holds Phi to a 240-bit evaluation, with an EMPTY map every bit is the restatement's
 * (tests/vtol_exact_reference.py).  Out of scope: the adaptive integrator, the
 * interceptor, a jac = 2 for socp_tangent_batch / socp_singular_batch / socp_branch_batch, hybrj for Goddard
 * (socp_ctx_has_variational stays 0 for it), more than one GPU.
 * socp_ctx_has_fields: 1 when the context's model has the entry (vtolUAV: after socp_ctx_set_exact_hooks(ctx, 1)), else 0.
 * SOCP_ERR_ARG: as socp_jacobi_batch, and cols outside 0 .. 1; B == 0: SOCP_OK without a launch; SOCP_ERR_UNSUPPORTED (the message
 * says which): the context's integrator is SOCP_INT_DOPRI5, or the model's launch table has no fields entry (the interceptor,
 * vtolUAV before socp_ctx_set_exact_hooks, a plugin without the rhs_t trait).  An error writes nothing and leaves the context unchanged.
 * One launch; socp_ctx_counters advances by B M C trajectories.  The _dev, host and _blocks forms as for socp_jacobi_batch. */
#define SOCP_FIELDS_COSTATE 0   /* C = d columns: the unit vectors of p(t_i)                 */
#define SOCP_FIELDS_ALL     1   /* C = s = 2d columns: the unit vectors of X(t_i), x first    */
int socp_ctx_has_fields(const socp_ctx *ctx);          /* 1 / 0 */
int socp_fields_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int cols, int stride, int skip, int cap, double *d_tq,
                          double *d_det, int *d_count, int *d_nchange, double *d_tconj, double *d_Phi);
int socp_fields_batch(socp_ctx *ctx, int B, const double *Z, int cols, int stride, int skip, int cap, double *tq, double *det,
                      int *count, int *nchange, double *tconj, double *Phi);
int socp_fields_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                             const double *xnode, int cols, int stride, int skip, int cap, double *tq, double *det, int *count,
                             int *nchange, double *tconj, double *Phi);

/* The EXACT Jacobian dF/dz of the shooting function itself, for a whole batch of unknown vectors: dual numbers carried through the
 * residual's own RK4 steps AND through the boundary, continuity, Hamiltonian and switching rows, with a column for every free time.
 * [ext] The reference differences (hybrd) or integrates variational equations the model must bring (hybrj); Goddard brings none.
 * Every other consumer of the Jacobian here reads a forward difference, which on the nominal Goddard extremal is wrong in the fourth
 * digit (table above).  Z[B][n] -> Fjac[B][n*n], COLUMN-major with leading dimension n -- the layout of socp_fd_jacobian_multi_dev, so
 * the result goes unchanged into socp_linsolve_batch_dev and socp_svd_batch_dev -- and, unless NULL, F[B][n], the residual.
 * SETUP, timeline, switching times and per-row blocks are those of socp_residual_batch; the rows and the unknowns are its rows and
 * unknowns (state unknowns z[S i + c] of node i < M, S = 2d, then the free times in node order).  DUAL NUMBERS as in socp_fields_batch.
 * COLUMNS AND LANES.  Segment i of row b carries S + 1 columns.  Column c < S starts from (X0, e_c), X0 = z[S i ..): the unknown
 * z[S i + c].  Column S starts from (X0, +0.0) and is the segment's LENGTH L = t2 - t1.  One lane per column, G = S + 1 neighbouring
 * lanes of one wavefront, 64 / G groups per wave (Goddard 15 lanes, 4 groups; double integrator 13, 4; covid19 9, 7).
 * STEPS.  ONE text for every lane.  t1 = (t1, +0.0), t2 = (t2, delta), delta = 1.0 in the length column and +0.0 in the state
 * columns; dt = (t2 - t1) / N (dual - dual, then / the plain N); t = t1; while t.v < (t2.v - dt.v / 2) [and the step guard of the
 * residual]: step = (t.v + dt.v > t2.v) ? (t2 - t) : dt; one RK4 step; t = t + dt -- all by the dual rules, conditions on value
 * parts.  The RK4 step is that of odeTools.cpp:89-98 in its association order with a DUAL step:
 *   h2 = step / 2.0; th = t + step / 2.0; F1 = f(t.v, X); Y = X + h2 F1; F2 = f(th.v, Y); Y = X + h2 F2; F3 = f(th.v, Y);
 *   Y = X + step F3; Fs = F2 + F3; F4 = f((t + step).v, Y); h6 = step / 6.0; X = X + h6 (F1 + (F4 + 2.0 Fs))
 * where every product h F is the full dual x dual rule: the term h.d F.v IS computed, also where h.d is zero.  f is the model's
 * rhs_t and receives the VALUE part of the stage time.  Consequences: the value trajectory of every column is the reference-order
 * residual's, bit for bit; the derivative parts of the state columns equal Phi of socp_fields_batch (SOCP_FIELDS_ALL) as numbers,
 * though not in the sign of a zero (there h is plain and its zero term dropped).
 * WHAT IS NOT DIFFERENTIATED.  An explicit dependence of the right-hand side, the Hamiltonian or the switching row on t: the in-tree
 * models use t only in comparisons.  The dependence on a switching time through the control law's comparisons (Goddard with
 * mu2 = 0: t <= sw0, t <= sw1): the discrete flow is piecewise constant in it.  A state-dependent kink differentiates the branch
 * taken.  So column k of a free time holds the derivative through the LENGTHS of the segments alone.
 * ROWS.  segment_residual on duals: each lane evaluates the rows its segment owns and stores the derivative part at (row, its
 * column); value parts go to F.
 *   segment 0, on the START state: rows j < d: X[j + d] where component j of node 0 is FREE, else X[j] - xd[j]; row ft_row[0] (t0
 *   FREE): hamiltonian_t(t1, X).  The length column has no part in these rows.
 *   segment i < M - 1, on the END state X, with Xp = z[S (i + 1) ..) as constants: row ft_row[i + 1] (that time FREE):
 *   switching_fn_t(t2, X, (Xp, +0.0)); rows S (i + 1) + j and S (i + 1) + d + j: FIXED: X[j] - xd[j] and the value Xp[j] - xd[j]
 *   (no derivative stored from this side); CONTINUOUS: X[j] - Xp[j] and X[j + d] - Xp[j + d].
 *   segment M - 1, on the END state: rows d + j: X[j + d] where component j of node M is FREE, else X[j] - xd[j]; row ft_row[M] (tf
 *   FREE): hamiltonian_t(t2, X).
 *   The part of node i's rows (1 <= i < M) that depends on segment i's START state belongs to the state lanes of segment i, which
 *   own those columns: -1.0 at (S i + c, S i + c) where component (c mod d) is CONTINUOUS; 1.0 at (S i + d + c, S i + c), c < d, where
 *   it is FIXED; and, where the model's free-time row is H(t, X) - H(t, Xp) (trait kSwitchingReadsXp: the double integrator,
 *   covid19; not Goddard, whose row is H(t, X)), the derivative part of -hamiltonian_t(t1, (X0, e_c)) at (ft_row[i], S i + c).
 *   Every entry then has exactly one writer.
 * CUSTOM FINAL ROWS AND THE SWITCHING_STATE HOOK (vtolUAV; a plugin through the traits of plugin_impl.hpp).  A model whose last node
 *   has rows of its own (kCustomFinal) brings final_row_t, the text of final_row over a number type: rows d + j of segment M - 1 are
 *   final_row_t(j, mode, X, xd) on the dual END state in either mode -- vtolUAV: X[j + d] - invSigmaXwp (nWP_tot - nWP) (X[j] - xd[j])
 *   - 0.02 (X[j] - xd[j]) where component j is FREE, X[j] - xd[j] otherwise -- and row ft_row[M] is hamiltonian_t(t2, X) +
 *   final_h_offset, the offset a plain double.  A model with a switching_state hook brings switching_state_t, the hook with X over a
 *   number type and Xp as the plain doubles they are: where component j of interior node i + 1 is FREE, rows S (i + 1) + j and
 *   S (i + 1) + d + j are its f_state and f_costate on the dual END state of segment i -- vtolUAV: X[j] - Xp[j] and
 *   (X[j + d] - Xp[j + d]) - invSigmaXwp (X[j] - xd[j]) -- stored by the lanes of the segment that ENDS there, its length lane
 *   included.  The model must also declare kSwitchingStateXpContinuous = true: the PROMISE that the hook reads Xp only as -Xp[j] in
 *   f_state and -Xp[j + d] in f_costate.  The state lanes of segment i + 1 then store -1.0 at (S (i + 1) + c, S (i + 1) + c) for
 *   these components exactly as for a CONTINUOUS one: every entry keeps one writer.  Without final_row_t, or without switching_state_t
 *   and the promise, such a model has no entry.
 * FREE-TIME COLUMNS.  The segment lies between the junctions A <= i and Bn >= i + 1 (A = i or lo[i], Bn = i + 1 or hi[i + 1]).  For
 * f in {A, Bn} with node f FREE and unknown index k, the length lane stores w (d row / d L) -- one product -- at (row, k) for every
 * END-state row above, w = c(i + 1, f) - c(i, f), where c(j, f) is 1.0 for j == f, (double)(j - a) / (double)(b - a) for a node j
 * interpolated between the junctions a and b = f, 1.0 minus that for a = f, and 0.0 otherwise.  Nothing is stored when w == 0.0.
 * The matrix is zero-filled first, on the call's stream; then ONE launch stores every entry listed above (zeros included) directly.
 * A zero-length or backward segment takes no step: its continuity block is the unit matrix, its length column zero.
 * ONE OBJECT, NO CONTRACTION, as socp_fields_batch: a throughput-flavour context returns the same bits, and F is
 * socp_residual_batch of a reference-order context, bit for bit.
 * WHAT IT IS AND IS NOT.  Exact for the DISCRETE flow, to rounding, apart from what is listed as not differentiated; the forward
 * difference sees those dependences (and noise).  tests/exact_jacobian_reference.py restates the definition; the tests compare whole
 * buffers to it.  Out of scope: jac = 2 in socp_tangent_batch / socp_singular_batch / socp_branch_batch (they keep 0 .. 1), hybrj
 * for Goddard inside socp_chains_solve, the adaptive integrator, the interceptor, derivatives with respect to parameters,
 * more than one GPU.  vtolUAV has the entry in both flavours once the context asked for it (socp_ctx_set_exact_hooks; one reference-order object, kernels_vtol_exact.hip; 13 lanes, 4 groups):
 * with an EMPTY map every bit is the restatement's, with a live map tanh is the device library's and the matrix is held to a 240-bit
 * evaluation (tests/vtol_exact_reference.py, tests/test_gpu_vtol_exact.py); its sensitivities, gains, guidance and Hamiltonian
 * point calls stay refused.
 * socp_ctx_has_exact_jacobian: 1 when the context's model has the entry -- the traits rhs_t, hamiltonian_t and switching_fn_t, no
 * ComputeTraj of its own, final_row_t if it has custom final rows, switching_state_t with kSwitchingStateXpContinuous if it has a
 * switching_state hook; vtolUAV: after socp_ctx_set_exact_hooks(ctx, 1) -- else 0; SOCP_ERR_ARG for a NULL context (as
 * socp_ctx_has_fields).
 * SOCP_ERR_ARG: no problem set, B < 0, a NULL Z or Fjac with B > 0, a wrong parameter stride (_blocks); B == 0: SOCP_OK without a
 * launch; SOCP_ERR_UNSUPPORTED (the message says which): the context's integrator is SOCP_INT_DOPRI5, the model's launch table has no
 * exact_jacobian entry (the interceptor, vtolUAV before socp_ctx_set_exact_hooks, a plugin without the traits), or the problem has a FREE state component on an
 * interior node of a model other than vtolUAV (its rows are the model's SwitchingStateFunction; the launch table does not say
 * whether a plugin's entry covers them).  An error writes nothing and leaves the context unchanged.
 * socp_ctx_counters advances by B M (S + 1) trajectories and one launch.  The _dev, host and _blocks forms as for socp_fields_batch. */
int socp_ctx_has_exact_jacobian(const socp_ctx *ctx);   /* 1 / 0; SOCP_ERR_ARG for a NULL context */
int socp_exact_jacobian_batch_dev(socp_ctx *ctx, int B, const double *d_Z, double *d_Fjac, double *d_F /* or NULL */);
int socp_exact_jacobian_batch(socp_ctx *ctx, int B, const double *Z, double *Fjac, double *F);
int socp_exact_jacobian_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                                     const double *time, const double *xnode, double *Fjac, double *F);

/* replaces: shooting::Move(tf) (shooting.cpp:383-437) for a whole batch: the state ON a stored solution at a query time, and the
 * re-grid the reference's multi-stage flows build from it (testGoddard.cpp:115-145: vX[i] = Move(vt[i]), then InitShooting(vt, vX)
 * on a new structure).  Z[B][n], tq[B][K] -> Xq[B][K][s]; tout[B][K] (may be NULL) = the time actually reached.
 * Per row b and query k, with z = Z[b], s = 2 d and tl(j) timeline entry j exactly as the residual forms it (socp_timeline; row
 * b's own blocks when socp_problem_set_blocks_dev is in force):
 *   t0 = tl(0), te = tl(M)                                   (:391-405  FIXED: the table's time, FREE: the unknown)
 *   target = (q >= t0 && q <= te) ? q : te                   (:407-409  out of range and NaN go to te)
 *   seg = 0; while (seg < M-1 && tl(seg+1) < target) seg++   (:416-424  the bound only makes a NaN / disordered timeline safe)
 *   X = z[s seg .. s seg + s)                                (:426-431)
 *   X <- model::ComputeTraj(tl(seg), X, target)              (:433      with the switching times the residual uses for the row)
 * So a query equal to an interior node time integrates the WHOLE previous segment (it does not copy the node state), q == t0 is a
 * zero-length integration that returns z[0 .. s) bit for bit, and every query costs one full step_nbr-step (or adaptive)
 * integration from its segment's start, as in the reference: it is not a sample of a stored trajectory.  The variational state
 * is not moved (the reference drops isJac here too, :440-444).  All models, both variants, both integrators.
 * socp_regrid_*: B solutions onto a new structure of M2 segments with time modes mode_t2[M2+1] (HOST array, read before the call
 * returns) and node times T2[B][M2+1]:
 *   Z2[b][s j + c]     = Move(T2[b][j])[c]  for j < M2
 *   Z2[b][s M2 + r]    = T2[b][j_r] AS GIVEN (not clamped), j_r the r-th FREE node in node order   (shooting.cpp:228-243)
 *   xnode2[b][j][:]    = Move(T2[b][j])     for j = 0 .. M2 (may be NULL): InitShooting(vt, vX)'s data->X, the block
 *                        socp_problem_set_blocks_dev and socp_chains_solve's x_goal take; the caller's own T2 is the time block
 * socp_regrid_num_param = n2 = s M2 + #FREE(mode_t2), the row length of Z2.  1 <= M2 <= 255, so that the mode table travels as a
 * kernel argument and the _dev form neither copies from pageable memory nor synchronises.
 * SOCP_ERR_ARG: no problem set, B < 0, K < 0, a NULL required pointer with B K > 0, _blocks with params and param_stride !=
 * nparams + 2, M2 outside 1 .. 255, a mode_t2 entry outside FIXED / FREE / CONTINUOUS; B == 0 or K == 0: SOCP_OK without a launch;
 * a model whose launch table has no move entry: SOCP_ERR_UNSUPPORTED.  An error leaves the context unchanged.
 * One launch (re-grid: two -- a move with K = M2 + 1 into d_xnode2, or into a workspace buffer of the context when that is NULL,
 * then the pack); socp_ctx_counters advances by B K trajectories (re-grid: B (M2 + 1)).  The _dev forms take device pointers and
 * only enqueue on the context's stream (one exception: socp_regrid_batch_dev with d_xnode2 NULL allocates its grow-only workspace
 * buffer the first time, and again when B (M2 + 1) outgrows it -- a hipMalloc, which synchronises the device; pass d_xnode2 where
 * that matters); the host forms stage through that stream and return when the results are in the caller's
 * arrays.  _blocks: per-row blocks like socp_residual_batch_blocks (any of params / time / xnode may be NULL); the context's own
 * blocks are restored afterwards. */
int socp_move_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int K, const double *d_tq, double *d_Xq, double *d_tout);
int socp_move_batch(socp_ctx *ctx, int B, const double *Z, int K, const double *tq, double *Xq, double *tout);
int socp_move_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                           const double *time, const double *xnode, int K, const double *tq, double *Xq, double *tout);
int socp_regrid_num_param(const socp_ctx *ctx, int M2, const int *mode_t2);
int socp_regrid_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int M2, const int *mode_t2, const double *d_T2, double *d_Z2,
                          double *d_xnode2);
int socp_regrid_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                             const double *xnode, int M2, const int *mode_t2, const double *T2, double *Z2, double *xnode2);

/* replaces: shooting::ShootingFunctionJacobian (shooting.cpp:996-1130), variational Jacobian
 * for models with modelOrder == 1 (socp_ctx_has_variational); fjac column-major as handed to hybrj (shooting.cpp:889-893).
 * The variational state follows the context's integrator (socp_ctx_set_integrator): fixed-step RK4, or -- as the reference does
 * for EVERY integrate() call when built with -D_USE_BOOST, odeTools.cpp:129-134 -- adaptive Dormand-Prince on the whole augmented
 * state, one wavefront per trajectory with per-wave step control ([ext] like the state-only adaptive path: pinned to the published pair and a 240-bit replay, agreement with Boost's own code unverified). */
int socp_var_jacobian(socp_ctx *ctx, const double *z, double *fjac);
/* The same for `np` unknown vectors of one problem structure, device pointers: Z[np][n] -> Fjac[np][n*n]; one wavefront per
 * (problem, segment); per-problem blocks (socp_problem_set_blocks_dev) apply. */
int socp_var_jacobian_multi_dev(socp_ctx *ctx, int np, const double *d_Z, double *d_Fjac);

/* Parameter sensitivities of a whole batch of converged unknown vectors: the tangent dz/dtheta of the solution branch
 * F(z; theta) = 0, i.e. the solution of J dz = -dF/dtheta with J the shooting Jacobian (implicit-function theorem).  [ext] The
 * reference restarts every continuation step from the previous solution (shooting.cpp:598-778); z + dtheta dz is the first-order
 * predictor, dp0/dx0 the gain of the neighbouring-extremal guidance law around a stored extremal.  A direction names ONE entry theta
 * of a row's blocks (its own when socp_problem_set_blocks_dev is in force, the shared tables otherwise): */
#define SOCP_DIR_PARAM 0   /* index: slot of the packed block, 0 .. nparams+1 (the two trailing slots are sw0, sw1) */
#define SOCP_DIR_TIME  1   /* index: node j, 0 .. M        (time[b][j]) */
#define SOCP_DIR_XNODE 2   /* index: j*2d + c, c < d       (xnode[b][j][c]; only the first d of a node row are read) */
/* Z[B][n], K directions (dir_kind[K], dir_index[K]: HOST arrays, read before the call returns -- they travel as a kernel argument;
 * 1 <= K <= 16) -> dZ[B][K][n], info[B], Fp[B][K][n] (may be NULL: dF/dtheta_k as differenced).  Per row b:
 *   1. e = sqrt(max(epsfcn, DBL_EPSILON))                   (the step rule of MINPACK's fdjac1, as socp_fd_jacobian)
 *   2. F0 = F(z; blocks)
 *   3. per direction k, theta the addressed entry: h = e |theta|, or e when theta == 0.0 (so h > 0, and mu2 + h > 0 when mu2 > 0);
 *      Fk = the residual with that ONE entry replaced by theta + h;  G[k][i] = (Fk[i] - F0[i]) / h.  The time of a FREE node, an
 *      xnode entry the modes never read or a parameter the model ignores is not refused: G = 0 and dz = -+0
 *   4. jac == 0: J = the forward-difference Jacobian of socp_fd_jacobian_multi_dev at (z, F0) with this epsfcn and dedup on;
 *      jac == 1: the variational Jacobian of socp_var_jacobian_multi_dev (a model without one: SOCP_ERR_UNSUPPORTED)
 *   5. dZ[b][k] = the solution of J x = -G[k] (the negation is exact) by the elimination of 6.
 *   6. on the column-major A and the right-hand sides y, for k = 0 .. n-1:
 *        best = |a_kk|, p = k;  for i = k+1 .. n-1 in order: if (|a_ik| > best) (best, p) = (|a_ik|, i)      (the first maximum wins; a
 *                                                                             NaN is never chosen over a number)
 *        if (!(best > 0.0) or best is infinite): info = k + 1, all K solution rows of this problem = NaN, stop
 *        swap rows k and p of A (all columns) and of every y;  l_i = a_ik / a_kk;
 *        a_ij <- a_ij - l_i a_kj,  y_i <- y_i - l_i y_k   for i, j > k
 *      then for k = n-1 .. 0:  x_k = y_k / a_kk;  y_i <- y_i - a_ik x_k for i < k;   info = 0, or n + 1 when a solution entry is not
 *      finite.  Every operation is element-wise and the pivot search is the only reduction, so the result does not depend on how the
 *      work is spread over lanes; in reference-order contexts (SOCP_VARIANT_AUTO / LANE_EXACT) each operation is one IEEE rounding
 *      (no contraction), in SOCP_VARIANT_LANE_FAST contexts the updates are fused multiply-adds.
 * All models, both variants, both integrators: only the launch-table entries residual, fdjac and var_jacobian are used, so a plugin
 * has the call without change.  A Goddard smooth-law promise (socp_problem_blocks_all_smooth) covers the moved blocks.
 * socp_tangent_work_bytes: the bytes of d_work for (B, K) on this context's problem (0 for arguments the call would refuse): the
 * block rows, replicated unknowns and residual rows of the B (K + 1) launched rows, J[B][n*n], h[B][K], and on a model with
 * variational equations what socp_var_jacobian_multi_dev integrates in.
 * Launches of the _dev form: the block rows; ONE residual launch of B (K + 1) rows (the base rows wait for nothing); the Jacobian
 * (1 launch, variational: 3); the differences; the elimination.  socp_ctx_counters advances by B (K + 1) M trajectories plus the
 * Jacobian's (np T of the dedup list, or B M) and by 5 launches (variational: 7).
 * SOCP_ERR_ARG: no problem set, B < 0, K outside 1 .. 16, a kind outside 0 .. 2 or an index outside its range, jac outside 0 .. 1, a
 * NULL required pointer (dir_kind, dir_index; with B > 0: Z, dZ, info, d_work), work_bytes below socp_tangent_work_bytes, _blocks
 * with params and param_stride != nparams + 2; B == 0: SOCP_OK without a launch; SOCP_ERR_UNSUPPORTED: jac == 1 without
 * variational equations, n above the elimination's limit (below).  An error leaves the context unchanged.
 * The _dev form takes device pointers (the directions stay host arrays), only enqueues on the context's stream and neither
 * allocates, copies nor synchronises: the caller owns d_work.  The host forms stage through that stream, take the workspace from
 * the context's grow-only buffers and return when the results are in the caller's arrays.  _blocks: per-row blocks like
 * socp_residual_batch_blocks (any of params / time / xnode may be NULL); the context's own blocks are restored afterwards.
 * Not covered: no predictor inside socp_chains_solve, one GPU.  info says singular, not ill-conditioned: how close J is to singular
 * is what socp_singular_batch (below) reports. */
size_t socp_tangent_work_bytes(const socp_ctx *ctx, int B, int K);
int socp_tangent_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int K, const int *dir_kind, const int *dir_index,
                           double epsfcn, int jac, void *d_work, size_t work_bytes,
                           double *d_dZ, int *d_info, double *d_Fp);
int socp_tangent_batch(socp_ctx *ctx, int B, const double *Z, int K, const int *dir_kind, const int *dir_index,
                       double epsfcn, int jac, double *dZ, int *info, double *Fp);
int socp_tangent_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                              const double *time, const double *xnode, int K, const int *dir_kind, const int *dir_index,
                              double epsfcn, int jac, double *dZ, int *info, double *Fp);
/* The linear-algebra half on its own, on the context's stream and in its variant: A[B][n*n] column-major, Y[B][K][n] (overwritten by
 * the solutions X), info[B]: the elimination of 6. above.  One problem per workgroup (n <= 16: four per workgroup); when the matrix
 * and its right-hand sides fit 64 KiB of LDS they are eliminated there and A is left as it was, otherwise A is eliminated in place in
 * HBM with the pivot row and the multiplier column of each step staged in LDS -- which bounds n and K: 2 n + K + 16 doubles (for
 * n <= 16: four times that) must fit 64 KiB.  What A holds after a call on the HBM path is unspecified (work in progress of the
 * elimination); callers that need A afterwards keep a copy.
 * SOCP_ERR_ARG: B < 0, n < 1, K < 1, n above that bound, a NULL pointer with B > 0; B == 0: SOCP_OK without a launch.  One launch. */
int socp_linsolve_batch_dev(socp_ctx *ctx, int B, int n, int K, double *d_A, double *d_Y, int *d_info);

/* How close to singular: the singular values of B small dense matrices, and of the shooting Jacobians of a whole sweep.
 *
 * socp_svd_batch_dev is the linear-algebra half: model-independent (no problem has to be set), on the context's stream and in its
 * variant, ONE launch, no allocation, no synchronisation.  A[B][n*n] column-major, left as it was -> sigma[B][n] descending,
 * Vt[B][n][n] (may be NULL; row j is the right singular vector of sigma[j]), sweeps[B], info[B].  One-sided Jacobi (Hestenes)
 * rotations on the ROWS of the matrix, per matrix:
 *   start.    W = a copy of A; w_p = its row p (entries A[p + i n], i = 0 .. n-1);  tol = n DBL_EPSILON (the error bound of an n-term
 *             dot product relative to |w_p| |w_q|: below it gamma is rounding noise).  An entry of A that is not finite: info = 2,
 *             sweeps = 0, sigma and Vt all NaN.
 *   schedule. round-robin, all pairs of a step disjoint:  m = n + (n & 1);  steps s = 0 .. m-2, slots k = 0 .. m/2-1;
 *             k == 0: (a, b) = (m-1, s);  else a = (s + k) mod (m-1), b = (s - k + m - 1) mod (m-1);  p = min(a, b), q = max(a, b);
 *             the pair is skipped when q >= n (the phantom row of an odd n).  Every pair p < q occurs exactly once per sweep.
 *   pair.     alpha = sum w_pi^2, beta = sum w_qi^2, gamma = sum w_pi w_qi: each sum starts from +0.0 and adds one rounded product
 *             at a time, i = 0 .. n-1.  No rotation when gamma == 0 or |gamma| <= fl(fl(tol sqrt(alpha)) sqrt(beta)).  Otherwise
 *               zeta = (beta - alpha) / (2 gamma);  t = (zeta >= 0 ? 1 : -1) / (|zeta| + sqrt(1 + zeta zeta));
 *               c = 1 / sqrt(1 + t t);  s = c t;   for every i: (w_pi, w_qi) <- (c w_pi - s w_qi, s w_pi + c w_qi)
 *   sweep.    all m - 1 steps.  The first sweep in which no pair rotates ends the iteration: info = 0 and sweeps counts that sweep
 *             too.  If sweep max_sweeps still rotated: info = 1, sweeps = max_sweeps, the outputs come from W as it stands.
 *   finish.   sigma_p = sqrt(sum_i w_pi^2), the same sequential sum; ordered descending, equal values by ascending row, ranked by
 *             counting (so the result does not depend on how the work is spread);  the Vt row = w_p / sigma_p, all zeros when
 *             sigma_p == 0, then negated if its entry of largest magnitude (the first among equals) is negative.
 * In reference-order contexts (SOCP_VARIANT_AUTO / LANE_EXACT) every operation is one IEEE rounding: no contraction, IEEE division
 * and square root, so the result is reproducible bit for bit and does not depend on how matrices are batched.  In
 * SOCP_VARIANT_LANE_FAST contexts the sums and the updates may be fused multiply-adds and the sums may take any order.
 * The right singular vectors come without accumulating anything, as the normalised rows; left singular vectors are not produced.
 * The matrix lives in LDS (row stride n | 1), with its n row norms and 32 bytes of flags: n <= 142 is the largest that fits the
 * 160 KiB of a compute unit -- so not the n = 253 and 832 of the large chains.  Accuracy: |sigma^ - sigma| is of the order
 * n DBL_EPSILON sigma_max (an ABSOLUTE bound; tests/test_svd_cpu.py measures it against LAPACK); the relative accuracy of small
 * singular values is not promised.
 * SOCP_ERR_ARG: B < 0, n < 1, max_sweeps outside 1 .. 1000, a NULL required pointer (A, sigma, sweeps, info) with B > 0;
 * SOCP_ERR_UNSUPPORTED: n > 142;  B == 0: SOCP_OK without a launch.  An error writes nothing. */
int socp_svd_batch_dev(socp_ctx *ctx, int B, int n, const double *d_A, int max_sweeps,
                       double *d_sigma, double *d_Vt, int *d_sweeps, int *d_info);
/* The model half: Z[B][n] -> sigma[B][n] descending, vmin[B][n] (the right singular vector of sigma[n-1]: the direction in which a
 * branch turns at a fold), colnorm[B][n] (may be NULL), sweeps[B], info[B].  Per row b:
 *   1. F0 = F(z; blocks)
 *   2. J exactly as step 4 of socp_tangent_batch: jac == 0 the forward-difference Jacobian of socp_fd_jacobian_multi_dev at (z, F0)
 *      with this epsfcn and dedup on; jac == 1 the variational Jacobian (a model without one: SOCP_ERR_UNSUPPORTED)
 *   3. scale == 1: colnorm_j = sqrt(sum_i J_ij^2), the sum in the order i = 0 .. n-1; a zero is replaced by 1; J_ij <- J_ij / colnorm_j
 *      (what MINPACK's mode = 1 scaling does with the first Jacobian);  scale == 0: colnorm = 1
 *   4. the decomposition above; vmin = the last row of Vt.  With scale == 1 it is in the scaled variables: x_j = colnorm_j z_j.
 * All models, both variants, both integrators: only the launch-table entries residual, fdjac and var_jacobian are used, so a plugin
 * has the call without change.
 * socp_singular_work_bytes: the bytes of d_work for B rows on this context's problem (0 without a problem or for B < 0): F[B][n],
 * J[B][n*n] and, on a model with variational equations, what socp_var_jacobian_multi_dev integrates in.
 * Launches of the _dev form: the residual; the Jacobian (1 launch, variational: 3); the column norms (only when scale == 1 or colnorm
 * is given); the decomposition.  socp_ctx_counters advances by B M trajectories plus the Jacobian's (np T of the dedup list, or B M)
 * and by 3 or 4 launches (variational: 5 or 6).
 * SOCP_ERR_ARG: no problem set, B < 0, jac or scale outside 0 .. 1, max_sweeps outside 1 .. 1000, a NULL required pointer with B > 0
 * (Z, sigma, vmin, sweeps, info, d_work), work_bytes below socp_singular_work_bytes, _blocks with params and param_stride !=
 * nparams + 2;  B == 0: SOCP_OK without a launch;  SOCP_ERR_UNSUPPORTED: jac == 1 without variational equations, n > 142.  An error
 * leaves the context unchanged and writes nothing.
 * The _dev form takes device pointers, only enqueues on the context's stream and neither allocates, copies nor synchronises.  The
 * host forms stage through that stream, take the workspace from the context's grow-only buffers and return when the results are in
 * the caller's arrays.  _blocks: per-row blocks like socp_residual_batch_blocks (any of params / time / xnode may be NULL); the
 * context's own blocks are restored afterwards.
 * Not covered: left singular vectors; n above 142 (n = 253 and 832); one GPU; relative accuracy of small singular values. */
size_t socp_singular_work_bytes(const socp_ctx *ctx, int B);
int socp_singular_batch_dev(socp_ctx *ctx, int B, const double *d_Z, double epsfcn, int jac, int scale, int max_sweeps,
                            void *d_work, size_t work_bytes, double *d_sigma, double *d_vmin, double *d_colnorm,
                            int *d_sweeps, int *d_info);
int socp_singular_batch(socp_ctx *ctx, int B, const double *Z, double epsfcn, int jac, int scale, int max_sweeps,
                        double *sigma, double *vmin, double *colnorm, int *sweeps, int *info);
int socp_singular_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride,
                               const double *time, const double *xnode, double epsfcn, int jac, int scale, int max_sweeps,
                               double *sigma, double *vmin, double *colnorm, int *sweeps, int *info);

/* Past a fold: pseudo-arclength (Keller) predictor-corrector continuation of B rows at once.  [ext] The reference moves a parameter
 * by natural-parameter homotopy (shooting.cpp:598-778; socp_chains_solve): it asks for the root at the NEXT parameter value, which
 * does not exist behind a fold of the branch.  Here the parameter is an unknown like the others and the branch is followed by its
 * arclength, so a fold is a point like any other.  What indirect-methods tools with a path-following layer (HamPath) do.
 *
 * Setting.  ONE direction (dir_kind, dir_index) for the call, with the meaning and the range checks of socp_tangent_batch; theta is
 * that ONE entry of a row's blocks (its own when per-row blocks are in force, the shared tables otherwise).  The internal unknown is
 * y = (z_0 .. z_{n-1}, lambda) with lambda = theta / wtheta: the caller's scale wtheta > 0 makes arclength meaningful when theta is
 * ~310 and costates ~1e-2 (1.0: no scaling).  EVERY evaluation uses theta = fl(lambda wtheta), point 0's included, with
 * lambda_0 = fl(theta_block / wtheta): with wtheta != 1 the start may be evaluated one ulp from the block's value. */
typedef struct socp_branch_options {
    double epsfcn;      /* the step rule of the differences, as socp_tangent_batch */
    int jac;            /* 0 forward-difference Jacobian, 1 variational */
    double wtheta;      /* the scale above: > 0 and finite */
    int dir;            /* +1 or -1: the initial orientation in theta */
    double h0, hmin, hmax, grow;   /* arclength step: the first, the smallest (below it: STEP_TOO_SMALL), the largest, the growth factor >= 1 */
    int kfast;          /* a step accepted with at most this many corrector updates lets h grow */
    int max_corr;       /* corrector updates allowed per step */
    double ftol;        /* acceptance bar on ||F||inf */
    int have_goal;      /* != 0: stop when theta crosses goal */
    double goal;
    int cap;            /* points kept per row, >= 2 */
    int rounds;         /* number of rounds */
} socp_branch_options;
#define SOCP_BRANCH_RUNNING        0   /* the rounds ran out; the accepted points are valid, call again from the last one to go on */
#define SOCP_BRANCH_REACHED        1   /* the goal was crossed */
#define SOCP_BRANCH_FULL           2   /* cap points recorded */
#define SOCP_BRANCH_STEP_TOO_SMALL 3   /* h fell below hmin */
#define SOCP_BRANCH_SINGULAR       4   /* the tangent system was singular (a bifurcation is reported, not resolved) */
#define SOCP_BRANCH_BAD_START      5   /* F at the start is not finite */
/* Z[B][n] -> per row: Y[B][cap][n+1] (z then theta of every accepted point; unused slots NaN), ttheta[B][cap] (the unit tangent's
 * lambda-component at that point), rnorm[B][cap] (||F||inf there), count[B], nfold[B], ifold[B] (index of the first point behind the
 * first fold, -1 if none), status[B], nreject[B], hlast[B] (the step length the row holds at the end), zgoal[B][n] (may be NULL;
 * NaN unless REACHED).
 * One ROUND, for every row that is not finished; v is its evaluation point, y its last accepted point, t the unit tangent there, h the
 * step length, k the number of corrector updates of this step:
 *   1. evaluate at v, with e, h_theta and the moved value exactly as steps 1-3 of socp_tangent_batch on theta = fl(v_n wtheta):
 *      F0 = F(v_z; theta), F1 = F(v_z; theta + h_theta) from ONE residual launch of 2B rows with expanded block rows;
 *      g_i = fl(fl(fl(F1_i - F0_i) / h_theta) wtheta);  J exactly as step 4 of socp_tangent_batch at (v_z, F0) under the SAME expanded
 *      blocks (so the base row's theta is the state's, not the caller's)
 *   2. rn = max_i |F0_i|; a NaN when an entry is one
 *   3. the bordered matrix M, (n+1) x (n+1): rows 0 .. n-1 = [J | g], row n = t^T (in a row's first round: dir e_{n+1}^T).  ONE
 *      elimination serves every case: step 6 of socp_tangent_batch with size n + 1 and K = 1; only the right-hand side differs
 *   4. start (the row's first round; v = (z, lambda_0)): rn not finite: BAD_START, nothing recorded.  Otherwise M tau = e_{n+1},
 *        s = sum tau_i^2 (sequential, i = 0 .. n, from +0.0), t = tau / sqrt(s).  Point 0 is recorded (y = v, rnorm = rn, no acceptance
 *        test).  info != 0, or s zero or not finite: SINGULAR, ttheta[0] stays NaN.  Otherwise h = h0 and predict.
 *      accept (rn <= ftol): y <- v; t' from M tau = e_{n+1} as above -- row n is the OLD t, so t'.t > 0: the orientation is carried
 *        along the branch and through folds.  The point is recorded.  Singular: SINGULAR, its ttheta stays NaN, nothing below happens.
 *        fold: signbit(t'_n) != signbit(t_n): nfold += 1, ifold = this point's index if it was -1.
 *        growth: k <= kfast: h = min(fl(h grow), hmax).
 *        goal (have_goal): a = theta_prev - goal, b = theta_now - goal (the recorded thetas); REACHED if b == 0, or a != 0 and
 *        (a < 0) != (b < 0); then zgoal = z_prev + w (z_now - z_prev), w = (goal - theta_prev) / (theta_now - theta_prev).
 *        Otherwise count == cap: FULL.  Otherwise t <- t' and predict.
 *      reject (rn not finite, or k == max_corr): nreject += 1, h <- h / 2; h < hmin: STEP_TOO_SMALL; y, t and the records stay;
 *        otherwise predict.
 *      correct (otherwise): M delta = (-F0, 0); dn = sqrt(sum delta_i^2), the same sequential sum; info != 0 or !(dn <= h): handled as
 *        reject (the distance guard that keeps Newton from jumping to another branch).  Otherwise v <- v + delta, k += 1.  Every delta
 *        is orthogonal to t: v stays in the hyperplane through the predictor.
 *      predict: v_i = y_i + fl(h t_i), k = 0.
 *   5. a finished row (status != 0) changes nothing any more; after `rounds` rounds an unfinished row is RUNNING.
 * In reference-order contexts every operation above is one IEEE rounding (no contraction, IEEE division and square root): the call
 * is a fixed sequence of roundings, independent of how rows are batched and of what the other rows do (tests/branch_reference.py
 * restates it in numpy).  SOCP_VARIANT_LANE_FAST contexts may fuse products and sums; as built they do so only in the model's own
 * launches (residual, Jacobian): the steps above -- the bordered matrix, the elimination, the state machine -- run in reference order in
 * both flavours, so a throughput path deviates from the reference-order one by what its residual and Jacobian deviate, and no more.  Finished rows are still integrated (their
 * results are not used): no output depends on it.
 * All models, plugins included, both variants, both integrators: only the launch-table entries residual, fdjac and var_jacobian are
 * used.  A Goddard smooth-law promise covers the moved blocks unless the direction is mu2 itself.
 * socp_branch_work_bytes: the bytes of d_work for B rows (0 without a problem or for B < 0): the block rows, unknowns and residual
 * rows of the 2B launched rows, J[B][n*n], M[B][(n+1)^2], the right-hand sides, the row state, and on a model with variational
 * equations what socp_var_jacobian_multi_dev integrates in.
 * Launches of the _dev form, per round: expand; ONE residual launch of 2B rows; the Jacobian (1 launch, variational: 3); assemble; the
 * elimination; update.  socp_ctx_counters advances per round by 2 B M trajectories plus the Jacobian's (np T of the dedup list, or
 * B M) and by 6 launches (variational: 8).
 * SOCP_ERR_ARG: no problem set, B < 0, a bad kind or index, jac outside 0 .. 1, a NULL options pointer, wtheta <= 0 or not finite, dir
 * not +-1, !(0 < hmin <= h0 <= hmax), grow < 1 (or NaN), max_corr < 1, kfast < 0, !(ftol > 0), cap < 2, rounds < 1, a NULL required
 * pointer with B > 0 (all but zgoal), work_bytes below socp_branch_work_bytes, _blocks with params and param_stride != nparams + 2;
 * SOCP_ERR_UNSUPPORTED: jac == 1 without variational equations, n + 1 beyond the elimination's bound;  B == 0: SOCP_OK without a
 * launch.  An error writes nothing and leaves the context unchanged.
 * The _dev form takes device pointers (the direction and the options are host values that travel as kernel arguments), only
 * enqueues on the context's stream -- exactly `rounds` rounds, no host decision between them -- and neither allocates, copies nor
 * synchronises.  The host forms stage through that stream and the context's grow-only buffers; they may stop early: the update
 * kernel leaves the number of unfinished rows in a word of the workspace, the host reads it back every 8 rounds and stops when it is
 * 0 (the counters then advance by the rounds that ran).  Their results equal the _dev form's with all rounds, since a finished row
 * changes nothing.  _blocks: per-row blocks like socp_residual_batch_blocks; the context's own blocks are restored afterwards.
 * Not covered: no change to socp_chains_solve; no branch switching at bifurcations; no resuming of a RUNNING row other than calling
 * again from its last point; one GPU. */
size_t socp_branch_work_bytes(const socp_ctx *ctx, int B);
int socp_branch_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int dir_kind, int dir_index, const socp_branch_options *opt,
                          void *d_work, size_t work_bytes, double *d_Y, double *d_ttheta, double *d_rnorm, int *d_count, int *d_nfold,
                          int *d_ifold, int *d_status, int *d_nreject, double *d_hlast, double *d_zgoal);
int socp_branch_batch(socp_ctx *ctx, int B, const double *Z, int dir_kind, int dir_index, const socp_branch_options *opt,
                      double *Y, double *ttheta, double *rnorm, int *count, int *nfold, int *ifold, int *status, int *nreject,
                      double *hlast, double *zgoal);
int socp_branch_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                             const double *xnode, int dir_kind, int dir_index, const socp_branch_options *opt,
                             double *Y, double *ttheta, double *rnorm, int *count, int *nfold, int *ifold, int *status, int *nreject,
                             double *hlast, double *zgoal);

/* Polishing a table of roots: damped Newton iteration on B rows at once, in lock step, with the exact shooting Jacobian.  [ext] A
 * sweep ends in roots hybrd stopped on at xtol with a Broyden-updated, differenced Jacobian; this call drives them to rounding level
 * and says per row how far it got -- the damped Newton corrector of the indirect-methods tools.  It stands beside socp_chains_solve
 * and changes none of its iterates.  It is the first consumer of socp_exact_jacobian_batch (jac = 2). */
typedef struct socp_newton_options {
    int jac;          /* 0 forward difference, 1 variational, 2 exact (socp_exact_jacobian_batch) */
    double epsfcn;    /* jac == 0 only: the step rule of socp_fd_jacobian_multi_dev */
    double ftol;      /* > 0: CONVERGED when ||F||inf <= ftol */
    double xtol;      /* >= 0: SMALL_STEP when the step taken is <= xtol ||z||inf; 0 disables */
    int trials;       /* 1 .. 8: step lengths 1, 1/2, ... 2^-(trials-1) tried per round */
    int rounds;       /* >= 1 */
} socp_newton_options;
#define SOCP_NEWTON_RUNNING    0   /* the rounds ran out; Zout is the last accepted point, call again from it to go on */
#define SOCP_NEWTON_CONVERGED  1   /* ||F||inf <= ftol */
#define SOCP_NEWTON_SMALL_STEP 2   /* the step taken was <= xtol ||z||inf */
#define SOCP_NEWTON_STALLED    3   /* no trial step lowered ||F||inf enough: as good as this arithmetic (or this Jacobian) gets */
#define SOCP_NEWTON_SINGULAR   4   /* the elimination found no pivot, or its solution is not finite */
#define SOCP_NEWTON_BAD_START  5   /* F at the start is not finite */
/* Z[B][n] -> per row: Zout[B][n] (the accepted point y), Fout[B][n] (F0 = F(y); may be NULL), rnorm[B] (rn = ||F0||inf), dnorm[B]
 * (||delta||inf of the FULL Newton step of the last system solved for the row: an a-posteriori error estimate of the point it was
 * solved at; NaN while no system was solved, and for SINGULAR and BAD_START), iters[B] (accepted steps), nhalf[B] (the sum of the
 * accepted steps' k), status[B], rhist[B][rounds + 1] (may be NULL; rn after 0, 1, ... accepted steps, unused slots NaN).
 * All norms are max-norms: max_i |x_i|, a NaN when an entry is one (an infinite entry makes it infinite).  They are maxima, so no
 * reduction order enters a result.  Per row the state is y, F0, rn and the counters.
 * Start: F0 = F(Z) from ONE residual launch of the B rows in the context's flavour, each row with its blocks; rhist[b][0] = rn.
 *   rn not finite: BAD_START, Zout = Z, dnorm NaN.  rn <= ftol: CONVERGED with iters = 0.
 * One ROUND, for every row that is not finished:
 *   1. J at (y, F0): jac 0: socp_fd_jacobian_multi_dev with epsfcn and dedup on (step 4 of socp_tangent_batch); jac 1: the variational
 *      Jacobian; jac 2: the exact Jacobian (socp_exact_jacobian_batch; its own F output is not requested -- F0 is always the residual
 *      launch's, so one flavour's merit function is measured by one kernel)
 *   2. J delta = -F0 (the negation is exact): step 6 of socp_tangent_batch with K = 1, in reference order in both flavours.
 *      dn = max_i |delta_i|.  info != 0: SINGULAR, y stays, dnorm NaN.  Otherwise dnorm = dn
 *   3. the trial points, k = 0 .. trials - 1: s_k = 2^-k, t_k,i = y_i + fl(s_k delta_i)
 *   4. F_k = F(t_k) from ONE residual launch of (rows x trials) rows, the row's block rows replicated where rows have their own
 *   5. c_k = 1 - s_k / 4 (exact).  The first k with max_i |F_k,i| < fl(c_k rn) wins; a NaN never passes.  None passes: STALLED, y stays
 *      (with an ftol below rounding level this is how a row says "as good as this arithmetic gets").  Otherwise y <- t_k, F0 <- F_k,
 *      rn <- max_i |F_k,i|, iters += 1, nhalf += k, rhist[iters] = rn
 *   6. rn <= ftol: CONVERGED.  Else if xtol > 0 and fl(s_k dn) <= fl(xtol max_i |y_i|) (the new y): SMALL_STEP
 *   7. a finished row (status != 0) changes nothing any more; after `rounds` rounds an unfinished row is RUNNING.
 * In reference-order contexts every operation above is one IEEE rounding (no contraction, IEEE division): the call is a fixed
 * sequence of roundings per row, independent of the other rows, of B and of which rows are still running
 * (tests/newton_reference.py restates it in numpy).  SOCP_VARIANT_LANE_FAST contexts differ through the model's own launches only
 * (residual, Jacobian); the exact Jacobian is the same object in both flavours.
 * Finished rows cost nothing: a round begins with a stable compaction of the unfinished rows, in ascending row order, into a list
 * (three launches -- count, scan, scatter -- none of which waits on another workgroup); a gather copies y, F0, -F0 and the rows' own
 * block rows into compact slots; the Jacobian, the elimination, the trial build and the trial residual run on compact slots, and the
 * update scatters back through the list.  Slots at or beyond the live count keep what an earlier round (or the start, which sets
 * slot b to row b) left there: valid rows no output depends on.
 * The _dev form takes device pointers (the options are host values that travel as kernel arguments), launches all B slots in every
 * round, enqueues exactly `rounds` rounds on the context's stream with no host decision, and neither allocates, copies nor
 * synchronises.  The host forms stage through that stream and the context's grow-only buffers; after every compaction they read the
 * live count back (one word), run the round on that many slots and stop at 0.  Both give identical bits.  _blocks: per-row blocks
 * like socp_residual_batch_blocks; the context's own blocks are restored afterwards.
 * socp_newton_work_bytes: the bytes of d_work for B rows and opt->trials (0 without a problem, for B < 0, a NULL opt or trials
 * outside 1 .. 8): F0, the compact slots (points, residuals, right-hand sides, block rows, J[B][n*n]), the B trials trial rows
 * (points, residuals, block rows), the list, and on a model with variational equations what socp_var_jacobian_multi_dev integrates in.
 * Launches: the start is 2 (residual, state).  A round on s slots is the compaction (3), the gather, the Jacobian (jac 0: 1, jac 1: 3,
 * jac 2: 1), the elimination, the trial build, ONE residual launch, the update: 9 launches (jac 1: 11).  socp_ctx_counters advances
 * by B M trajectories and 2 launches for the start and, per round on s slots, by the Jacobian's trajectories (jac 0: s T of the dedup
 * list, jac 1: s M, jac 2: s M (S + 1)) plus s trials M, and by 9 (11) launches; s = B in the _dev form, the live count in the host
 * forms, whose last compaction (live count 0) adds 3 launches and nothing else.
 * jac 0 / 1: all models, plugins included, both variants, both integrators (entries residual, fdjac, var_jacobian); jac 2 adds the
 * entry exact_jacobian and its limits.  No new launch-table entry.
 * SOCP_ERR_ARG: no problem set, B < 0, a NULL options pointer, jac outside 0 .. 2, trials outside 1 .. 8, rounds < 1, !(ftol > 0),
 * xtol < 0 or NaN, a NULL required pointer with B > 0 (all but Fout and rhist), work_bytes below socp_newton_work_bytes, _blocks with
 * params and param_stride != nparams + 2;  SOCP_ERR_UNSUPPORTED: jac == 1 without variational equations, jac == 2 where
 * socp_exact_jacobian_batch refuses (no entry, SOCP_INT_DOPRI5, a FREE interior state component), n beyond the elimination's bound;
 * B == 0: SOCP_OK without a launch.  An error writes nothing and leaves the context unchanged.
 * Not covered: no trust region (the only globalisation is the halving above); it does not replace hybrd -- it polishes rows that are
 * already near a root; no change to socp_chains_solve; a state-dependent kink differentiates the branch taken; with jac = 2 Goddard's
 * mu2 = 0 switching times are not differentiated (socp_exact_jacobian_batch); one GPU. */
size_t socp_newton_work_bytes(const socp_ctx *ctx, int B, const socp_newton_options *opt);
int socp_newton_batch_dev(socp_ctx *ctx, int B, const double *d_Z, const socp_newton_options *opt, void *d_work, size_t work_bytes,
                          double *d_Zout, double *d_Fout, double *d_rnorm, double *d_dnorm, int *d_iters, int *d_nhalf, int *d_status,
                          double *d_rhist);
int socp_newton_batch(socp_ctx *ctx, int B, const double *Z, const socp_newton_options *opt, double *Zout, double *Fout,
                      double *rnorm, double *dnorm, int *iters, int *nhalf, int *status, double *rhist);
int socp_newton_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                             const double *xnode, const socp_newton_options *opt, double *Zout, double *Fout, double *rnorm,
                             double *dnorm, int *iters, int *nhalf, int *status, double *rhist);

/* EXACT parameter sensitivities of a whole batch of converged unknown vectors: dz/dtheta from J dz = -dF/dtheta, where BOTH sides are
 * exact for the discrete flow -- J is socp_exact_jacobian_batch's, dF/dtheta comes from dual numbers carried through the residual's own
 * RK4 steps and rows with the PARAMETER as the seeded quantity.  [ext] socp_tangent_batch differences both sides; on the nominal Goddard
 * extremal its predictor z + dtheta dz then carries a first-order error (README).  Directions (dir_kind[K], dir_index[K]: HOST arrays,
 * read before the call returns; 1 <= K <= 16) with the kinds and ranges of socp_tangent_batch, except that a SOCP_DIR_PARAM index must
 * be < nparams: the slots nparams and nparams + 1 (sw0, sw1) are refused, the discrete flow is piecewise constant in them and a zero
 * would mislead.  Z[B][n] -> dZ[B][K][n], info[B], Gp[B][K][n] (may be NULL: G = dF/dtheta_k).  SETUP, timeline, switching times and
 * per-row blocks are those of socp_residual_batch; DUAL NUMBERS as in socp_fields_batch.  Per row b:
 *   1. J: exactly what socp_exact_jacobian_batch_dev stores for the row (the same launch, the same bits; its F is not requested).
 *   2. G[b][k][:], zero-filled first on the call's stream; every entry then has exactly one writer: the lane of the segment that owns
 *      the row in the ROWS paragraph of socp_exact_jacobian_batch.  One lane per (row, segment, integrating direction); the directions
 *      of one kind of one (row, segment) are neighbouring lanes, 64 / (their number) groups per wave; one launch per kind present.
 *      SOCP_DIR_PARAM, index q.  The lane reads the row's packed block as dual numbers: every one of the nparams slots is (p_i, +0.0),
 *      the addressed one (p_q, 1.0).  A parameter takes part by the full dual x dual rules, its zero terms computed; literals, t, N,
 *      the switching times and the step stay plain, as in socp_fields_batch.  The start state is (z, +0.0).  The step loop and the RK4
 *      step are socp_fields_batch's (plain t and h).  The rows are segment_residual on duals with the dual parameters: row ft_row[0]
 *      (t0 FREE): hamiltonian_t(t1, X) on the start state of segment 0; on the END state X of segment i < M - 1: row ft_row[i + 1]
 *      (that time FREE): switching_fn_t(t2, X, (Xp, +0.0)) -- the -H(Xp) term of a model with kSwitchingReadsXp sees the parameter in
 *      this same evaluation -- and the derivative parts of X[j] at row S (i + 1) + j and, unless component j is FIXED, of X[j + d] at
 *      row S (i + 1) + d + j; on the END state of segment M - 1: X[j + d] where component j of node M is FREE, else X[j], at row d + j,
 *      and hamiltonian_t(t2, X) at row ft_row[M] (tf FREE).  (x - c).d is x.d for a plain c, so the subtractions of xd and Xp are not
 *      formed.  The rows j < d of node 0 and the second row of a FIXED interior component read no parameter: nothing is stored.
 *      Comparisons read value parts (mu2 > 0, singularControl < 0, the u_max saturation, covid19's bounds and Imax): a kink
 *      differentiates the branch taken, and a control clamped to a bound IS that parameter, (u_max, its derivative part).  The value
 *      parts are the reference-order residual's, bit for bit.
 *      SOCP_DIR_TIME, node f.  Where node f is FIXED (a junction of the timeline whose time is the table's), the lane of segment i
 *      runs the LENGTH column of socp_exact_jacobian_batch unchanged -- t2 = (t2, 1.0), dual step, plain parameters -- and stores
 *      w (d row / d L), one product, at (row, k) for the END-state rows above, w = c(i + 1, f) - c(i, f) the free-time columns' weight
 *      with FIXED in place of FREE; nothing is stored when w == 0.0.  A FREE or CONTINUOUS node's table time is never read: G = +0.0,
 *      no lane is launched, and the direction is not refused (as in socp_tangent_batch).  What socp_exact_jacobian_batch does not
 *      differentiate (an explicit t, the mu2 = 0 comparisons against sw0 / sw1) is not differentiated here either.
 *      SOCP_DIR_XNODE, (j, c).  No integration.  -1.0 at every row that reads xd[j][c]: row c where component c of node 0 is not
 *      FREE, row d + c where component c of node M is not FREE, rows S j + c and S j + d + c of a FIXED interior component; otherwise
 *      nothing.
 *   3. rhs = -G entry by entry (exact; a +0.0 becomes -0.0); dZ[b][k] = the solution of J x = rhs[k] by step 6 of socp_tangent_batch,
 *      run in REFERENCE ORDER in both flavours (as socp_newton_batch and socp_branch_batch do); info[b] as there.
 * ONE OBJECT, NO CONTRACTION: a throughput-flavour context returns the same bits.  tests/sensitivity_reference.py restates the
 * definition; the tests compare whole buffers to it.
 * socp_ctx_has_sensitivity: 1 when the model's launch table has the entry -- everything socp_ctx_has_exact_jacobian asks for, and
 * rhs_t / hamiltonian_t / switching_fn_t generic in the parameter view (Goddard in both laws, the double integrator, covid19, a plugin
 * that writes its traits so: tests/plugin/osc1d_sensitivity_plugin.hip) -- else 0.
 * socp_sensitivity_work_bytes: the bytes of d_work for (B, K) on this context's problem (0 for arguments the call would refuse):
 * J[B][n*n] and G[B][K][n].
 * Launches of the _dev form: the exact Jacobian (its zero-fill and ONE launch); G's zero-fill and one launch per integrating kind
 * present (PARAM; TIME on a FIXED node); the finish (XNODE stores, rhs = -G); the elimination.  socp_ctx_counters advances by
 * B M (S + 1) trajectories plus B M per integrating direction, and by 3 launches plus one per integrating kind present.
 * SOCP_ERR_ARG: socp_tangent_batch's argument errors (no problem set, B < 0, K outside 1 .. 16, a kind outside 0 .. 2 or an index
 * outside its range, a NULL required pointer, work_bytes below socp_sensitivity_work_bytes, a wrong parameter stride in _blocks), and
 * a SOCP_DIR_PARAM index >= nparams.  SOCP_ERR_UNSUPPORTED (the message says which): the context's integrator is SOCP_INT_DOPRI5, the
 * launch table has no sensitivity entry (the interceptor, vtolUAV, a model without the generic traits, with a switching_state hook or
 * custom final rows; a plugin built before launch-table ABI 15 is refused when it registers: rebuild it), a FREE state component on an
 * interior node, n beyond the elimination's bound.  B == 0: SOCP_OK without a launch.  An error writes nothing and leaves the context
 * and its counters unchanged.
 * The _dev form takes device pointers (the directions stay host arrays), only enqueues on the context's stream and neither allocates,
 * copies nor synchronises.  The host forms stage through that stream and the context's grow-only buffers; _blocks: per-row blocks like
 * socp_residual_batch_blocks, the context's own blocks restored afterwards.
 * Not covered: jac = 2 inside socp_tangent_batch / socp_singular_batch / socp_branch_batch, a predictor inside socp_chains_solve, the
 * adaptive integrator, the interceptor, vtolUAV, derivatives in sw0 / sw1, second derivatives, more than one GPU. */
int socp_ctx_has_sensitivity(const socp_ctx *ctx);      /* 1 / 0; SOCP_ERR_ARG for a NULL context */
size_t socp_sensitivity_work_bytes(const socp_ctx *ctx, int B, int K);
int socp_sensitivity_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int K, const int *dir_kind, const int *dir_index, void *d_work,
                               size_t work_bytes, double *d_dZ, int *d_info, double *d_Gp /* or NULL */);
int socp_sensitivity_batch(socp_ctx *ctx, int B, const double *Z, int K, const int *dir_kind, const int *dir_index, double *dZ,
                           int *info, double *Gp);
int socp_sensitivity_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                                  const double *xnode, int K, const int *dir_kind, const int *dir_index, double *dZ, int *info,
                                  double *Gp);

/* NEIGHBOURING-EXTREMAL FEEDBACK GAINS along every row of a batch (the backward sweep of Bryson-Ho / Breakwell-Speyer-Bryson on the
 * DISCRETE flow): for a measured state deviation dx at the sample time t_q, the costate correction dp = K(t_q) dx that keeps the final
 * boundary rows satisfied to first order.  The caller applies the model's own control law at (x, p_nom + K dx), saturations
 * included.  socp_tangent_batch / socp_sensitivity_batch with SOCP_DIR_XNODE directions give dp0/dx0, the gain at the first instant
 * only; this call gives it along the flight.  [ext] The reference has no such call.
 * Z[B][n] -> tq[B][M][cap], Kp[B][M][cap][d*d], info[B][M][cap], count[B][M] and, each unless NULL, Xq[B][M][cap][s],
 * Wq[B][M][cap][d*s], Psi[B][M][cap][s*s];  s = 2d.
 * SETUP, timeline, switching times and per-row blocks are those of socp_fields_batch; every node time is FIXED (or interpolated
 * between FIXED ones), every interior node CONTINUOUS.  DUAL NUMBERS as in socp_fields_batch.  Fixed-step integrator only.
 * SAMPLES.  Segment i of row b takes the nst steps of the residual's loop (dt = (t2 - t1) / step_nbr; t accumulated by t += dt; the last
 *   step clamped).  Q = max(1, ceil(nst / stride)), count[b][i] = Q.  Sample q sits at the START of step q stride: tq[b][i][q] is the
 *   loop's own t there, Xq[b][i][q][s] the value state there -- bit for bit the rows socp_trace_batch keeps with the same stride in the
 *   reference-order flavour.  Sample 0 is the segment's start node; the segment's end is not a sample.
 * BLOCKS.  Psi_q = dX(after step min((q + 1) stride, nst)) / dX(sample q), s x s, stored ROW-major (row r of X, column c: the layout
 *   of Phi): column c is carried as the derivative parts of a state that takes the residual's RK4 steps on dual numbers exactly as a
 *   column of socp_fields_batch does (association order of odeTools.cpp:89-98, t and the step plain).  At every sample each column
 *   RE-SEEDS: its state becomes (X[j].v, j == c ? 1.0 : +0.0).  The value parts are never touched: the value trajectory is the
 *   reference-order residual's, bit for bit.  A segment that takes no step has Q = 1 and Psi_0 = I.  With one block per segment
 *   (stride >= nst) Psi_0 equals Phi of socp_fields_batch(cols = SOCP_FIELDS_ALL) bit for bit.
 * BACKWARD SWEEP.  E is the d x s selector of the final boundary rows: row j is e_{d+j} when final component j is FREE, else e_j.
 *   W after the last block is E; then downward over (i, q), across segment boundaries, W_{i,q} = W_next Psi_{i,q}:
 *     W'[r][j] = sum_m W[r][m] Psi[m][j],  m ascending, every product rounded, the sum sequential and started from the first product,
 *     nothing contracted.
 *   Wq[b][i][q] = W_{i,q}, ROW-major (row r, column j): the sensitivity of the terminal rows to the state at the sample, a
 *   miss-distance table in its own right.
 * GAIN.  W_{i,q} = [A_x | A_p].  Kp[b][i][q] is d x d COLUMN-major, entry (r, c) at [c d + r] = dp_r/dx_c, the solution of
 *   A_p K = -A_x by the elimination of socp_linsolve_batch_dev in REFERENCE ORDER in both flavours (as socp_newton_batch and
 *   socp_sensitivity_batch use it); info[b][i][q] is that elimination's code (0: solved; k + 1: no pivot in step k, Kp = NaN; d + 1: a
 *   solution entry is not finite).  A singular A_p means that no costate correction reaches the target from there -- on the nominal
 *   Goddard flight, every sample after the thrust has gone off for good.
 * SLOTS q >= count keep what the buffers held, in every output.  A segment whose loop counted more blocks than cap (rounding gave
 *   it a step beyond step_nbr) stores the first cap and leaves the chain of products incomplete: the row's W starts from NaN and
 *   every sample of the row reports a failed elimination.
 * WORKSPACE.  The elimination's matrices (B M cap d^2 doubles) and, when Psi is NULL, the blocks (B M cap s^2 8 bytes) live in a
 *   grow-only workspace arena of the context: the first use and every growth is a hipMalloc, which synchronises the device.
 * ONE OBJECT, NO CONTRACTION, as socp_fields_batch: a throughput-flavour context returns the same bits.
 * WHAT IT IS NOT.  The gain of the continuous problem (it is exact for the DISCRETE flow, to rounding, with no step size); the far
 *   side of a kink (the branch taken is differentiated); a control gain (the caller applies the control law); more than one GPU.
 * socp_ctx_has_gain: 1 when the model's launch table has the entry -- the rhs_t trait, no switching_state hook, no custom final rows,
 * no ComputeTraj of its own (Goddard in both laws, the double integrator, covid19, every plugin with rhs_t, FromHamiltonianExact ones
 * included) -- else 0; SOCP_ERR_ARG for a NULL context.
 * SOCP_ERR_ARG: no problem set, B < 0, stride < 1, cap < ceil(step_nbr / stride), a NULL required pointer (Z, tq, Kp, info, count) with
 * B > 0, _blocks with params and param_stride != nparams + 2; B == 0: SOCP_OK without a launch.  SOCP_ERR_UNSUPPORTED (the message
 * says which): the context's integrator is SOCP_INT_DOPRI5; the model's launch table has no gain entry (the interceptor, vtolUAV,
 * lqr1d; a plugin built before launch-table ABI 18 is refused when it registers: rebuild it); a problem with any FREE time, interior
 * or final; an interior node with a FIXED or FREE component -- those structures need a bordered sweep.  An error writes nothing,
 * launches nothing and leaves the counters unchanged.
 * Three launches (the blocks, the backward sweep, the elimination); socp_ctx_counters advances by B M s trajectories.  The _dev, host
 * and _blocks forms as for socp_fields_batch; in the host forms every output travels both ways. */
int socp_ctx_has_gain(const socp_ctx *ctx);             /* 1 / 0; SOCP_ERR_ARG for a NULL context */
int socp_gain_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int stride, int cap, double *d_tq, double *d_Kp, int *d_info,
                        int *d_count, double *d_Xq /* or NULL */, double *d_Wq /* or NULL */, double *d_Psi /* or NULL */);
int socp_gain_batch(socp_ctx *ctx, int B, const double *Z, int stride, int cap, double *tq, double *Kp, int *info, int *count,
                    double *Xq, double *Wq, double *Psi);
int socp_gain_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                           const double *xnode, int stride, int cap, double *tq, double *Kp, int *info, int *count, double *Xq,
                           double *Wq, double *Psi);

/* NEIGHBOURING-EXTREMAL FEEDBACK GAINS WITH A FREE FINAL TIME (Bryson-Ho 6, free terminal time, on the DISCRETE flow): for a measured
 * state deviation dx at sample q, the costate correction dp = K_p dx AND the correction dt_f = k_t . dx of the final time that keep
 * the d final boundary rows and the transversality row H(t_f, X_f) = 0 satisfied to first order -- time-to-go feedback.
 * socp_gain_batch refuses a free time; this call is the bordered sweep it names.  [ext] The reference has no such call.
 * Z[B][n] -> tq[B][M][cap], Ke[B][M][cap][(d+1)*d], info[B][M][cap], count[B][M] and, each unless NULL, Xq[B][M][cap][s],
 * Wq[B][M][cap][(d+1)*(s+1)], Psi[B][M][cap][s*s], Len[B][M][cap][s];  s = 2d.
 * STRUCTURE.  Node M's time is FREE (the last unknown of a row); every other time is FIXED or interpolated; every interior node has
 *   all components CONTINUOUS; fixed-step integrator.  SETUP, switching times and per-row blocks as in socp_fields_batch.
 * SAMPLES, tq, Xq, count, cap and the slots >= count are exactly socp_gain_batch's; t2 of a segment comes from the row's own z
 *   through the timeline.
 * BLOCKS.  S + 1 columns per (row, segment): S state columns and the LENGTH column.  The loop is the exact Jacobian's dual loop
 *   (socp_exact_jacobian_batch), cut into blocks of `stride` steps:
 *     t2 = (t2, delta), delta = 1.0 in the length column and +0.0 in the others;  dt = (t2 - (t1, 0)) / step_nbr;  t = (t1, 0);
 *     while t.v < t2.v - dt.v / 2 (and the guard):  h = t.v + dt.v > t2.v ? t2 - t : dt;  X = rk4(t, X, h);  t = t + dt
 *   with t, dt and h dual numbers in EVERY column and h F the full dual product (dual x dual), the right-hand side given the value
 *   part of the stage time.  At a sample state column c re-seeds to (X[j].v, j == c ? 1.0 : +0.0) and the length column to
 *   (X[j].v, +0.0).  The derivative parts of t and dt are NOT re-seeded: the clamped last step t2 - t needs dt/dL.  The value parts
 *   are never touched.  Psi_q as in socp_gain_batch, row-major s x s -- as NUMBERS equal to socp_gain_batch's on the twin problem with
 *   t_f FIXED at the row's value (a dual step with a zero derivative part adds products with zero), not always as bits (-0.0).
 *   Len[b][i][q][r] = the length column's derivative part of component r after the block: dX(after the block)/dL with the state at
 *   the sample held.  A segment that takes no step has Q = 1, Psi_0 = I, l_0 = 0.  With one block per segment and M = 1, Psi_0 and l_0
 *   equal the state block and the t_f column (rows d .. 2d-1 through the selector) of socp_exact_jacobian_batch bit for bit.
 *   After the last block of segment M - 1 the state columns re-seed once more and hamiltonian_t is evaluated on them at (t2, X_f):
 *   grad H[c] is column c's derivative part (an explicit t is not differentiated).
 * BACKWARD SWEEP.  d + 1 rows: rows r < d start from socp_gain_batch's selector E, row d from grad H(X_f); the border entry wtau of
 *   every row starts from +0.0.  Downward over (i, q), across segment boundaries, two updates in this order:
 *     1. wtau' = wtau + w_i (sum_m W[m] l_q[m]):  m ascending, every product rounded, the sum sequential and started from the first
 *        product; then the product with w_i, then the addition.  w_i = c(i+1, M) - c(i, M), the weight the exact Jacobian gives the
 *        t_f column of segment i (c(j, M) = 1 for j == M, (double)(j - a) / (double)(b - a) for a node j interpolated between the
 *        junctions a and b = M, else 0).  When w_i == 0 the update is skipped.
 *     2. W' = W Psi_q, as in socp_gain_batch.
 *   Wq[b][i][q] is ROW-major (d+1) x (s+1): row r, its s state columns, then wtau.
 * GAIN.  W = [A_x | A_p], both (d+1) x d.  The (d+1) x (d+1) system [A_p | wtau] [K_p; k_t] = -A_x, d right-hand sides, by the
 *   elimination of socp_linsolve_batch_dev in REFERENCE ORDER in both flavours (n = d + 1, K = d).  Ke[b][i][q] is COLUMN-major with
 *   leading dimension d + 1: column c is (dp_0/dx_c .. dp_{d-1}/dx_c, dt_f/dx_c).  info is the elimination's code (0: solved; k + 1:
 *   no pivot in step k, Ke = NaN; d + 2: a solution entry is not finite).
 * MEANING.  dx is measured at the sample INDEX: the guidance clock is the normalised time of the timeline, not t.  The remaining
 *   steps of the row are re-timed with t_f + dt_f, so the remaining flight time changes by dt_f times the share of the timeline
 *   still to fly.  For an autonomous model K_p does not depend on that convention.  An explicit t and the mu2 = 0 comparisons are not
 *   differentiated, as everywhere.
 * WORKSPACE.  The bordered matrices (B M cap (d+1)^2 doubles), grad H (B s) and, when NULL, Psi and Len live in socp_gain_batch's
 *   grow-only arena.  ONE OBJECT, NO CONTRACTION: a throughput-flavour context returns the same bits.
 * socp_ctx_has_gain_free: 1 when the model's launch table has the entry -- socp_ctx_has_gain's condition and the hamiltonian_t trait
 * (Goddard in both laws, the double integrator, covid19, every plugin with both traits) -- else 0; SOCP_ERR_ARG for a NULL context.
 * SOCP_ERR_ARG: as for socp_gain_batch (required pointers: Z, tq, Ke, info, count).  SOCP_ERR_UNSUPPORTED (the message says which):
 * SOCP_INT_DOPRI5; no gain_free entry in the launch table (a plugin built before launch-table ABI 19 is refused when it registers);
 * node M's time not FREE (use socp_gain_batch); a free time on a node k < M; an interior node with a FIXED or FREE component; too many
 * states for the batched linear solve.  An error writes nothing, launches nothing and leaves the counters unchanged.
 * Three launches; socp_ctx_counters advances by B M (s + 1) trajectories.  The _dev, host and _blocks forms as for socp_gain_batch. */
int socp_ctx_has_gain_free(const socp_ctx *ctx);        /* 1 / 0; SOCP_ERR_ARG for a NULL context */
int socp_gain_free_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int stride, int cap, double *d_tq, double *d_Ke, int *d_info,
                             int *d_count, double *d_Xq /* or NULL */, double *d_Wq /* or NULL */, double *d_Psi /* or NULL */,
                             double *d_Len /* or NULL */);
int socp_gain_free_batch(socp_ctx *ctx, int B, const double *Z, int stride, int cap, double *tq, double *Ke, int *info, int *count,
                         double *Xq, double *Wq, double *Psi, double *Len);
int socp_gain_free_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                                const double *xnode, int stride, int cap, double *tq, double *Ke, int *info, int *count, double *Xq,
                                double *Wq, double *Psi, double *Len);

/* CLOSED-LOOP FLIGHT UNDER THE SAMPLED NEIGHBOURING-EXTREMAL LAW: K dispersed cases per row of a batch, each flown from the first sample
 * to the last with the costate RESET to p_nom + K_p dx at the samples of socp_gain_batch / socp_gain_free_batch -- what the two gain
 * calls leave to the caller ("the caller applies the model's own control law at (x, p_nom + K dx), saturations included"), for a whole
 * Monte-Carlo set in ONE launch.  The model's rhs forms its control from (x, p) inside, saturations included.  [ext] The reference has
 * no such call.
 * STRUCTURE.  Exactly the two the gain calls accept, and the context's problem decides which tables are expected:
 *   every time FIXED or interpolated, interior nodes CONTINUOUS: Kg is socp_gain_batch's Kp, ldk = d;
 *   node M's time FREE (other times FIXED or interpolated, interior nodes CONTINUOUS): Kg is socp_gain_free_batch's Ke, ldk = d + 1,
 *   column c = (dp_0/dx_c .. dp_{d-1}/dx_c, dt_f/dx_c).
 *   Fixed-step integrator only.  SETUP, switching times and per-row blocks as in socp_gain_batch.
 * INPUTS.  Z[B][n], the nominal rows; stride, cap and Xq[B][M][cap][s], Kg[B][M][cap][ldk*d], info[B][M][cap], count[B][M] exactly as the
 *   gain call with the same stride and cap left them; K >= 1 cases per row; dX0[B][K][d], the state deviation at the first sample;
 *   every >= 0.  The tables are INPUTS, never written.  The caller may DISABLE samples by writing a nonzero info: a cut-off before the
 *   gains blow up near the target is done that way.
 * START.  Case (b, k) starts segment 0 from x_c = z[c] + dX0[b][k][c] (one addition per component) and p = z[d .. 2d).
 * LOOP.  Segment after segment; across an interior node the flight goes on FROM ITS OWN STATE (it does not restart from z).  In segment i
 *   with t1, t2 from the timeline (the final time in force in place of z[n-1] when it is FREE):
 *     dt = (t2 - t1) / step_nbr;  t = t1;  k = 0 (the steps this segment has taken);  q = 0
 *     act = t < t2 - dt / 2  &&  k < step_nbr + 8                      (the residual's condition and guard)
 *     repeat:  SAMPLE q (below; it may re-time t1, t2, dt, t and then re-evaluates act)
 *              up to `stride` times while act:  h = t + dt > t2 ? t2 - t : dt;  X = rk4(t, X, h);  t = t + dt;  k = k + 1;  act as above
 *              q = q + 1
 *     while act
 *   rk4 is the residual's step on the full 2d state (Lane::rk4 in the context's flavour).  A segment that takes no step has sample 0.
 * SAMPLE q of segment i, the start of step q stride.  g = the row-global sample index, counted over the flight's own samples in flight
 *   order, sample (0, 0) being 0.  The sample is DUE when every > 0 and g is a multiple of `every`.  A due sample with a table slot
 *   (q < min(count[b][i], cap)) forms dx_c = x_c - Xq[b][i][q][c] and updates dxmax = |dx_c| > dxmax ? |dx_c| : dxmax, c ascending,
 *   from +0.0 (strict: a NaN never displaces a value, as in socp_extrema_batch).  When moreover info[b][i][q] == 0 the correction is
 *   APPLIED (nupd + 1); every other due sample leaves the costate flowing (nskip + 1).  The correction:
 *     p_r = Xq[b][i][q][d + r] + (Kg[r] dx_0 + Kg[ldk + r] dx_1 + ... + Kg[(d-1) ldk + r] dx_{d-1}),  r = 0 .. d-1:
 *     c ascending, every product rounded, the sum sequential and started from the first product, then the ONE addition to the nominal
 *     costate (reference order: nothing contracted; the throughput flavour contracts).  The costate is RESET, not incremented.
 *   FREE final time, at an applied correction: tf' = z[n-1] + (Kg[d] dx_0 + ... + Kg[(d-1) ldk + d] dx_{d-1}), the same sum rule.  Only
 *     when tf' != the final time in force:  it becomes tf'; t1', t2' of segment i and the switching times are re-evaluated from the
 *     timeline with tf' as the last unknown (later segments read it when they start);  dt = (t2' - t1') / step_nbr;
 *     t = t1' + (double)k dt;  act is re-evaluated.  Samples stay tied to the step INDEX (socp_gain_free_batch, MEANING).
 *   Then Xs[b][k][i][q] = the state AFTER the correction, when the slot exists (q < min(count, cap)).
 *   every = 0 is the open-loop flight; an `every` beyond the number of samples corrects once, at the first sample: dp0/dx0 alone.
 *   With dX0 = 0 every dx is +0.0, p_nom + (a sum of zeros) is p_nom and tf' is z[n-1]: the flight is the nominal one bit for bit.
 * OUTPUTS per case.  Xf[B][K][s]: the state as the last segment leaves it.  miss[B][K][d] ([d + 1] with a FREE final time): row j is
 *   p_j(t_f) when final component j is FREE, else x_j(t_f) - xnode[M][j] -- the gain selector's rows as the residual forms them -- and
 *   with a FREE final time row d = hamiltonian(t2 of the last segment, X_f).  nupd[B][K], nskip[B][K] (int32).  Each unless NULL:
 *   tf[B][K], t2 of the last segment as in force at the end; dxmax[B][K]; Xs[B][K][M][cap][s], slots >= min(count, cap) keep what the
 *   buffer held.
 * FLAVOURS.  UNLIKE the gain calls each flavour flies its own arithmetic: a reference-order context the reference-order residual's
 *   steps (every output is tests/guide_reference.py's bit for bit), a throughput context the throughput residual's, at its speed.
 *   The double integrator is one text in both flavours and flies the reference-order arithmetic in both.
 *   The tables are the gain calls' and hold the REFERENCE-order nominal states in both flavours: a throughput flight sees the flavours'
 *   own deviation (rounding level) as part of dx and corrects it like any other.
 * socp_ctx_has_guide: 1 when the model's launch table has the entry -- rhs, no switching_state hook, no custom final rows, no
 * ComputeTraj of its own (rhs_t is not needed) -- else 0; SOCP_ERR_ARG for a NULL context.  The call itself also needs the gain entry
 * of the structure at hand (socp_ctx_has_gain / socp_ctx_has_gain_free).
 * SOCP_ERR_ARG: no problem set, K < 1, every < 0, B < 0, stride < 1, cap < ceil(step_nbr / stride), a NULL required pointer (Z, Xq, Kg,
 * info, count, dX0, Xf, miss, nupd, nskip) with B > 0, _blocks with params and param_stride != nparams + 2; B == 0: SOCP_OK without a
 * launch.  SOCP_ERR_UNSUPPORTED with the gain calls' messages: SOCP_INT_DOPRI5; no gain / gain_free entry; a free time before the final
 * node; an interior node with a FIXED or FREE component; too many states for the batched linear solve; and: no guide entry in the launch
 * table (the interceptor, vtolUAV, lqr1d; a plugin built before launch-table ABI 20 is refused when it registers).  An error writes
 * nothing, launches nothing and leaves the counters unchanged.
 * ONE launch; socp_ctx_counters advances by B K M trajectories.  _dev: device pointers, enqueue only, no allocation, no
 * synchronisation.  Host form: stages through the context's buffers and synchronises once; Xs travels both ways.  _blocks: per-row
 * parameter / time / xnode blocks as for socp_gain_batch_blocks. */
int socp_ctx_has_guide(const socp_ctx *ctx);            /* 1 / 0; SOCP_ERR_ARG for a NULL context */
int socp_guide_batch_dev(socp_ctx *ctx, int B, const double *d_Z, int stride, int cap, const double *d_Xq, const double *d_Kg,
                         const int *d_info, const int *d_count, int K, const double *d_dX0, int every, double *d_Xf, double *d_miss,
                         int *d_nupd, int *d_nskip, double *d_tf /* or NULL */, double *d_dxmax /* or NULL */, double *d_Xs /* or NULL */);
int socp_guide_batch(socp_ctx *ctx, int B, const double *Z, int stride, int cap, const double *Xq, const double *Kg, const int *info,
                     const int *count, int K, const double *dX0, int every, double *Xf, double *miss, int *nupd, int *nskip, double *tf,
                     double *dxmax, double *Xs);
int socp_guide_batch_blocks(socp_ctx *ctx, int B, const double *Z, const double *params, int param_stride, const double *time,
                            const double *xnode, int stride, int cap, const double *Xq, const double *Kg, const int *info,
                            const int *count, int K, const double *dX0, int every, double *Xf, double *miss, int *nupd, int *nskip,
                            double *tf, double *dxmax, double *Xs);

/* HAMILTONIAN GRADIENT: the costate equations a model's Hamiltonian text implies, G = (dH/dp, -dH/dx), at a batch of points -- the
 * check of a hand-written right-hand side against its Hamiltonian, and the right-hand side of a model that brings no dynamics at all
 * (include/socp_plugin.h, "A MODEL FROM ITS HAMILTONIAN").  A model-authoring instrument: no problem has to be set, there is no sweep
 * flag and no per-row parameter block.
 * t[B], sw[B][2] (or NULL: the context's switching times), X[B][S] exactly as socp_eval_batch takes them -> G[B][S], directly comparable
 * with what SOCP_EVAL_RHS writes.  One lane per point, ONE launch.  Per point, with H = the model's hamiltonian_t (the Hamiltonian
 * over a number type, the control law evaluated INSIDE it: X -> H(X, u(X))):
 *   1. Y[i] = (X[i]; e_i), i < S: the value X[i] and S derivative parts, 1.0 in part i and +0.0 elsewhere.
 *   2. h = hamiltonian_t(P, sw0, sw1, t, Y) on numbers with S derivative parts.  Part k of every operation is the DUAL NUMBERS rule
 *      of socp_fields_batch on (v, d[k]), one IEEE rounding per listed step, no contraction; the value part and whatever reads value
 *      parts only (a quotient's q = a.v / b.v, a root's s + s, exp's e) is computed once.  A plain double (a parameter, a literal, t,
 *      a control or penalty the law makes a constant) takes part with its zero terms DROPPED, as there.  Parts never meet, so part k
 *      is what a single dual number seeded with e_k gives, bit for bit: the result does not depend on how many directions travel in
 *      one evaluation (the kernel may cut the S directions into passes of any width; it takes one pass for every in-tree model).
 *   3. G[i] = h.d[i + d] and G[i + d] = -(h.d[i]) for i < d: one unary minus, nothing else.
 * WHAT IT IS: the TOTAL derivative of X -> H(X, u(X)).  It equals Pontryagin's x' = dH/dp, p' = -dH/dx (partials at fixed u) where
 * the law minimises H(X, .) over a set that does not depend on X -- at an interior minimiser dH/du = 0, on the set's boundary the
 * extra term is a multiplier times the derivative of a constraint X does not move (envelope theorem) -- up to the rounding of the
 * rules above.  A kink (a clamp, a penalty's onset, Goddard's t <= sw0) differentiates the BRANCH TAKEN at X.  A law that is not such
 * a minimiser gives something else, and its model needs a hand-written right-hand side.  For the in-tree models (measured in 240
 * bits, tests/test_hamiltonian_model_cpu.py): the double integrator on both sides of its saturation, and Goddard with the thrust
 * saturated, interior and off (mu2 > 0) and full, at a given singular value and off (mu2 = 0) agree with their right-hand sides to
 * rounding.  Goddard's CLOSED-FORM singular control (mu2 = 0, singularControl < 0, sw0 < t <= sw1) is a feedback that minimises H only
 * ON the singular surface Switch = mu1 - b p_m - C |p_v| / m = 0: there G agrees too; off it G - rhs = Switch (d alpha/dp, -d alpha/dx)
 * with alpha the singular thrust -- not an error of either text, but a model written from H alone would leave that surface where the
 * hand-written dynamics stay on it.  covid19 does NOT agree in rows 4 and 6, by exactly (pS - pE) (Rt - R) I / Tinf / N and
 * (pS - pE) (Rt - R) S / Tinf / N with Rt = R0 (1 - u): the upstream dynamics (covid19.cpp:88,90) multiply by the state R = X[3] where
 * -dH/dx has Rt.  The library keeps the upstream text for parity, bit for bit; the call is how to see it.
 * ONE OBJECT, NO CONTRACTION: a throughput-flavour context returns the same bits.  Goddard takes the law from the context's mu2 as
 * socp_eval_batch does.  tests/hamiltonian_model_reference.py restates the definition; the tests compare whole buffers to it.
 * socp_ctx_has_hamiltonian_gradient: 1 when the model's launch table has the entry -- any model with the hamiltonian_t trait: Goddard,
 * the double integrator, covid19, a plugin that brings it -- else 0 (the interceptor, vtolUAV, a plugin without the trait).
 * socp_ctx_counters advances by one launch and no trajectory.  SOCP_ERR_ARG: B < 0, or t, X or G NULL with B > 0.
 * SOCP_ERR_UNSUPPORTED: the launch table has no hamiltonian_gradient entry (a plugin built before launch-table ABI 16 is refused when
 * it registers: rebuild it).  B == 0: SOCP_OK without a launch.  An error writes nothing and leaves the context and its counters
 * unchanged.  The _dev form takes device pointers, only enqueues on the context's stream and neither allocates, copies nor
 * synchronises; the host form stages through that stream and the context's grow-only buffers.
 * Not covered: per-row parameter blocks, second derivatives (exact fields of a model written from H alone), reverse mode. */
int socp_ctx_has_hamiltonian_gradient(const socp_ctx *ctx);      /* 1 / 0; SOCP_ERR_ARG for a NULL context */
int socp_hamiltonian_gradient_batch_dev(socp_ctx *ctx, int B, const double *d_t, const double *d_sw /* or NULL */, const double *d_X,
                                        double *d_G);
int socp_hamiltonian_gradient_batch(socp_ctx *ctx, int B, const double *t, const double *sw /* or NULL */, const double *X, double *G);

/* NESTED DUAL NUMBERS and the JACOBIAN OF THE HAMILTONIAN VECTOR FIELD: A = dG/dX of the gradient above at a batch of points -- the
 * linearised dynamics of an extremal, A(t, X) = d/dX (dH/dp, -dH/dx), the matrix of the variational equations and of every
 * neighbouring-extremal or Riccati computation on top of Phi -- and the number type that gives a model written from H alone its
 * right-hand side over dual numbers (include/socp_plugin.h, "A MODEL FROM ITS HAMILTONIAN, WITH THE EXACT ENTRIES").
 * THE NUMBER.  A nested number is (v; d[0 .. W)) whose parts are themselves DUAL NUMBERS (v, d) of socp_fields_batch: 2 (1 + W)
 * doubles.  Part k of every rule is the rule of DUAL NUMBERS / HAMILTONIAN GRADIENT on (v, d[k]) with every listed operation carried
 * out ON DUAL NUMBERS, each of those with its own listed roundings.  With a, b nested, c plain, all operations dual-number ones:
 *     a + b = (a.v + b.v; a.d[k] + b.d[k])        a - b likewise        -a = (-a.v; -a.d[k])
 *     a b   = (a.v b.v; l + m),  l = a.d[k] b.v,  m = a.v b.d[k]
 *     a / b = (q; (a.d[k] - m) / b.v),  q = a.v / b.v,  m = q b.d[k]
 *     c + a = (c + a.v; a.d[k])    a + c = (a.v + c; a.d[k])    c - a = (c - a.v; -a.d[k])    a - c = (a.v - c; a.d[k])
 *     c a   = (c a.v; c a.d[k])    a c   = (a.v c; a.d[k] c)    a / c = (a.v / c; a.d[k] / c)
 *     c / a = (q; (-m) / a.v),  q = c / a.v,  m = q a.d[k]
 *     |a|   = (|a.v|; a.d[k] negated when the innermost value a.v.v < 0)
 *     sqrt a = (s; q),  s = sqrt(a.v),  s2 = s + s,  q = a.d[k] / s2, and q = (0.0, +0.0) when the innermost value s.v == 0
 *     exp a  = (e; e a.d[k]),  e = exp(a.v) (the dual-number exp: exp_glibc on the innermost value)
 * The value part v and whatever reads value parts only (q, s2, e) is computed ONCE.  A plain c is a double -- its zero terms are
 * dropped at both levels, by these rules and by DUAL NUMBERS' own mixed rules inside them -- or a plain DUAL NUMBER, a parameter read
 * through the dual view of socp_sensitivity_batch: plain at the outer level (the outer zero terms dropped), a full dual number at the
 * inner one.  A comparison reads the innermost value.  Seeds are the explicit dual numbers (1.0, +0.0) and (0.0, +0.0) and are
 * computed with, not dropped.  Parts never meet, so part k does not depend on W.  CONSEQUENCE: the value part of every nested operation
 * is the corresponding operation of HAMILTONIAN GRADIENT's numbers, step for step -- the value parts of a nested gradient are the
 * gradient's bits.
 * THE NESTED GRADIENT of dual numbers X[i] = (x_i, xd_i), i < S:
 *   1. Y[i] = (X[i]; e_i): the nested number with value part X[i] and parts (1.0, +0.0) in part i, (0.0, +0.0) elsewhere; the S parts
 *      cut into passes of W, a part at or beyond S dropped.
 *   2. h = hamiltonian_t(P, sw0, sw1, t, Y) on nested numbers.
 *   3. G[i] = h.d[i + d] and G[i + d] = -(h.d[i]) for i < d, the minus DUAL NUMBERS' (-v, -d).
 * G[i].v is the HAMILTONIAN GRADIENT at x, bit for bit; G[i].d is the directional derivative of the gradient along xd.  This is the
 * rhs_t of a model registered through SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT, with the parameter view passed through.
 * THE CALL.  t[B], sw[B][2] (or NULL), X[B][S] exactly as socp_hamiltonian_gradient_batch takes them -> A[B][S * S], column-major per
 * point: A[b][S j + i] = dG_i/dX_j, and, unless G is NULL, G[B][S]: the value parts, bit-equal to socp_hamiltonian_gradient_batch.
 * One lane per point, ONE launch, no LDS.  Per point, for j = 0 .. S-1 (a loop): X seeded with e_j -- X[i] = (x_i, 1.0 if i == j else
 * +0.0) -- the nested gradient above, and column j = its derivative parts; G from j = 0.
 * WHAT IT IS: the TOTAL second derivative of X -> H(X, u(X)), the control law inside: A = Omega Hess with Omega = [0 I; -I 0], so
 * -Omega A is symmetric wherever the text is twice differentiable on the branch taken (to rounding in doubles; to 2^-200 in the 240-bit
 * restatement).  It is the linearisation of Pontryagin's equations where the envelope argument of HAMILTONIAN GRADIENT holds on an open
 * set: the double integrator on both arcs, Goddard mu2 > 0 on its three arcs, Goddard mu2 = 0 at full thrust and off agree with
 * d rhs_t/dX in 240 bits.  On Goddard's closed-form singular arc and for covid19, where G itself is not rhs or agrees on a surface only,
 * A is NOT d rhs/dX (tests/test_hamiltonian_exact_cpu.py records by how much).  At a kink it is the BRANCH TAKEN.
 * ONE OBJECT, NO CONTRACTION: a throughput-flavour context returns the same bits.  Goddard takes the law from the context's mu2 as
 * socp_eval_batch does.  tests/hamiltonian_exact_reference.py restates the definition; the tests compare whole buffers to it.
 * socp_ctx_has_hamiltonian_jacobian: 1 when the model's launch table has the entry -- any model whose hamiltonian_t takes nested
 * numbers: Goddard, the double integrator, covid19, a plugin with the hamiltonian_t trait -- else 0 (the interceptor, vtolUAV, a plugin
 * without the trait).  socp_ctx_counters advances by one launch and no trajectory.  SOCP_ERR_ARG: B < 0, or t, X or A NULL with B > 0.
 * SOCP_ERR_UNSUPPORTED: the launch table has no hamiltonian_jacobian entry (a plugin built before launch-table ABI 17 is refused when
 * it registers: rebuild it).  B == 0: SOCP_OK without a launch.  An error writes nothing and leaves the context and its counters
 * unchanged.  The _dev form takes device pointers, only enqueues on the context's stream and neither allocates, copies nor
 * synchronises; the host form stages through that stream and the context's grow-only buffers.
 * Not covered: per-row parameter blocks, a third nesting level, reverse mode, vtolUAV and the interceptor (their tanh and hooks need
 * definitions of their own). */
int socp_ctx_has_hamiltonian_jacobian(const socp_ctx *ctx);      /* 1 / 0; SOCP_ERR_ARG for a NULL context */
int socp_hamiltonian_jacobian_batch_dev(socp_ctx *ctx, int B, const double *d_t, const double *d_sw /* or NULL */, const double *d_X,
                                        double *d_A, double *d_G /* or NULL */);
int socp_hamiltonian_jacobian_batch(socp_ctx *ctx, int B, const double *t, const double *sw /* or NULL */, const double *X, double *A,
                                    double *G /* or NULL */);

/* The distinct roots of a whole sweep: which distinct rows does a table hold, how many rows went to each, and which row went where.
 * Model-independent (no problem has to be set, no launch table is used).
 * Rows V[B][ld]; the first n <= ld entries of a row are compared.  Greedy leader grouping IN ROW ORDER:
 *
 *   G = 0
 *   for b = 0 .. B-1:
 *       if mask != NULL and mask[b] == 0:      label[b] = SOCP_GROUP_MASKED    (-3); continue
 *       if any of V[b][0..n) is not finite:    label[b] = SOCP_GROUP_NOTFINITE (-2); continue
 *       for g = 0 .. G-1 (in this order): if near(V[b], V[leader[g]]): label[b] = g; break
 *       else if G < max_groups:  leader[G] = b; label[b] = G; G += 1
 *       else:                    label[b] = SOCP_GROUP_OVERFLOW (-1)
 *
 *   near(v, l)  <=>  for every i < n:  |fl(v_i - l_i)| <= fl(atol + fl(rtol * |l_i|))      (inclusive; no contraction)
 *
 * A row joins the FIRST leader it is near, not the nearest.  The relation is not transitive, and this rule is what makes the result
 * unique.
 * Outputs:
 *   label[B]
 *   leader[max_groups]   the leader's row index, ascending; unused slots are -1
 *   count[max_groups]    the number of members, leader included; unused slots are 0
 *   radius[max_groups]   the maximum over a group's members and over i of |fl(v_i - l_i)|; unused slots are 0
 *   summary[4]           G, and the number of overflow, non-finite and masked rows
 * Every output is independent of summation order: label, leader, count and summary are integers, radius is a maximum of exactly
 * rounded differences.  So there is ONE build of the kernels, compiled without contraction, and it serves both arithmetic flavours
 * (every SOCP_VARIANT_*) bit for bit.
 * On the device one round per group: in round g the leader is the lowest row still unassigned, and every unassigned row near it
 * takes label g (kernels_group.hip has the equivalence argument).  A round reads the 4 B bytes of the labels and the rows still
 * unassigned; the cost is G rounds, and a table of all-distinct rows costs max_groups rounds and ends in overflow labels.  Rounds are
 * enqueued in chunks (1, 2, 4, 8, then 16 at a time) and the "next leader" word is read back once per chunk: BOTH forms synchronise
 * the context's stream, the _dev form once per chunk.  Launches: two to begin (one when B == 0), the rounds, one to end;
 * socp_ctx_counters advances by them and by no trajectory.
 * The _dev form takes device pointers; its scratch (max_groups + 1 words) comes from the context's grow-only workspace.  The host
 * form stages through the context's stream and returns when the results are in the caller's arrays.  All element offsets are 64-bit
 * (B ld may exceed 2^31).
 * SOCP_ERR_ARG (with a message): B < 0, n < 1, ld < n, max_groups < 1; atol or rtol negative or not finite; a NULL output pointer
 * (label may be NULL when B == 0); V NULL with B > 0.  An error writes nothing.  B == 0: SOCP_OK, summary all zero and the slots
 * filled as unused. */
#define SOCP_GROUP_OVERFLOW  -1
#define SOCP_GROUP_NOTFINITE -2
#define SOCP_GROUP_MASKED    -3
int socp_group_batch_dev(socp_ctx *ctx, int B, int n, int ld, const double *d_V, const int *d_mask /* or NULL */,
                         double atol, double rtol, int max_groups,
                         int *d_label, int *d_leader, int *d_count, double *d_radius, int *d_summary);
int socp_group_batch    (socp_ctx *ctx, int B, int n, int ld, const double *V, const int *mask,
                         double atol, double rtol, int max_groups,
                         int *label, int *leader, int *count, double *radius, int *summary);

#ifdef __cplusplus
}
#endif
#endif /* SOCP_HIP_H_ */
