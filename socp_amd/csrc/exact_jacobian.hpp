// exact_jacobian.hpp -- K_exactjac: the exact Jacobian dF/dz of the shooting function of B unknown vectors (socp_exact_jacobian_batch;
// the definition is the comment of the entry points in include/socp_hip.h, tests/exact_jacobian_reference.py restates it in Python).
//
// The kernel shape of fields_group_kernel (fields.hpp): the S + 1 columns of one (row, segment) take identical steps, so they sit
// in G = S + 1 NEIGHBOURING lanes of one wavefront (group_lane, segment_views.hpp).  Lane c < S carries the
// state as S dual numbers started from (X0, e_c): column S i + c of the matrix, the unknown z[S i + c].  Lane S -- the LENGTH lane --
// starts from (X0, 0) and carries the derivative with respect to the segment's length L = t2 - t1: t2 = (t2, 1.0) there, (t2, +0.0)
// in the state lanes.  ONE text for every lane: the step length is a dual number in all of them, h F is the full dual product, and
// the loop condition and the clamp read value parts, so a group never diverges.
// After the loop every lane evaluates the residual rows its segment owns on its dual end state (segment_residual restated on
// duals) and stores the derivative part at (row, its column); the length lane stores w (d row / d L) at (row, k) for each of
// the at most two FREE times its segment's ends depend on.  Lane 0 stores the value parts into F.  The part of a node's rows that
// depends on the NEXT segment's start state is stored by that segment's state lanes, which own those columns: every entry of the
// matrix has one writer, so there is no atomic and no second launch; the matrix is zero-filled on the stream before the launch
// (plugin_impl.hpp).  Every store site is ONE block under ONE computed predicate; no register array is indexed by a run-time
// value (see the note in segment_residual).
#pragma once
#include "dual.hpp"
#include "fields.hpp"
#include "integrator.hpp"

namespace socp {

// optional trait kSwitchingReadsXp: the model's free-interior-time row is H(t, X-) - H(t, X+) (model.hpp:299-304) -- the lanes
// of the next segment store -grad H(X+).  Absent or false: the row does not read X+ (Goddard: goddard.cpp:343-370)
template <class M, class = void> struct switching_reads_xp : std::false_type {};
template <class M> struct switching_reads_xp<M, std::void_t<decltype(M::kSwitchingReadsXp)>> : std::bool_constant<M::kSwitchingReadsXp> {};

// optional trait final_row_t: the text of a custom final row (kCustomFinal: final_row, final_h_offset) over a number type -- the rows of
// the last node are then final_row_t on the dual end state and H + final_h_offset, as segment_residual forms them
template <class M, class = void> struct has_final_row_t : std::false_type {};
template <class M>
struct has_final_row_t<M, std::void_t<decltype(M::template final_row_t<Dual>(std::declval<const ModelParams &>(), 0, 0,
                                                                             std::declval<const Dual (&)[M::S]>(), (const double *)nullptr))>>
    : std::true_type {};

// optional trait switching_state_t: the switching_state hook with the arriving state X over a number type and the node's unknowns Xp
// as plain doubles -- the two rows of a FREE state component of an interior node, differentiated by the lanes of the segment that ENDS
// there.  The model must also declare kSwitchingStateXpContinuous = true: the promise that the hook reads Xp only as -Xp[j] in f_state
// and -Xp[j + D] in f_costate, so that the lanes of the NEXT segment store the same -1 entries they store for a CONTINUOUS row
template <class M, class = void> struct switching_state_xp_continuous : std::false_type {};
template <class M>
struct switching_state_xp_continuous<M, std::void_t<decltype(M::kSwitchingStateXpContinuous)>> : std::bool_constant<M::kSwitchingStateXpContinuous> {};
template <class M, class = void> struct has_switching_state_t : std::false_type {};
template <class M>
struct has_switching_state_t<M, std::void_t<decltype(M::template switching_state_t<Dual>(
                                    std::declval<const ModelParams &>(), 0.0, 0, std::declval<const Dual (&)[M::S]>(),
                                    std::declval<const double (&)[M::S]>(), (const double *)nullptr, std::declval<Dual &>(), std::declval<Dual &>()))>>
    : std::bool_constant<switching_state_xp_continuous<M>::value> {};

// the hooks the definition covers: custom final rows through final_row_t, a switching_state hook through switching_state_t
template <class M>
struct exact_jacobian_covers_hooks : std::bool_constant<(!has_custom_final<M>::value || has_final_row_t<M>::value) &&
                                                        (!has_switching_state<M>::value || has_switching_state_t<M>::value)> {};

// c(j, f): the weight of junction f's time in node j's (Timeline::nt): 1.0 for j == f; (double)(j - a) / (double)(b - a) for
// f == b, 1.0 minus that for f == a when node j is interpolated between the junctions a and b; 0.0 otherwise
__device__ __forceinline__ double time_weight(const ProblemDev &pb, int j, int f)
{
    if (j == f) return 1.0;
    if (pb.node_kind[j] != -2) return 0.0;
    const int a = pb.lo[j], b = pb.hi[j];
    const double q = (double)(j - a) / (double)(b - a);
    return f == b ? q : (f == a ? 1.0 - q : 0.0);
}

template <class Mdl, bool PERPROB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void exact_jacobian_kernel(ModelParams P, ProblemDev pb, int B,
                                                               const double *__restrict__ Z, double *__restrict__ Fjac,
                                                               double *__restrict__ Fout)
{
    static_assert(!has_custom_traj<Mdl>::value && exact_jacobian_covers_hooks<Mdl>::value,
                  "the exact Jacobian of such a model needs a definition of its own");
    constexpr int S = Mdl::S;
    constexpr int D = Mdl::D;
    constexpr int G = S + 1;                                          // one lane per column: S state columns and the length
    static_assert(G <= 64, "a group fits one wavefront");
    const GroupLane L = group_lane(B, pb.M, G);
    const double *zr = Z + L.b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    ModelParams Pq = P;
    ProblemDev pq = pb;
    if constexpr (PERPROB) load_problem_block(pb, L.b, Pq, pq);
    const int c = L.c, i = L.i;
    const long b = L.b;
    const bool live = L.live;
    const int M = pq.M, n = pq.n;
    double X0[S];
    const SegmentSpan<Mdl> sp(Pq, pq, z, i, X0);
    const double t1 = sp.t1, t2 = sp.t2, sw0 = sp.sw0, sw1 = sp.sw1;

    const bool len = c == S;                                          // the length lane
    const bool ws = live && !len;                                     // stores derivative parts into its own column S i + c
    const bool wf = live && c == 0 && Fout != nullptr;                // stores value parts into F
    double *const Jb = Fjac + b * ((long)n * n);
    double *const col = Jb + (long)n * (S * i + (len ? 0 : c));
    double *const Fb = Fout + (Fout != nullptr ? b * n : 0);

    Dual X[S];
    dual_start(X0, c, X);                                             // the length lane: c == S, no unit entry

    // ---- the rows that read the segment's START state: the length lane has no part in them
    if (i == 0) {
        // model.hpp:196-228 InitialFunction / :239-290 InitialHFunction on duals
#pragma unroll
        for (int j = 0; j < D; j++) {
            // FREE: the costate; else the state against xd.  Both are formed and each has its own store sites: a select between
            // X[j + D] and X[j] becomes a select between two ADDRESSES -- a run-time index into X, which then lives in LDS or scratch
            const bool fr = pq.mode_x[j] == 1;
            const Dual ef = X[j + D], ex = X[j] - pq.xnode[j];
            const bool s1 = ws && fr, s2 = ws && !fr, f1 = wf && fr, f2 = wf && !fr;
            if (s1) { col[j] = ef.d; }
            if (s2) { col[j] = ex.d; }
            if (f1) { Fb[j] = ef.v; }
            if (f2) { Fb[j] = ex.v; }
        }
        const int hr = pq.ft_row[0];
        if (hr >= 0) {
            const Dual H = Mdl::template hamiltonian_t<Dual>(Pq, sw0, sw1, t1, X);
            if (ws) { col[hr] = H.d; }
            if (wf) { Fb[hr] = H.v; }
        }
    } else {
        // node i's rows, the part that depends on this segment's start state Xp = z[S i ..): the -1 of a CONTINUOUS row
        // (X - Xp), the unit of a FIXED row's second half (Xp - xd), and -grad H(Xp) of the free-time row where it reads Xp
        const int jc = len ? 0 : (c < D ? c : c - D);
        const int mode = pq.mode_x[i * D + jc];
        const bool st = ws && (mode == 0 ? c < D : true);
        const int row = S * i + (mode == 0 ? D + c : c);
        const double unit = mode == 0 ? 1.0 : -1.0;
        if (st) { col[row] = unit; }
        if constexpr (switching_reads_xp<Mdl>::value) {
            const int hr = pq.ft_row[i];
            if (hr >= 0) {
                const Dual Hp = -Mdl::template hamiltonian_t<Dual>(Pq, sw0, sw1, t1, X);
                if (ws) { col[hr] = Hp.d; }
            }
        }
    }

    // ---- the steps: t2 = (t2, delta), delta = 1.0 in the length lane
    fixed_steps_dual(Pq.step_nbr, t1, Dual(t2, len ? 1.0 : 0.0),
                     [&](const Dual &t, const Dual &step) { dual_rk4<Mdl>(Pq, sw0, sw1, t, X, step); });

    // ---- the free times this segment's length depends on: the junctions A <= i and Bn >= i + 1 that bracket it
    const int A = pq.node_kind[i] == -2 ? pq.lo[i] : i;
    const int Bn = pq.node_kind[i + 1] == -2 ? pq.hi[i + 1] : i + 1;
    const int kA = pq.node_kind[A], kB = pq.node_kind[Bn];            // >= 0: the index of the free time's unknown
    const double wA = time_weight(pq, i + 1, A) - time_weight(pq, i, A);
    const double wB = time_weight(pq, i + 1, Bn) - time_weight(pq, i, Bn);
    const bool fA = live && len && kA >= 0 && wA != 0.0;
    const bool fB = live && len && kB >= 0 && wB != 0.0;
    double *const colA = Jb + (long)n * (kA >= 0 ? kA : 0);
    double *const colB = Jb + (long)n * (kB >= 0 ? kB : 0);
    // `deriv` false: a row whose derivative belongs to other lanes (the second half of a FIXED row); `on` false: nothing is stored
    auto emit = [&](int row, const Dual &e, bool deriv, bool on = true) {
        const bool s0 = ws && deriv && on, sa = fA && deriv && on, sb = fB && deriv && on, sf = wf && on;
        if (s0) { col[row] = e.d; }
        if (sa) { colA[row] = wA * e.d; }
        if (sb) { colB[row] = wB * e.d; }
        if (sf) { Fb[row] = e.v; }
    };

    // ---- the rows that read the segment's END state
    if (i < M - 1) {
        double Xp[S];
#pragma unroll
        for (int k = 0; k < S; k++) Xp[k] = z(S * (i + 1) + k);
        // free interior time: model::SwitchingTimesFunction (shooting.cpp:964-968); Xp takes part as constants
        if (pq.ft_row[i + 1] >= 0) {
            Dual XpD[S];
#pragma unroll
            for (int k = 0; k < S; k++) XpD[k] = Dual(Xp[k], 0.0);
            emit(pq.ft_row[i + 1], Mdl::template switching_fn_t<Dual>(Pq, sw0, sw1, t2, X, XpD), true);
        }
        // shooting::MultipleShootingFunction (shooting.cpp:1511-1576): FIXED pins both sides, otherwise state and costate jumps
        const int *mx = pq.mode_x + (i + 1) * D;
        const double *xd = pq.xnode + (i + 1) * S;
#pragma unroll
        for (int j = 0; j < D; j++) {
            const int row = S * (i + 1) + j;
            const bool fixed = mx[j] == 0;
            const double xdj = xd[j];
            const Dual a = X[j] - (fixed ? xdj : Xp[j]);
            const Dual bb(fixed ? Xp[j] - xdj : X[j + D].v - Xp[j + D], X[j + D].d);      // FIXED: only the value is read
            if constexpr (has_switching_state<Mdl>::value) {
                // FREE: the model's SwitchingStateFunction on the dual end state (segment_residual's third arm).  The hook is
                // evaluated for every mode and its two numbers are SELECTED part by part: the store sites stay the two emits.  The
                // -1 of Xp[j] and of Xp[j + D] belong to the next segment's lanes, which store them for every mode != FIXED
                Dual fs, fc;
                Mdl::template switching_state_t<Dual>(Pq, t2, j, X, Xp, xd, fs, fc);
                const bool hook = mx[j] == 1;
                emit(row, Dual(hook ? fs.v : a.v, hook ? fs.d : a.d), true);
                emit(row + D, Dual(hook ? fc.v : bb.v, hook ? fc.d : bb.d), !fixed);
            } else {
                emit(row, a, true);
                emit(row + D, bb, !fixed);
            }
        }
    }
    if (i == M - 1) {
        // model.hpp:90-122 FinalFunction / :133-185 FinalHFunction on duals
        const int *mx = pq.mode_x + M * D;
        const double *xd = pq.xnode + M * S;
        if constexpr (has_custom_final<Mdl>::value) {
            // the model's own final rows (segment_residual's custom arm): final_row_t returns a COMPUTED number in either mode
#pragma unroll
            for (int j = 0; j < D; j++) emit(D + j, Mdl::template final_row_t<Dual>(Pq, j, mx[j], X, xd), true);
            if (pq.ft_row[M] >= 0) emit(pq.ft_row[M], Mdl::template hamiltonian_t<Dual>(Pq, sw0, sw1, t2, X) + Mdl::final_h_offset(Pq), true);
        } else {
#pragma unroll
            for (int j = 0; j < D; j++) {
                const bool fr = mx[j] == 1;                               // two gated emits, not a select: see the initial rows
                emit(D + j, X[j + D], true, fr);
                emit(D + j, X[j] - xd[j], true, !fr);
            }
            if (pq.ft_row[M] >= 0) emit(pq.ft_row[M], Mdl::template hamiltonian_t<Dual>(Pq, sw0, sw1, t2, X), true);
        }
    }
}

}  // namespace socp
