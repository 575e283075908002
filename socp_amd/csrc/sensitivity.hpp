// sensitivity.hpp -- K_sens: the exact right-hand sides G = dF/dtheta of socp_sensitivity_batch (the definition is the comment of the
// entry points in include/socp_hip.h, tests/sensitivity_reference.py restates it in Python).
//
// One lane per (row, segment, direction); the nd directions of one kind of one (row, segment) take identical steps, so they sit in nd
// NEIGHBOURING lanes of one wavefront (group_lane, segment_views.hpp), as the columns of exact_jacobian_kernel do.
// Two kinds integrate, one launch each (a wave then runs ONE text):
//   PARAM  the lane reads the row's parameter block through SeededParams: every slot a dual number (p_i, +0.0), the addressed one
//          (p_i, 1.0).  The view forms the pair where a slot is read, so no dual block is kept: the parameters stay where the residual
//          has them (kernel arguments, or the registers of the row's own block) and the seed is one compare per read.  The state starts
//          from (z, +0.0), the step is dual_rk4's with plain t and h (fields.hpp), the rows are segment_residual's on duals.
//   TIME   the LENGTH lane of exact_jacobian_kernel unchanged: t2 = (t2, 1.0), dual_rk4's dual step, plain parameters; the
//          lane stores w (d row / d L), w = c(i+1, f) - c(i, f), and nothing when w == 0.0.
// XNODE directions do not integrate (kernels_sensitivity.hip).  G is zero-filled on the stream before the launches; every entry has one
// writer: the lane of the segment that owns the row (the ROWS paragraph of socp_exact_jacobian_batch).  Every store site is ONE block
// under ONE computed predicate; no register array is indexed by a run-time value -- the directions travel packed in kernel-argument
// words, not in an array.
#pragma once
#include "dual.hpp"
#include "exact_jacobian.hpp"
#include "fields.hpp"
#include "integrator.hpp"
#include "launch.hpp"

namespace socp {

// the dual view of a packed parameter block: p[i] is (p_i, 1.0) for the seeded slot and (p_i, +0.0) for every other one
struct SeededParams {
    struct Block {
        const double *v;
        int seed;
        __device__ __forceinline__ Dual operator[](int i) const { return Dual(v[i], i == seed ? 1.0 : 0.0); }
    } p;
};

// entry c of the 16-bit fields a SensDirs (launch.hpp) carries in four words
__host__ __device__ __forceinline__ int sens_index(const unsigned long long (&w)[4], int c)
{
    const unsigned long long word = c < 4 ? w[0] : (c < 8 ? w[1] : (c < 12 ? w[2] : w[3]));
    return (int)((word >> (16 * (c & 3))) & 0xffffull);
}

// the rows that read the segment's END state (exact_jacobian_kernel's, derivative parts only): emit(row, e, on) stores e.d when on
template <class Mdl, class PV, class ZRead, class Emit>
__device__ __forceinline__ void sensitivity_end_rows(const PV &Pv, const ProblemDev &pq, int i, double sw0, double sw1, double t2,
                                                     const Dual (&X)[Mdl::S], const ZRead &z, const Emit &emit)
{
    constexpr int S = Mdl::S;
    constexpr int D = Mdl::D;
    const int M = pq.M;
    if (i < M - 1) {
        // free interior time: model::SwitchingTimesFunction; Xp takes part as (Xp, +0.0), the parameter view as it is
        if (pq.ft_row[i + 1] >= 0) {
            Dual XpD[S];
#pragma unroll
            for (int k = 0; k < S; k++) XpD[k] = Dual(z(S * (i + 1) + k), 0.0);
            emit(pq.ft_row[i + 1], Mdl::template switching_fn_t<Dual>(Pv, sw0, sw1, t2, X, XpD), true);
        }
        // FIXED: X - xd (the second row reads Xp alone); otherwise the state and costate jumps X - Xp
        const int *mx = pq.mode_x + (i + 1) * D;
#pragma unroll
        for (int j = 0; j < D; j++) {
            const int row = S * (i + 1) + j;
            emit(row, X[j], true);
            emit(row + D, X[j + D], mx[j] != 0);
        }
    }
    if (i == M - 1) {
        const int *mx = pq.mode_x + M * D;
#pragma unroll
        for (int j = 0; j < D; j++) {
            const bool fr = mx[j] == 1;                                   // two gated emits, not a select: see exact_jacobian_kernel
            emit(D + j, X[j + D], fr);
            emit(D + j, X[j], !fr);
        }
        if (pq.ft_row[M] >= 0) emit(pq.ft_row[M], Mdl::template hamiltonian_t<Dual>(Pv, sw0, sw1, t2, X), true);
    }
}

template <class Mdl, int KIND, bool PERPROB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void sensitivity_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, SensDirs dirs, int K,
                                                             double *__restrict__ G)
{
    static_assert(!has_custom_traj<Mdl>::value && !has_custom_final<Mdl>::value && !has_switching_state<Mdl>::value,
                  "the sensitivities of such a model need a definition of their own");
    constexpr int S = Mdl::S;
    const GroupLane L = group_lane(B, pb.M, dirs.n);
    const double *zr = Z + L.b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    ModelParams Pq = P;
    ProblemDev pq = pb;
    if constexpr (PERPROB) load_problem_block(pb, L.b, Pq, pq);
    const int c = L.c, i = L.i;                                   // c: direction of this kind
    const bool live = L.live;
    // the prologue and the parameter arm's loop spelled out, not SegmentSpan / a shared loop: through them the direction launch ran 1.1 % longer
    const Timeline<decltype(z)> tl{pq, z};
    const double t1 = tl.nt(i), t2 = tl.nt(i + 1);
    const double sw0 = tl.template switching_time<Mdl>(Pq.sw0, pq.sw_node0), sw1 = tl.template switching_time<Mdl>(Pq.sw1, pq.sw_node1);

    const int slot = (int)((dirs.slot >> (4 * c)) & 0xfull);
    const int index = sens_index(dirs.index, c);
    double *const Gr = G + ((L.b * K + slot) * (long)pq.n);

    Dual X[S];
    {
        double X0[S];
        segment_start(z, S * i, X0);
#pragma unroll
        for (int j = 0; j < S; j++) X[j] = Dual(X0[j], 0.0);
    }

    if constexpr (KIND == kSensParam) {
        const SeededParams Pv{{Pq.p, index}};
        // the only START-state row that reads a parameter: the Hamiltonian of a free t0
        if (i == 0) {
            const int hr = pq.ft_row[0];
            if (hr >= 0) {
                const Dual H = Mdl::template hamiltonian_t<Dual>(Pv, sw0, sw1, t1, X);
                if (live) { Gr[hr] = H.d; }
            }
        }
        // the loop of Lane::integrate: plain t and h, as fields_group_kernel
        const double dt = (t2 - t1) / Pq.step_nbr;
        double t = t1;
        int guard = Pq.step_nbr + 8;
        while (t < (t2 - dt / 2) && guard-- > 0) {
            const double step = (t + dt > t2) ? (t2 - t) : dt;
            dual_rk4<Mdl>(Pv, sw0, sw1, t, X, step);
            t += dt;
        }
        auto emit = [&](int row, const Dual &e, bool on) {
            const bool s0 = live && on;
            if (s0) { Gr[row] = e.d; }
        };
        sensitivity_end_rows<Mdl>(Pv, pq, i, sw0, sw1, t2, X, z, emit);
    } else {
        // node `index` is a FIXED junction: its weight in this segment's length
        const double w = time_weight(pq, i + 1, index) - time_weight(pq, i, index);
        const bool ws = live && w != 0.0;
        if (!__any(ws)) return;                                   // wave-uniform: no lane of this wave has anything to store
        fixed_steps_dual(Pq.step_nbr, t1, Dual(t2, 1.0),
                         [&](const Dual &t, const Dual &step) { dual_rk4<Mdl>(Pq, sw0, sw1, t, X, step); });
        auto emit = [&](int row, const Dual &e, bool on) {
            const bool s0 = ws && on;
            if (s0) { Gr[row] = w * e.d; }
        };
        sensitivity_end_rows<Mdl>(Pq, pq, i, sw0, sw1, t2, X, z, emit);
    }
}

}  // namespace socp
