// guide.hpp -- K_guide: K dispersed cases per row of a batch flown IN CLOSED LOOP under the sampled neighbouring-extremal law
// (socp_guide_batch; the definition is the comment of the entry points in include/socp_hip.h, tests/guide_reference.py restates it
// in Python).  The tables of socp_gain_batch / socp_gain_free_batch are INPUTS.
//
// One lane = (row b, case k), T = b K + k (row_lane with K items per row): the K cases of a row sit in neighbouring lanes, read the
// same Xq, Kg and info words in the same instruction, and a table entry travels once per row.  The lane flies ALL M segments one after
// the other from its own state -- a plain 2d-state trajectory on Lane<Mdl>::rk4, the residual's hot path; no dual numbers, so the
// occupancy is the residual's, not the gain kernels' one wave per SIMD.  The loop of a segment is gain_blocks_kernel's value loop (the
// same t, dt, clamped last step and guard, the guard written as a bound on the steps taken so that it survives a re-timing), cut into
// blocks of `stride` steps; at the head of every block sits the SAMPLE: the correction when it is due, then the stores.
// FREE_TF: the final time in force is a register of the lane; the z reader hands it out in place of z[n - 1], so the timeline is the
// residual's own Timeline evaluated on it, and an applied correction that moves it re-times the segment under way.
// No register array is indexed by a run-time value, every store site is ONE block under ONE computed predicate (segment_residual's
// note); the d^2 gain entries are consumed as they are loaded, one running sum per costate component.
#pragma once
#include "launch.hpp"
#include "segment_views.hpp"

namespace socp {

template <class Mdl, bool FREE_TF>
__device__ __forceinline__ void guide_lane(const ModelParams &P, const ProblemDev &pb, const double *__restrict__ zr, long b, long T,
                                           const GuideArgs &A)
{
    static_assert(!has_custom_traj<Mdl>::value && !has_custom_final<Mdl>::value && !has_switching_state<Mdl>::value,
                  "the closed-loop flight of such a model needs a definition of its own");
    constexpr int S = Mdl::S, D = Mdl::D;
    constexpr int LDK = FREE_TF ? D + 1 : D;
    constexpr int NM = FREE_TF ? D + 1 : D;
    const int M = pb.M, n = pb.n, cap = A.cap, stride = A.stride, N = P.step_nbr;
    double tfc = FREE_TF ? zr[n - 1] : 0.0;                           // the final time in force
    auto z = [&](int k) -> double { return (FREE_TF && k == n - 1) ? tfc : zr[k]; };
    const Timeline<decltype(z)> tl{pb, z};

    // the start: x = z_x + dX0, p = z_p
    double X[S];
    {
        const double *d0 = A.dX0 + T * D;
#pragma unroll
        for (int j = 0; j < D; j++) X[j] = zr[j] + d0[j];
#pragma unroll
        for (int j = 0; j < D; j++) X[D + j] = zr[D + j];
    }
    int nupd = 0, nskip = 0;
    int wait = 0;                        // samples until the next due one; every == 0: never due
    double dmax = 0.0;
    double t2 = 0.0, sw0 = P.sw0, sw1 = P.sw1;
    for (int i = 0; i < M; i++) {
        double t1 = tl.nt(i);
        t2 = tl.nt(i + 1);
        sw0 = tl.template switching_time<Mdl>(P.sw0, pb.sw_node0);
        sw1 = tl.template switching_time<Mdl>(P.sw1, pb.sw_node1);
        double dt = (t2 - t1) / N;
        double t = t1;
        int k = 0;                       // steps this segment has taken
        const long seg = b * M + i;
        const int cnt = A.count[seg];
        const int nq = cnt < cap ? cnt : cap;                       // the table slots of this segment
        bool act = t < (t2 - dt / 2) && k < N + 8;
        int q = 0;
        bool go = true;                  // the first sample always (a segment without a step has sample 0)
        while (go) {
            // ---- sample q, the start of step q stride
            const long slot = seg * cap + q;
            const bool has = q < nq;
            const bool due = A.every > 0 && wait == 0;
            wait = A.every > 0 ? (wait == 0 ? A.every : wait) - 1 : 0;
            const bool look = due && has;
            const bool apply = look && A.info[slot] == 0;
            nskip += (due && !apply) ? 1 : 0;
            nupd += apply ? 1 : 0;
            if (look) {
                const double *xq = A.Xq + slot * S;
                double dx[D];
#pragma unroll
                for (int c = 0; c < D; c++) {
                    dx[c] = X[c] - xq[c];
                    const double a = fabs(dx[c]);
                    dmax = a > dmax ? a : dmax;
                }
                if (apply) {
                    const double *kg = A.Kg + slot * (LDK * D);
#pragma unroll
                    for (int r = 0; r < D; r++) {
                        double s = kg[r] * dx[0];
#pragma unroll
                        for (int c = 1; c < D; c++) s = s + kg[c * LDK + r] * dx[c];
                        X[D + r] = xq[D + r] + s;
                    }
                    if constexpr (FREE_TF) {
                        double s = kg[D] * dx[0];
#pragma unroll
                        for (int c = 1; c < D; c++) s = s + kg[c * LDK + D] * dx[c];
                        const double tfn = zr[n - 1] + s;
                        if (tfn != tfc) {
                            // the timeline with tf' as the last unknown; the clock keeps the step index
                            tfc = tfn;
                            t1 = tl.nt(i);
                            t2 = tl.nt(i + 1);
                            sw0 = tl.template switching_time<Mdl>(P.sw0, pb.sw_node0);
                            sw1 = tl.template switching_time<Mdl>(P.sw1, pb.sw_node1);
                            dt = (t2 - t1) / N;
                            t = t1 + (double)k * dt;
                            act = t < (t2 - dt / 2) && k < N + 8;
                        }
                    }
                }
            }
            const bool sx = has && A.Xs != nullptr;
            if (sx) {
                double *out = A.Xs + ((T * M + i) * cap + q) * S;
#pragma unroll
                for (int j = 0; j < S; j++) out[j] = X[j];
            }
            // ---- the block: up to `stride` of the residual's steps
            int left = stride;
            while (act && left > 0) {
                const double step = (t + dt > t2) ? (t2 - t) : dt;
                Lane<Mdl>::rk4(P, sw0, sw1, t, X, step);
                t += dt;
                k++;
                act = t < (t2 - dt / 2) && k < N + 8;
                left--;
            }
            q++;
            go = act;
        }
    }

    // where the case ended: the state, the final boundary rows as the residual forms them, H with a free final time
    {
        double *out = A.Xf + T * S;
#pragma unroll
        for (int j = 0; j < S; j++) out[j] = X[j];
    }
    {
        const int *mx = pb.mode_x + M * D;
        const double *xd = pb.xnode + M * S;
        double *out = A.miss + T * NM;
#pragma unroll
        for (int j = 0; j < D; j++) {
            const bool fr = mx[j] == 1;
            out[j] = fr ? X[j + D] : X[j] - xd[j];
        }
        if constexpr (FREE_TF) out[D] = Mdl::hamiltonian(P, sw0, sw1, t2, X);
    }
    A.nupd[T] = nupd;
    A.nskip[T] = nskip;
    const bool st = A.tf != nullptr;
    if (st) A.tf[T] = t2;
    const bool sd = A.dxmax != nullptr;
    if (sd) A.dxmax[T] = dmax;
}

template <class Mdl, bool FREE_TF, bool PERPROB>
__device__ __forceinline__ void guide_body(const ModelParams &P, const ProblemDev &pb, int B, const double *__restrict__ Z,
                                           const GuideArgs &A)
{
    row_lane<PERPROB>(P, pb, B, A.K, Z, [&](const ModelParams &Pq, const ProblemDev &pq, auto, long b, int, long T) {
        guide_lane<Mdl, FREE_TF>(Pq, pq, Z + b * pb.n, b, T, A);
    });
}

// every time FIXED or interpolated (the tables of socp_gain_batch) and node M's time FREE (those of socp_gain_free_batch): two kernels
// of one launch-macro shape
template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void guide_kernel(ModelParams P, ProblemDev pb, int B,
                                                                                               const double *__restrict__ Z, GuideArgs A)
{
    static_assert(INTEG == 0, "the closed-loop flight takes the fixed steps of the tables");
    guide_body<Mdl, false, PERPROB>(P, pb, B, Z, A);
}
template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void guide_free_kernel(ModelParams P, ProblemDev pb, int B,
                                                                                                    const double *__restrict__ Z, GuideArgs A)
{
    static_assert(INTEG == 0, "the closed-loop flight takes the fixed steps of the tables");
    guide_body<Mdl, true, PERPROB>(P, pb, B, Z, A);
}

}  // namespace socp
