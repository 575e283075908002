// fields.hpp -- K_fields: the exact Jacobi fields of every segment of B unknown vectors (socp_fields_batch; the definition is the
// comment of the entry points in include/socp_hip.h, tests/fields_reference.py restates it in Python).
//
// Modelled on jacobi_group_kernel (jacobi.hpp): the C columns of one (row, segment) take identical steps, so they sit in G = C
// NEIGHBOURING lanes of one wavefront (group_lane, segment_views.hpp).  Lane c carries the state as S dual
// numbers (dual.hpp): the value parts are the residual's trajectory, the same in every lane of the group, the derivative parts
// are column c of the transition matrix dX(t)/dX(t_i) -- column d + c with cols = COSTATE.  Nothing is differenced, so no base
// trajectory and no step length: the lanes only meet in the determinant, which is jacobi_det's elimination across the lanes
// that hold the costate columns (lanes base + OFF .. base + OFF + D, OFF = 0 or D).
// The loop over the SAMPLES is wave-uniform, the residual-shaped per-lane step loop sits inside it, as in jacobi_group_kernel.
// A lane holds 2 S doubles per RK4 array (five arrays): the Goddard instantiations live
// in the 264 .. 512-register step at one wave per SIMD, which is what the kernel asks for (profiles/fields_kernel_meta.txt).
//
// Also here, for this kernel, exact_jacobian.hpp and sensitivity.hpp: the RK4 step and the fixed-step loop on dual numbers.
#pragma once
#include "dual.hpp"
#include "integrator.hpp"
#include "jacobi.hpp"

namespace socp {

// Lane::rk4's reference-order arm (odeTools.cpp:89-98) on dual numbers.  TS = double: t and step are plain and take part through
// the mixed overloads of dual.hpp; TS = Dual: a DUAL step, h F the full dual product.  The right-hand side is given the value part
// of the stage time.  PV: ModelParams, or the dual view of a parameter block (sensitivity.hpp)
template <class Mdl, class PV, class TS>
__device__ __forceinline__ void dual_rk4(const PV &P, double sw0, double sw1, const TS &t, Dual (&X)[Mdl::S], const TS &step)
{
    constexpr int S = Mdl::S;
    Dual F1[S], Fs[S], F[S], Y[S];
    const TS h2 = step / 2.0;
    const TS th = t + step / 2.0;
    Mdl::template rhs_t<Dual>(P, sw0, sw1, d_val(t), X, F1);
#pragma unroll
    for (int i = 0; i < S; i++) Y[i] = X[i] + h2 * F1[i];
    Mdl::template rhs_t<Dual>(P, sw0, sw1, d_val(th), Y, Fs);          // F2
#pragma unroll
    for (int i = 0; i < S; i++) Y[i] = X[i] + h2 * Fs[i];
    Mdl::template rhs_t<Dual>(P, sw0, sw1, d_val(th), Y, F);           // F3
#pragma unroll
    for (int i = 0; i < S; i++) { Y[i] = X[i] + step * F[i]; Fs[i] = Fs[i] + F[i]; }   // F2 + F3
    Mdl::template rhs_t<Dual>(P, sw0, sw1, d_val(t + step), Y, F);     // F4
    const TS h6 = step / 6.0;
#pragma unroll
    for (int i = 0; i < S; i++) X[i] = X[i] + h6 * (F1[i] + (F[i] + 2.0 * Fs[i]));
}

// The loop of Lane::integrate with a dual end time: t1 = (t1, 0), t2 = (t2, delta) -- delta = 1.0 differentiates with respect
// to the segment's length.  The step length is a dual number; the loop condition and the clamp read value parts, so lanes with
// different delta never diverge.  step(t, h) gets both as duals.
template <class Step>
__device__ __forceinline__ void fixed_steps_dual(int step_nbr, double t1, const Dual &t2, Step &&step)
{
    const Dual dt = (t2 - Dual(t1, 0.0)) / (double)step_nbr;
    Dual t(t1, 0.0);
    int guard = step_nbr + 8;
    while (t.v < (t2.v - dt.v / 2) && guard-- > 0) {
        const Dual h = (t.v + dt.v > t2.v) ? (t2 - t) : dt;
        step(t, h);
        t = t + dt;
    }
}

// the dual start state (X0, e_k) of the column that differentiates with respect to entry k of X0; k < 0: (X0, +0.0)
template <int S>
__device__ __forceinline__ void dual_start(const double (&X0)[S], int k, Dual (&X)[S])
{
#pragma unroll
    for (int j = 0; j < S; j++) X[j] = Dual(X0[j], j == k ? 1.0 : 0.0);
}

// ALL = false: SOCP_FIELDS_COSTATE (C = D columns), ALL = true: SOCP_FIELDS_ALL (C = S columns)
template <class Mdl, bool ALL, bool PERPROB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void fields_group_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, int stride, int skip, int cap,
                                                             double *__restrict__ tq, double *__restrict__ det,
                                                             int *__restrict__ count, int *__restrict__ nchange,
                                                             double *__restrict__ tconj, double *__restrict__ Phi)
{
    static_assert(!has_custom_traj<Mdl>::value, "the fields of a model with its own ComputeTraj need a definition of their own");
    constexpr int S = Mdl::S;
    constexpr int D = Mdl::D;
    constexpr int G = ALL ? S : D;                                    // = C: one lane per column
    constexpr int OFF = ALL ? D : 0;                                  // the group's lane of costate column 0
    static_assert(G <= 64, "a group fits one wavefront");
    const GroupLane L = group_lane(B, pb.M, G);
    const double *zr = Z + L.b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    ModelParams Pq = P;
    ProblemDev pq = pb;
    if constexpr (PERPROB) load_problem_block(pb, L.b, Pq, pq);
    const int c = L.c;
    double X0[S];
    const SegmentSpan<Mdl> sp(Pq, pq, z, L.i, X0);
    Dual X[S];
    dual_start(X0, ALL ? c : D + c, X);                           // the unit vector this column starts from
    // the loop of Lane::integrate, its condition carried in `act` (the scan of jacobi_group_kernel; see the note there)
    const int base = L.base;
    const long T = L.T;
    const bool live = L.live;
    const double t1 = sp.t1, t2 = sp.t2, sw0 = sp.sw0, sw1 = sp.sw1;
    const double dt = (t2 - t1) / Pq.step_nbr;
    double t = t1;
    int guard = Pq.step_nbr + 8;
    bool act = t < (t2 - dt / 2) && guard-- > 0;
    int left = stride;              // steps until the next one the stride samples
    int ns = 0;                     // samples so far (those beyond cap are counted, not stored)
    int nch = 0;
    double dprev = 0.0, tprev = 0.0, tc = __builtin_nan("");
    // one iteration per SAMPLE, wave-uniform
    while (__any(act)) {
        bool due = false;
        double ts = t;
        while (act && !due) {
            const double step = (t + dt > t2) ? (t2 - t) : dt;
            dual_rk4<Mdl>(Pq, sw0, sw1, t, X, step);
            ts = t + step;
            t += dt;
            act = t < (t2 - dt / 2) && guard-- > 0;
            due = --left == 0 || !act;
        }
        left = left == 0 ? stride : left;
        // every lane is back here: the cross-lane reads below are executed by all 64
        if (__any(due)) {
            double a[D];
#pragma unroll
            for (int r = 0; r < D; r++) a[r] = X[r].d;
            const double d1 = jacobi_det<D, OFF, G>(a, base, c);
            const bool st = due && live && c == 0 && ns < cap;
            if (st) {
                tq[T * cap + ns] = ts;
                det[T * cap + ns] = d1;
            }
            // consecutive samples ns - 1, ns with ns - 1 >= skip
            const bool cmp = due && ns >= 1 && ns - 1 >= skip && dprev == dprev && d1 == d1 && (dprev < 0.0) != (d1 < 0.0);
            const double cand = tprev + (ts - tprev) * (dprev / (dprev - d1));
            tc = (cmp && nch == 0) ? cand : tc;
            nch += cmp ? 1 : 0;
            dprev = due ? d1 : dprev;
            tprev = due ? ts : tprev;
            ns += due ? 1 : 0;
        }
    }

    const bool sm = live && c == 0;
    if (sm) {
        count[T] = ns;
        nchange[T] = nch;
        tconj[T] = tc;
    }
    // column c of the transition matrix after the last step; no step: the unit column it started from
    const bool st = L.live && Phi != nullptr;
    if (st) {
        double *out = Phi + L.T * (S * G) + c;
#pragma unroll
        for (int r = 0; r < S; r++) out[r * G] = X[r].d;
    }
}

}  // namespace socp
