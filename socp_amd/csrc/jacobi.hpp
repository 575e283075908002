// jacobi.hpp -- K_jacobi: the Jacobi field test of every segment of B unknown vectors (socp_jacobi_batch; the definition is
// the comment of the entry points in include/socp_hip.h, tests/jacobi_reference.py restates it in numpy).
//
// Unlike every other lane kernel here, a trajectory does not stand alone: the D + 1 trajectories of one (row, segment) -- the
// extremal itself and one per perturbed costate component -- take identical steps, so they sit in G = D + 1 NEIGHBOURING lanes
// of one wavefront, 64 / G groups per wave (the remaining lanes idle), and everything that combines them happens in registers
// with cross-lane moves:
//   lane c of a group integrates column c (0: the extremal; c >= 1: costate component c - 1 moved by h_c)
//   at a sample the base state reaches the group by __shfl; lane c >= 1 then holds column c - 1 of J = dx(t)/dp(t0)
//   the elimination runs across the lanes: the owner of column k finds the pivot among its own D registers and broadcasts the
//   pivot row, the pivot and the multipliers; every lane swaps and updates its column with fully unrolled selects over r, so no
//   register array is ever indexed by a run-time value (no private segment: profiles/jacobi_kernel_meta.txt)
//   every lane of the group ends up with the same determinant, and carries the sign test's few scalars itself.
// The groups are group_lane's (segment_views.hpp: tail and idle lanes run a copy of the launch's last slab and store nothing).
// The loop over the SAMPLES is wave-uniform -- it runs while ANY lane has a step left; inside it every lane takes its steps up to
// its next sample in a per-lane loop of the residual's own shape, and all 64 lanes meet again before anything crosses lanes.  A
// group with fewer steps (another timeline under per-row blocks, a zero-length segment) and the tail lanes skip the inner loop
// and stay in the outer one -- so every cross-lane read is executed by all 64 lanes and reads a defined register.
// Every store site is ONE block under ONE computed predicate (see the note in segment_residual): the sample (tq, det) inside
// the loop, the slab's summary and Jend after it.  Jend is formed after the loop from the state the last step left, by the
// operations of the last sample.
#pragma once
#include "integrator.hpp"

namespace socp {

// a[r] with r a run-time index.  Bit masks, not a chain of selects between the registers: the compiler folds such a chain over an
// array it has not yet split into a load through a computed ADDRESS, and the array then lives in memory (the same hazard as
// the note in fdjac_lane_kernel)
template <int D>
__device__ __forceinline__ double jacobi_pick(const double (&a)[D], int r)
{
    long long v = 0;
#pragma unroll
    for (int q = 0; q < D; q++) v |= __double_as_longlong(a[q]) & -(long long)(r == q);
    return __longlong_as_double(v);
}

// The determinant of the D x D matrix whose column c - OFF is in registers a[0 .. D) of lane base + c (c = OFF .. OFF + D - 1) of a
// group of G lanes; the group's other lanes hold anything finite or not, they are not read.  OFF = 1, G = D + 1: the groups of
// jacobi_group_kernel (lane base is the extremal); fields.hpp has OFF = 0 or D.  Called by all 64 lanes; the result is the
// same in every lane of a group.
// Gaussian elimination with partial pivoting in the operation order of include/socp_hip.h.  `a` is destroyed.
template <int D, int OFF = 1, int G = D + 1>
__device__ __forceinline__ double jacobi_det(double (&a)[D], int base, int c)
{
    static_assert(OFF >= 0 && OFF + D <= G && G <= 64, "the columns lie inside the group");
    // not finite anywhere in the group's columns -> NaN
    bool fin = true;
#pragma unroll
    for (int r = 0; r < D; r++) fin = fin && (fabs(a[r]) <= 1.7976931348623157e308);
    const unsigned long long bad = __ballot(c >= OFF && c < OFF + D && !fin);
    const unsigned long long gmask = (G >= 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << base;
    const bool nonfinite = (bad & gmask) != 0ull;

    double det = 0.0;
    bool zero = false, odd = false;
#pragma unroll
    for (int k = 0; k < D; k++) {
        // the owner of column k: the smallest r >= k with |a[r]| maximal
        int p = k;
        double best = fabs(a[k]);
#pragma unroll
        for (int r = k + 1; r < D; r++) {
            const bool gt = fabs(a[r]) > best;
            best = gt ? fabs(a[r]) : best;
            p = gt ? r : p;
        }
        const int owner = (base + k + OFF) & 63;                      // (& 63: an idle lane behind the last group reads a lane that exists)
        p = __shfl(p, owner);
        // swap rows k and p (columns < k are finished: swapping them too changes nothing that is read again)
        const double ap = jacobi_pick<D>(a, p);
#pragma unroll
        for (int r = k + 1; r < D; r++) a[r] = (r == p) ? a[k] : a[r];
        a[k] = ap;
        odd = odd != (p != k);
        const double v = __shfl(a[k], owner);
        zero = zero || (v == 0.0);
        det = (k == 0) ? v : det * v;
        const bool mine = (c - OFF) > k;
#pragma unroll
        for (int r = k + 1; r < D; r++) {
            const double l = __shfl(a[r] / v, owner);
            const double u = a[r] - l * a[k];
            a[r] = mine ? u : a[r];
        }
    }
    det = odd ? -det : det;
    det = zero ? 0.0 : det;
    return nonfinite ? __builtin_nan("") : det;
}

template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void jacobi_group_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, double eps, int stride, int skip, int cap,
                                                             double *__restrict__ tq, double *__restrict__ det,
                                                             int *__restrict__ count, int *__restrict__ nchange,
                                                             double *__restrict__ tconj, double *__restrict__ Jend)
{
    static_assert(INTEG == 0, "the Jacobi fields follow the fixed-step integrator only");
    static_assert(!has_custom_traj<Mdl>::value, "the Jacobi fields of a model with its own ComputeTraj need a definition of their own");
    constexpr int D = Mdl::D;
    constexpr int G = D + 1;                                          // column 0 the extremal, c >= 1 costate component c - 1 moved
    static_assert(G < 64, "a group fits one wavefront");
    const GroupLane L = group_lane(B, pb.M, G);
    const double *zr = Z + L.b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    ModelParams Pq = P;
    ProblemDev pq = pb;
    if constexpr (PERPROB) load_problem_block(pb, L.b, Pq, pq);
    const int c = L.c, base = L.base;
    double X[Mdl::S];
    const SegmentSpan<Mdl> sp(Pq, pq, z, L.i, X);
    // column c: X[D + c - 1] + h_c, h_c by MINPACK's rule; x + -0.0 == x bit for bit in every other entry and in column 0
    double h = 1.0;
    {
        double xc = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) xc = (j == c - 1) ? X[D + j] : xc;
        h = c >= 1 ? fd_step(xc, eps) : 1.0;
#pragma unroll
        for (int j = 0; j < D; j++) X[D + j] = X[D + j] + ((j == c - 1) ? h : -0.0);
    }
    // the loop of Lane::integrate, its condition carried in `act`.  Spelled out here and in fields_group_kernel: with the scan handed to
    // one helper the reference-order Goddard instantiations are allocated 278 registers for 308 and run 1.8 % longer at stride 1
    const double t1 = sp.t1, t2 = sp.t2, sw0 = sp.sw0, sw1 = sp.sw1;
    const long T = L.T;
    const bool live = L.live;
    const double dt = (t2 - t1) / Pq.step_nbr;
    double t = t1;
    int guard = Pq.step_nbr + 8;
    bool act = t < (t2 - dt / 2) && guard-- > 0;
    const bool any_step = act;
    int left = stride;              // steps until the next one the stride samples
    int ns = 0;                     // samples so far (those beyond cap are counted, not stored)
    int nch = 0;
    double dprev = 0.0, tprev = 0.0, tc = __builtin_nan("");
    // one iteration per SAMPLE, wave-uniform
    while (__any(act)) {
        // the steps up to the lane's next sample: a per-lane loop like Lane::integrate's own (the lanes of a group leave it
        // together), so the steps between two samples run in a loop of the residual's shape
        bool due = false;
        double ts = t;
        while (act && !due) {
            const double step = (t + dt > t2) ? (t2 - t) : dt;
            Lane<Mdl>::rk4(Pq, sw0, sw1, t, X, step);
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
            for (int r = 0; r < D; r++) a[r] = (X[r] - __shfl(X[r], base)) / h;
            const double d1 = jacobi_det<D>(a, base, c);
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
    // J of the last sample: the state after the last step, differenced as the last sample differenced it; no step: +0.0
    double je[D];
#pragma unroll
    for (int r = 0; r < D; r++) {
        const double v = (X[r] - __shfl(X[r], base)) / h;
        je[r] = any_step ? v : 0.0;
    }
    const bool sj = live && c >= 1 && Jend != nullptr;
    if (sj) {
        double *out = Jend + T * (D * D) + (c - 1);
#pragma unroll
        for (int r = 0; r < D; r++) out[r * D] = je[r];
    }
}

}  // namespace socp

