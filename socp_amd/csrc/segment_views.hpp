// segment_views.hpp -- the kernels that LOOK at the segments the residual integrates without being on the solver's path: the dense
// trace of one trajectory and, for a whole batch of unknown vectors, trace, extrema, observables, cost, events and Move(tf) / re-grid.
// Included at the end of integrator.hpp, which brings Lane, the traits and the segment prologue (Timeline / segment_start).
//
// The pieces every such kernel is made of exist once, here (the group kernels of jacobi.hpp, fields.hpp, exact_jacobian.hpp and
// sensitivity.hpp use them too).  Where a helper moved an instantiation's spills or scratch upwards the text it would replace
// stays, with a comment at the place (profiles/segment_views_kernel_meta.txt):
//   row_lane                which (row, item) a lane owns, its z reader and its view of (P, pb) under per-row blocks
//   group_lane              the same for a group of neighbouring lanes per (row, segment)
//   SegmentSpan             t1, t2, the two auxiliary scalars and the start state of segment i: the residual's own prologue
//   walk_rows               every row the trace keeps at stride 1, in order
// The rules they keep: every store site is ONE block under ONE computed predicate (see the note in segment_residual), and no
// register array is indexed by a run-time value.
#pragma once
#include "integrator.hpp"

namespace socp {

// One lane = (row b, item w of W per row), T = b W + w; the lanes past B W leave.  body(Pq, pq, z, b, w, T): z reads row b's
// unknowns, (Pq, pq) are (P, pb) or, under PERPROB, row b's own blocks (dev_common.hpp load_problem_block) -- a separate
// instantiation, so the shared-parameter kernels keep their parameters in scalar registers.
template <bool PERPROB, class Body>
__device__ __forceinline__ void row_lane(const ModelParams &P, const ProblemDev &pb, int B, int W, const double *Z, Body &&body)
{
    const long T = (long)blockIdx.x * 64 + threadIdx.x;
    if (T >= (long)B * W) return;
    const long b = T / W;
    const int w = (int)(T - b * W);
    const double *zr = Z + b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    if constexpr (PERPROB) {
        ModelParams Pq = P;
        ProblemDev pq = pb;
        load_problem_block(pb, b, Pq, pq);
        body(Pq, pq, z, b, w, T);
    } else {
        body(P, pb, z, b, w, T);
    }
}

// One GROUP of G neighbouring lanes = (row b, segment i), 64 / G groups per wave, T = b M + i; lane c of the group is its column.
// The lanes behind the last group of a wave and the groups past B M are not live: they run a copy of the launch's last slab and
// store nothing, so that every cross-lane read that follows is executed by all 64 lanes and reads a defined register -- a kernel
// never returns on `live`.  G may be a run-time value (sensitivity_kernel's is).
// The z reader and the always-copied (Pq, pq) stay with the kernels: handed to a body through this helper the parameter block
// is read at the top of the kernel, and the Goddard instantiations of fields_group_kernel go 12 bytes into scratch.
struct GroupLane {
    int g, c, base;             // the group, the lane's column in it, the group's first lane
    bool live;
    long T, b;                  // T clamped to the last slab when not live
    int i;
};
__device__ __forceinline__ GroupLane group_lane(int B, int M, int G)
{
    const int gpw = 64 / G;                                           // groups per wavefront
    const int lane = threadIdx.x;
    GroupLane L;
    L.g = lane / G;
    L.c = lane - L.g * G;
    L.base = lane - L.c;
    const long total = (long)B * M;
    const long Tl = (long)blockIdx.x * gpw + L.g;
    L.live = L.g < gpw && Tl < total;
    L.T = L.live ? Tl : total - 1;
    L.b = L.T / M;
    L.i = (int)(L.T - L.b * M);
    return L;
}

// What a view of segment i starts from: its timeline entries, the model's two auxiliary scalars and, in X, its start state
// z[S i .. S i + S) -- the prologue of segment_residual (Timeline / segment_start), so that the segment viewed IS the segment the
// residual integrates.  For the kernels that are not hot: segment_residual keeps its own text (see the note above Timeline).
// X stays the caller's own array: as a member of this struct the state is no longer vectorised the way the residual's is, and
// the Goddard extrema kernels spill more.
template <class Mdl>
struct SegmentSpan {
    double t1, t2, sw0, sw1;
    template <class ZRead>
    __device__ __forceinline__ SegmentSpan(const ModelParams &P, const ProblemDev &pb, const ZRead &z, int i, double (&X)[Mdl::S])
    {
        const Timeline<ZRead> tl{pb, z};
        t1 = tl.nt(i);
        t2 = tl.nt(i + 1);
        sw0 = tl.template switching_time<Mdl>(P.sw0, pb.sw_node0);
        sw1 = tl.template switching_time<Mdl>(P.sw1, pb.sw_node1);
        segment_start(z, Mdl::S * i, X);
    }
};

// The rows of a trajectory t1 -> t2 from X, each shown to row(t, X, aux0, aux1) once and in order -- THE definition of "the rows
// the trace keeps with stride 1", for every kernel that stores or reduces them.  Row 0 is (t1, X_start); row k the accumulated
// time and the state after k steps of the loop the residual runs (the observer form of integrate, odeTools.cpp:103-123; with
// INTEG == 1 the end of the k-th accepted step of the adaptive integrator).  A kCustomTraj model shows the rows its own ComputeTraj
// traces, then one more: the state as ComputeTraj returns it (back in the model's default chart) and the flags it leaves, at t2.
// X, sw0 and sw1 are left as the integration leaves them.
template <class Mdl, int INTEG, class Row>
__device__ __forceinline__ void walk_rows(const ModelParams &P, double &sw0, double &sw1, double t1, double t2, double (&X)[Mdl::S],
                                          Row &&row)
{
    if constexpr (has_custom_traj<Mdl>::value) {
        Mdl::template compute_traj<INTEG>(P, sw0, sw1, t1, t2, X, row);
        row(t2, X, sw0, sw1);
    } else {
        row(t1, X, sw0, sw1);
        auto after = [&](double t, const double (&Xr)[Mdl::S]) { row(t, Xr, sw0, sw1); };
        if constexpr (INTEG == 1) Lane<Mdl>::integrate_dopri5(P, sw0, sw1, t1, t2, X, NoStepHook(), after);
        else Lane<Mdl>::integrate(P, sw0, sw1, t1, t2, X, after);
    }
}

// K_dense: ONE trajectory with the state after every step kept (trace replay, shooting.cpp:496-544): the rows of walk_rows --
// exactly what the reference's observer is shown -- with the two auxiliary scalars of each row in aux[row][2] (may be null).
// The rows beyond cap are counted, not stored -- row 0 too, which the text before walk_rows stored unconditionally (the host
// refuses cap < 1, so no call sees the difference).  Not hot.
template <class Mdl, int INTEG = 0>
__global__ __launch_bounds__(64) void traj_dense_kernel(ModelParams P, double t0, double tf, double sw0, double sw1,
                                  const double *__restrict__ X0, double *__restrict__ dense,
                                  double *__restrict__ times, int cap, int *__restrict__ rows, double *__restrict__ aux)
{
    constexpr int S = Mdl::S;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double X[S];
#pragma unroll
    for (int k = 0; k < S; k++) X[k] = X0[k];
    int r = 0;
    walk_rows<Mdl, INTEG>(P, sw0, sw1, t0, tf, X, [&](double t, const double (&Xr)[S], double b0, double b1) {
        if (r < cap) {
#pragma unroll
            for (int k = 0; k < S; k++) dense[(long)r * S + k] = Xr[k];
            times[r] = t;
            if (aux) { aux[2 * r] = b0; aux[2 * r + 1] = b1; }
        }
        r++;
    });
    *rows = r;
}

// ---------------------------------------------------------------------------------------------
// K_trace: the sampled trace rows of every segment of B unknown vectors (shooting::Trace, shooting.cpp:496-544, for a
// whole batch).  Z[B][n] -> rows[B][M][cap][W], count[B][M];  W = 1 + S + NU + 1 + 2:  t, X[S], u[NU], H, aux0, aux1.
// One lane = (row, segment) (row_lane, direct stores) walks the rows of its segment (SegmentSpan, walk_rows), so row k is what
// traj_dense_kernel reports for that segment, and row k is KEPT iff k % stride == 0 or it is the last one.  This launch stores
// t, X and the aux pair of the kept rows; trace_fill_kernel adds u and H, one lane per kept row, which keeps control_only /
// hamiltonian out of this kernel's register budget.
// A lane carries across the integration only two counters and the last row's time beside what the residual lane carries; the row
// address is formed from them at the store.  A kept row is W consecutive doubles and a segment's rows are adjacent.
// An adaptive trajectory that fails (NaN result, integrate_dopri5) has no row for the failed step: its last row
// reports the NaN state, unless the stride had already kept the last accepted step.
// ---------------------------------------------------------------------------------------------
template <class Mdl>
constexpr int trace_width() { return 1 + Mdl::S + Mdl::NU + 1 + 2; }

template <class Mdl, int INTEG, class ZRead>
__device__ __forceinline__ void segment_trace(const ModelParams &P, const ProblemDev &pb, const ZRead &z, int i,
                                              int stride, int cap, double *__restrict__ slab, int *__restrict__ count)
{
    constexpr int S = Mdl::S;
    constexpr int W = trace_width<Mdl>();
    double X[S];
    SegmentSpan<Mdl> sp(P, pb, z, i, X);

    int kept = 0;       // rows kept so far (those beyond cap are counted, not stored)
    int left = 1;       // rows until the next one the stride keeps; == stride right after a kept row
    double tlast = sp.t1;
    auto put = [&](bool want, double t, const double (&Xr)[S], double b0, double b1) {
        const bool st = want && kept < cap;
        if (st) {
            double *row = slab + (long)kept * W;
            row[0] = t;
#pragma unroll
            for (int k = 0; k < S; k++) row[1 + k] = Xr[k];
            row[W - 2] = b0;
            row[W - 1] = b1;
        }
        kept += want ? 1 : 0;
    };
    auto sample = [&](double t, const double (&Xr)[S], double b0, double b1) {
        const bool due = --left == 0;
        put(due, t, Xr, b0, b1);
        left = due ? stride : left;
        tlast = t;
    };
    if constexpr (has_custom_traj<Mdl>::value) {
        // walk_rows' own first arm, spelled out (through the helper the interceptor's adaptive instantiations spill more); its
        // extra row is the last: always kept
        Mdl::template compute_traj<INTEG>(P, sp.sw0, sp.sw1, sp.t1, sp.t2, X, sample);
        put(true, sp.t2, X, sp.sw0, sp.sw1);
    } else {
        walk_rows<Mdl, INTEG>(P, sp.sw0, sp.sw1, sp.t1, sp.t2, X, sample);
        put(left != stride, tlast, X, sp.sw0, sp.sw1);                   // the last row, when the stride passed over it
    }
    *count = kept;
}

template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void trace_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                           const double *__restrict__ Z, int stride, int cap,
                                                           double *__restrict__ rows, int *__restrict__ count)
{
    row_lane<PERPROB>(P, pb, B, pb.M, Z, [&](const ModelParams &Pq, const ProblemDev &pq, auto z, long, int i, long T) {
        segment_trace<Mdl, INTEG>(Pq, pq, z, i, stride, cap, rows + T * cap * trace_width<Mdl>(), count + T);
    });
}

// ---------------------------------------------------------------------------------------------
// K_extrema: per-segment extrema over the rows K_trace keeps with stride = 1 (socp_extrema_batch), without the rows ever
// leaving the lane.  Z[B][n] -> vmin, vmax, tmin, tmax [B][M][C], count[B][M], nbad[B][M];  C = S + NU + 1 + EC:  X[S], u[NU],
// H, g[EC] (EC = the model's event channels when its table has an events entry, else 0).  One lane = (row, segment), T = b M + i,
// walks the rows of its segment (SegmentSpan, walk_rows): the rows reduced are the rows traced.  On every row it evaluates
// control_only / hamiltonian / event_fn at the row's (t, X) with the row's aux pair -- what K_trace_fill evaluates -- and updates
// the running (value, time) pairs, which live in registers beside the state:
//     row 0:  vmin = vmax = v, tmin = tmax = t;   later:  if (v < vmin) { vmin = v; tmin = t; }  if (v > vmax) { vmax = v; tmax = t; }
// (strict comparisons: the first attainment wins, -0.0 never displaces +0.0, a NaN never displaces anything and a NaN in row 0
// stays).  nbad = rows in which a selected channel is not finite.
// FULL = false: the state channels only -- the lane carries neither u, H, g nor their 4 (NU + 1 + EC) running doubles.
// FULL = true: every channel is reduced; the bits of `what` (1: u, 2: H, 4: g) select which groups count for nbad and are stored.
// The C-wide results leave once, at the end; a lane's C doubles are consecutive and consecutive lanes own adjacent spans.
// ---------------------------------------------------------------------------------------------
template <class Mdl>
constexpr int extrema_event_channels() { return has_custom_traj<Mdl>::value ? 0 : event_channels<Mdl>::value; }
template <class Mdl>
constexpr int extrema_width() { return Mdl::S + Mdl::NU + 1 + extrema_event_channels<Mdl>(); }

template <class Mdl, int INTEG, bool FULL, class ZRead>
__device__ __forceinline__ void segment_extrema(const ModelParams &P, const ProblemDev &pb, const ZRead &z, int i, int what,
                                                double *__restrict__ vmin, double *__restrict__ vmax, double *__restrict__ tmin,
                                                double *__restrict__ tmax, int *__restrict__ count, int *__restrict__ nbad)
{
    constexpr int S = Mdl::S, NU = Mdl::NU, EC = extrema_event_channels<Mdl>();
    constexpr int L = FULL ? extrema_width<Mdl>() : S;          // channels this instantiation carries
    double X[S];
    SegmentSpan<Mdl> sp(P, pb, z, i, X);

    const bool wu = (what & 1) != 0, wh = (what & 2) != 0, wg = (what & 4) != 0;
    double lo[L], hi[L], tlo[L], thi[L];
#pragma unroll
    for (int c = 0; c < L; c++) lo[c] = hi[c] = tlo[c] = thi[c] = 0.0;     // row 0 overwrites them
    int rows = 0, bad = 0;
    auto finite = [](double v) { return fabs(v) <= 1.7976931348623157e308; };      // false for NaN and the infinities
    auto row = [&](double t, const double (&Xr)[S], double b0, double b1) {
        double v[L];
#pragma unroll
        for (int k = 0; k < S; k++) v[k] = Xr[k];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < S; k++) ok = ok && finite(v[k]);
        if constexpr (FULL) {
            double u[3];
            Mdl::control_only(P, b0, b1, t, Xr, u);
#pragma unroll
            for (int k = 0; k < NU; k++) { v[S + k] = u[k]; ok = ok && (!wu || finite(u[k])); }
            v[S + NU] = Mdl::hamiltonian(P, b0, b1, t, Xr);
            ok = ok && (!wh || finite(v[S + NU]));
            if constexpr (EC > 0) {
#pragma unroll
                for (int c = 0; c < EC; c++) {
                    v[S + NU + 1 + c] = Mdl::event_fn(P, b0, b1, t, Xr, c);
                    ok = ok && (!wg || finite(v[S + NU + 1 + c]));
                }
            }
        }
        const bool first = rows == 0;
#pragma unroll
        for (int c = 0; c < L; c++) {
            const bool dn = first || v[c] < lo[c], up = first || v[c] > hi[c];
            lo[c] = dn ? v[c] : lo[c];
            tlo[c] = dn ? t : tlo[c];
            hi[c] = up ? v[c] : hi[c];
            thi[c] = up ? t : thi[c];
        }
        bad += ok ? 0 : 1;
        rows++;
    };
    if constexpr (has_custom_traj<Mdl>::value) {
        // walk_rows' own first arm, spelled out (through the helper the interceptor's state-only instantiations spill more)
        Mdl::template compute_traj<INTEG>(P, sp.sw0, sp.sw1, sp.t1, sp.t2, X, row);
        row(sp.t2, X, sp.sw0, sp.sw1);
    } else {
        walk_rows<Mdl, INTEG>(P, sp.sw0, sp.sw1, sp.t1, sp.t2, X, row);
    }

    // channels [c0, c1) of the four arrays, each under its own predicate
    // (compile-time bounds: the running pairs are registers, never indexed by a variable)
    auto store = [&](bool sel, auto c0, auto c1) {
        if (sel) {
#pragma unroll
            for (int c = c0(); c < c1(); c++) { vmin[c] = lo[c]; vmax[c] = hi[c]; }
        }
        const bool sa = sel && tmin != nullptr;
        if (sa) {
#pragma unroll
            for (int c = c0(); c < c1(); c++) tmin[c] = tlo[c];
        }
        const bool sb = sel && tmax != nullptr;
        if (sb) {
#pragma unroll
            for (int c = c0(); c < c1(); c++) tmax[c] = thi[c];
        }
    };
    using std::integral_constant;
    store(true, integral_constant<int, 0>(), integral_constant<int, S>());
    if constexpr (FULL) {
        store(wu, integral_constant<int, S>(), integral_constant<int, S + NU>());
        store(wh, integral_constant<int, S + NU>(), integral_constant<int, S + NU + 1>());
        if constexpr (EC > 0) store(wg, integral_constant<int, S + NU + 1>(), integral_constant<int, S + NU + 1 + EC>());
    }
    *count = rows;
    const bool sn = nbad != nullptr;
    if (sn) *nbad = bad;
}

template <class Mdl, int INTEG, bool PERPROB, bool FULL>
__device__ __forceinline__ void extrema_lane(const ModelParams &P, const ProblemDev &pb, int B, const double *__restrict__ Z, int what,
                                             double *__restrict__ vmin, double *__restrict__ vmax, double *__restrict__ tmin,
                                             double *__restrict__ tmax, int *__restrict__ count, int *__restrict__ nbad)
{
    constexpr int C = extrema_width<Mdl>();
    // row_lane spelled out: through the helper the interceptor's adaptive instantiation with per-row blocks goes 8 bytes deeper into scratch
    const long T = (long)blockIdx.x * 64 + threadIdx.x;              // = b * M + i: index into count / nbad, span of the four arrays
    if (T >= (long)B * pb.M) return;
    const long b = T / pb.M;
    const int i = (int)(T - b * pb.M);
    const double *zr = Z + b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    double *ta = tmin ? tmin + T * C : nullptr, *tb = tmax ? tmax + T * C : nullptr;
    int *nb = nbad ? nbad + T : nullptr;
    if constexpr (PERPROB) {
        ModelParams Pq = P;
        ProblemDev pq = pb;
        load_problem_block(pb, b, Pq, pq);
        segment_extrema<Mdl, INTEG, FULL>(Pq, pq, z, i, what, vmin + T * C, vmax + T * C, ta, tb, count + T, nb);
    } else {
        segment_extrema<Mdl, INTEG, FULL>(P, pb, z, i, what, vmin + T * C, vmax + T * C, ta, tb, count + T, nb);
    }
}

// every channel (what != 0) and the state channels only (what == 0): two kernels of one launch-macro shape
template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void extrema_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, int what, double *__restrict__ vmin,
                                                             double *__restrict__ vmax, double *__restrict__ tmin,
                                                             double *__restrict__ tmax, int *__restrict__ count, int *__restrict__ nbad)
{
    extrema_lane<Mdl, INTEG, PERPROB, true>(P, pb, B, Z, what, vmin, vmax, tmin, tmax, count, nbad);
}
template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void extrema_state_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, double *__restrict__ vmin,
                                                             double *__restrict__ vmax, double *__restrict__ tmin,
                                                             double *__restrict__ tmax, int *__restrict__ count, int *__restrict__ nbad)
{
    extrema_lane<Mdl, INTEG, PERPROB, false>(P, pb, B, Z, 0, vmin, vmax, tmin, tmax, count, nbad);
}

// ---------------------------------------------------------------------------------------------
// K_observe: extrema and integrals of the model's observables over the rows K_trace keeps with stride = 1 (socp_observe_batch).
// Z[B][n] -> ymin, ymax, tmin, tmax, integral [B][M][NO], count[B][M], nbad[B][M];  NO = the model's kObservables.  One lane =
// (row, segment), T = b M + i, walks the rows of its segment (SegmentSpan, walk_rows): the rows observed are the rows traced.  On
// every row it evaluates control_only once at the row's (t, X) with the row's aux pair -- what K_trace_fill evaluates -- hands
// (t, X, u) to the model's observe() and updates, per observable y, in registers beside the state:
//     row 0:  ymin = ymax = y, tmin = tmax = t, I = +0.0
//     later:  if (y < ymin) { ymin = y; tmin = t; }  if (y > ymax) { ymax = y; tmax = t; }
//             w = t - t_prev;  s = y + y_prev;  I = I + (0.5 w) s            (composite trapezoid, one rounding per operation)
// (strict comparisons, as in segment_extrema; a value that is not finite enters the sum).  nbad = rows in which an observable is not finite.  The NO-wide results leave once,
// at the end.
// ---------------------------------------------------------------------------------------------
template <class Mdl, int INTEG, class ZRead>
__device__ __forceinline__ void segment_observe(const ModelParams &P, const ProblemDev &pb, const ZRead &z, int i,
                                                double *__restrict__ ymin, double *__restrict__ ymax, double *__restrict__ tmin,
                                                double *__restrict__ tmax, double *__restrict__ integral, int *__restrict__ count,
                                                int *__restrict__ nbad)
{
    static_assert(!has_custom_traj<Mdl>::value, "the observables of a model with its own ComputeTraj need a definition of their own");
    constexpr int S = Mdl::S, NU = Mdl::NU, NO = observables<Mdl>::value;
    double X[S];
    SegmentSpan<Mdl> sp(P, pb, z, i, X);

    double lo[NO], hi[NO], tlo[NO], thi[NO], sum[NO], prev[NO];
#pragma unroll
    for (int c = 0; c < NO; c++) lo[c] = hi[c] = tlo[c] = thi[c] = sum[c] = prev[c] = 0.0;     // row 0 overwrites all but the sum
    double tprev = 0.0;
    int rows = 0, bad = 0;
    auto finite = [](double v) { return fabs(v) <= 1.7976931348623157e308; };      // false for NaN and the infinities
    walk_rows<Mdl, INTEG>(P, sp.sw0, sp.sw1, sp.t1, sp.t2, X, [&](double t, const double (&Xr)[S], double b0, double b1) {
        double u3[3], u[NU], y[NO];
        Mdl::control_only(P, b0, b1, t, Xr, u3);
#pragma unroll
        for (int k = 0; k < NU; k++) u[k] = u3[k];
        Mdl::observe(P, b0, b1, t, Xr, u, y);
        const bool first = rows == 0;
        const double hw = 0.5 * (t - tprev);
        bool ok = true;
#pragma unroll
        for (int c = 0; c < NO; c++) {
            ok = ok && finite(y[c]);
            const bool dn = first || y[c] < lo[c], up = first || y[c] > hi[c];
            lo[c] = dn ? y[c] : lo[c];
            tlo[c] = dn ? t : tlo[c];
            hi[c] = up ? y[c] : hi[c];
            thi[c] = up ? t : thi[c];
            const double s = y[c] + prev[c];
            const double next = sum[c] + hw * s;
            sum[c] = first ? 0.0 : next;
            prev[c] = y[c];
        }
        tprev = t;
        bad += ok ? 0 : 1;
        rows++;
    });

#pragma unroll
    for (int c = 0; c < NO; c++) { ymin[c] = lo[c]; ymax[c] = hi[c]; }
    const bool sa = tmin != nullptr;
    if (sa) {
#pragma unroll
        for (int c = 0; c < NO; c++) tmin[c] = tlo[c];
    }
    const bool sb = tmax != nullptr;
    if (sb) {
#pragma unroll
        for (int c = 0; c < NO; c++) tmax[c] = thi[c];
    }
    const bool si = integral != nullptr;
    if (si) {
#pragma unroll
        for (int c = 0; c < NO; c++) integral[c] = sum[c];
    }
    *count = rows;
    const bool sn = nbad != nullptr;
    if (sn) *nbad = bad;
}

template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void observe_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, double *__restrict__ ymin,
                                                             double *__restrict__ ymax, double *__restrict__ tmin,
                                                             double *__restrict__ tmax, double *__restrict__ integral,
                                                             int *__restrict__ count, int *__restrict__ nbad)
{
    constexpr int NO = observables<Mdl>::value;
    // row_lane spelled out: through the helper the throughput flavour's adaptive Goddard instantiation with per-row blocks spills more
    const long T = (long)blockIdx.x * 64 + threadIdx.x;              // = b * M + i: index into count / nbad, span of the five arrays
    if (T >= (long)B * pb.M) return;
    const long b = T / pb.M;
    const int i = (int)(T - b * pb.M);
    const double *zr = Z + b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    double *ta = tmin ? tmin + T * NO : nullptr, *tb = tmax ? tmax + T * NO : nullptr, *in = integral ? integral + T * NO : nullptr;
    int *nb = nbad ? nbad + T : nullptr;
    if constexpr (PERPROB) {
        ModelParams Pq = P;
        ProblemDev pq = pb;
        load_problem_block(pb, b, Pq, pq);
        segment_observe<Mdl, INTEG>(Pq, pq, z, i, ymin + T * NO, ymax + T * NO, ta, tb, in, count + T, nb);
    } else {
        segment_observe<Mdl, INTEG>(P, pb, z, i, ymin + T * NO, ymax + T * NO, ta, tb, in, count + T, nb);
    }
}

// K_trace_fill: u and H of every stored row, in place; one lane = (row b, segment i, kept row k), the rows at or beyond
// min(count, cap) untouched.  Evaluated like eval_lane_kernel evaluates them: at the row's (t, X) with the row's aux pair.
template <class Mdl, bool PERPROB>
__global__ __launch_bounds__(64) void trace_fill_kernel(ModelParams P, ProblemDev pb, int B, int cap,
                                                        double *__restrict__ rows, const int *__restrict__ count)
{
    constexpr int S = Mdl::S;
    constexpr int W = trace_width<Mdl>();
    const long T = (long)blockIdx.x * 64 + threadIdx.x;              // = (b * M + i) * cap + k
    if (T >= (long)B * pb.M * cap) return;
    const long seg = T / cap;
    const int k = (int)(T - seg * cap);
    if (k >= count[seg]) return;
    double *row = rows + T * W;
    double X[S];
#pragma unroll
    for (int j = 0; j < S; j++) X[j] = row[1 + j];
    const double t = row[0], a0 = row[W - 2], a1 = row[W - 1];
    double u[3];
    double H;
    if constexpr (PERPROB) {
        ModelParams Pq = P;
        ProblemDev pq = pb;
        load_problem_block(pb, seg / pb.M, Pq, pq);
        Mdl::control_only(Pq, a0, a1, t, X, u);
        H = Mdl::hamiltonian(Pq, a0, a1, t, X);
    } else {
        Mdl::control_only(P, a0, a1, t, X, u);
        H = Mdl::hamiltonian(P, a0, a1, t, X);
    }
#pragma unroll
    for (int j = 0; j < Mdl::NU; j++) row[1 + S + j] = u[j];
    row[1 + S + Mdl::NU] = H;
}

// ---------------------------------------------------------------------------------------------
// K_cost: the integrated running cost of every segment of B unknown vectors (socp_cost_batch).  Z[B][n] -> cost[B][M],
// optionally the segments' end states Xend[B][M][S].  One lane = (row, segment) (row_lane) takes the residual's fixed steps over
// its segment (SegmentSpan, integrate_cost) with q' = L = H - <p, f_x> beside the state, q = 0.0 at the segment's start.  A
// zero-length or backward segment takes no step: cost +0.0, end state = start state.
// Fixed-step RK4 only, and no model with its own ComputeTraj (its chart changes rewrite the costate in mid-trajectory).
// Consecutive lanes store consecutive doubles of cost.
// ---------------------------------------------------------------------------------------------
// Every in-tree Hamiltonian has the form H = L + <p, f_x>, so the running cost at a stage (t, Y) with F = rhs(t, Y) is
// L = H(t, Y) - sum_k Y[D+k] F[k], the sum taken left to right.  The difference carries an absolute rounding error of the
// order of eps |p . f| per evaluation.
template <class Mdl>
__device__ __forceinline__ double lagrangian(const ModelParams &P, double sw0, double sw1, double t, const double (&Y)[Mdl::S],
                                             const double (&F)[Mdl::S])
{
    constexpr int D = Mdl::D;
    double s = Y[D] * F[0];
#pragma unroll
    for (int k = 1; k < D; k++) s = s + Y[D + k] * F[k];
    return Mdl::hamiltonian(P, sw0, sw1, t, Y) - s;
}

// Lane::rk4 with the quadrature: the state update is the one of rk4(), expression for expression, and
// q + (step/6.0)*(L1 + (L4 + 2.0*(L2 + L3))) is the same rule applied to L.  A copy, not a hook into rk4(): the hot kernels
// keep their code.
template <class Mdl>
__device__ __forceinline__ void rk4_cost(const ModelParams &P, double sw0, double sw1, double t, double (&X)[Mdl::S], double step,
                                         double &q)
{
    constexpr int S = Mdl::S;
    if constexpr (Mdl::kRefOrder) {
        double F1[S], Fs[S], F[S], Y[S];
        const double h2 = step / 2.0;
        const double th = t + step / 2.0;
        Mdl::rhs(P, sw0, sw1, t, X, F1);
        const double L1 = lagrangian<Mdl>(P, sw0, sw1, t, X, F1);
#pragma unroll
        for (int i = 0; i < S; i++) Y[i] = X[i] + h2 * F1[i];
        Mdl::rhs(P, sw0, sw1, th, Y, Fs);                 // F2
        double Ls = lagrangian<Mdl>(P, sw0, sw1, th, Y, Fs);   // L2
#pragma unroll
        for (int i = 0; i < S; i++) Y[i] = X[i] + h2 * Fs[i];
        Mdl::rhs(P, sw0, sw1, th, Y, F);                  // F3
        Ls = Ls + lagrangian<Mdl>(P, sw0, sw1, th, Y, F);      // L2 + L3
#pragma unroll
        for (int i = 0; i < S; i++) { Y[i] = X[i] + step * F[i]; Fs[i] = Fs[i] + F[i]; }   // F2 + F3
        Mdl::rhs(P, sw0, sw1, t + step, Y, F);            // F4
        const double L4 = lagrangian<Mdl>(P, sw0, sw1, t + step, Y, F);
        const double h6 = step / 6.0;
#pragma unroll
        for (int i = 0; i < S; i++) X[i] = X[i] + h6 * (F1[i] + (F[i] + 2.0 * Fs[i]));
        q = q + h6 * (L1 + (L4 + 2.0 * Ls));
    } else {
        // throughput flavour: the running sums of rk4(), and one more for L
        double A[S], F[S], Y[S];
        const double h2 = 0.5 * step;
        const double th = t + h2;
        Mdl::rhs(P, sw0, sw1, t, X, A);
        double LA = lagrangian<Mdl>(P, sw0, sw1, t, X, A);
#pragma unroll
        for (int i = 0; i < S; i++) Y[i] = X[i] + h2 * A[i];
        Mdl::rhs(P, sw0, sw1, th, Y, F);
        LA = LA + 2.0 * lagrangian<Mdl>(P, sw0, sw1, th, Y, F);
#pragma unroll
        for (int i = 0; i < S; i++) { Y[i] = X[i] + h2 * F[i]; A[i] = A[i] + 2.0 * F[i]; }
        Mdl::rhs(P, sw0, sw1, th, Y, F);
        LA = LA + 2.0 * lagrangian<Mdl>(P, sw0, sw1, th, Y, F);
#pragma unroll
        for (int i = 0; i < S; i++) { Y[i] = X[i] + step * F[i]; A[i] = A[i] + 2.0 * F[i]; }
        Mdl::rhs(P, sw0, sw1, t + step, Y, F);
        LA = LA + lagrangian<Mdl>(P, sw0, sw1, t + step, Y, F);
        const double h6 = step * (1.0 / 6.0);
#pragma unroll
        for (int i = 0; i < S; i++) X[i] = X[i] + h6 * (A[i] + F[i]);
        q = q + h6 * LA;
    }
}

// the loop of Lane::integrate around rk4_cost(): the steps are the steps the residual takes.  Spelled out: with the step handed to a
// shared loop helper the throughput flavour's Goddard kernel ran 1.0 % longer
template <class Mdl>
__device__ __forceinline__ void integrate_cost(const ModelParams &P, double sw0, double sw1, double t0, double tf, double (&X)[Mdl::S],
                                               double &q)
{
    const double dt = (tf - t0) / P.step_nbr;
    double t = t0;
    int guard = P.step_nbr + 8;
    while (t < (tf - dt / 2) && guard-- > 0) {
        const double step = (t + dt > tf) ? (tf - t) : dt;
        rk4_cost<Mdl>(P, sw0, sw1, t, X, step, q);
        t += dt;
    }
}

template <class Mdl, class ZRead>
__device__ __forceinline__ void segment_cost(const ModelParams &P, const ProblemDev &pb, const ZRead &z, int i,
                                             double *__restrict__ cost, double *__restrict__ xend)
{
    static_assert(!has_custom_traj<Mdl>::value, "the running cost of a model with its own ComputeTraj needs a definition of its own");
    constexpr int S = Mdl::S;
    double X[S];
    const SegmentSpan<Mdl> sp(P, pb, z, i, X);
    double q = 0.0;
    integrate_cost<Mdl>(P, sp.sw0, sp.sw1, sp.t1, sp.t2, X, q);
    *cost = q;
    const bool st = xend != nullptr;
    if (st) {
#pragma unroll
        for (int k = 0; k < S; k++) xend[k] = X[k];
    }
}

template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void cost_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                          const double *__restrict__ Z, double *__restrict__ cost,
                                                          double *__restrict__ Xend)
{
    static_assert(INTEG == 0, "the running cost is integrated with the fixed-step integrator only");
    row_lane<PERPROB>(P, pb, B, pb.M, Z, [&](const ModelParams &Pq, const ProblemDev &pq, auto z, long, int i, long T) {
        double *xe = Xend ? Xend + T * Mdl::S : nullptr;
        segment_cost<Mdl>(Pq, pq, z, i, cost + T, xe);
    });
}

#ifdef SOCP_DEFINE_COMMON
// K_cost_total: total[b] = cost[b][0] + cost[b][1] + ... + cost[b][M-1], summed left to right; one lane per row
__global__ __launch_bounds__(64) void cost_total_kernel(int B, int M, const double *__restrict__ cost, double *__restrict__ total)
{
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double *c = cost + b * M;
    double s = c[0];
    for (int i = 1; i < M; i++) s = s + c[i];
    total[b] = s;
}
#endif

// ---------------------------------------------------------------------------------------------
// K_events: the control-structure events of every segment of B unknown vectors (socp_events_batch).  Z[B][n], levels[B][E] ->
// tev[B][M][cap], id[B][M][cap], count[B][M] and, unless null, Xev[B][M][cap][S].  One lane = (row, segment) (row_lane) watches
// the residual's fixed steps over its segment (SegmentSpan, integrate_events).  The events of a segment are
// stored in (step, watch) order: the first `cap` are stored, all are counted, and the rows at or beyond min(count, cap) keep
// what the buffer held (the conventions of K_trace); nothing is written past slab [b][i].  Xev of an event is one more RK4 step
// of the located length from the state before the step.  A zero-length or backward segment takes no step: count 0.
// NOT SEEN: a crossing in the gap between a segment's end state and the next node's unknowns (an unconverged row, whose
// trajectory jumps there) -- the watch compares the two ends of STEPS, and no step spans a node.
// Fixed-step RK4 only, and no model with its own ComputeTraj.  Consecutive lanes store consecutive words of count.
// ---------------------------------------------------------------------------------------------
// Event location: the loop of Lane::integrate around Lane::rk4 -- spelled out: with the step body handed to a shared loop
// helper the Goddard instantiations go into scratch -- with the state before the step (Xk, at the accumulated time tk) and the
// channel values at both ends of the step kept.  Watch e looks at
// channel chan[e] (four bits of `chans` each) minus level[e]; a sign change over a step, neg(v) = (v < 0.0) and neither end
// NaN, is an event.  It is refined inside the step by `refine` bracketed false-position steps, each ONE RK4 step of length
// th from Xk (not an interpolant: the located state is a state the integrator itself produces), then one more interpolation:
//     a = 0.0, c = step, ga = a0, gc = a1
//     repeat:  th = a + (c - a) * (ga / (ga - gc));  Y = rk4(tk, Xk, th);  gt = event_fn(tk + th, Y) - level
//              neg(gt) == neg(ga) ? (a = th, ga = gt) : (c = th, gc = gt)
//     te = tk + (a + (c - a) * (ga / (ga - gc)))
// in exactly this operation order (the parity contract of tests/events_reference.py).  id = +(e+1) rising through the level,
// -(e+1) falling.  Events leave through sink(te, id, tk, Xk, th) in (step, e) order.  All channels are evaluated at every
// step end (their number is a compile-time constant, so g0 / g1 stay in registers); the refinement runs under the exec
// mask of the few lanes that have an event in the step.
template <class Mdl, class Sink>
__device__ __forceinline__ void integrate_events(const ModelParams &P, double sw0, double sw1, double t0, double tf,
                                                 double (&X)[Mdl::S], int E, unsigned chans, const double *__restrict__ level,
                                                 int refine, Sink &&sink)
{
    constexpr int S = Mdl::S;
    constexpr int NC = event_channels<Mdl>::value;
    static_assert(NC >= 1, "the model has no event channels");
    auto pick = [](const double (&g)[NC], int ch) {
        double v = g[0];
#pragma unroll
        for (int c = 1; c < NC; c++) v = (ch == c) ? g[c] : v;
        return v;
    };
    double g0[NC], g1[NC], Xk[S];
#pragma unroll
    for (int c = 0; c < NC; c++) g0[c] = Mdl::event_fn(P, sw0, sw1, t0, X, c);
    const double dt = (tf - t0) / P.step_nbr;
    double t = t0;
    int guard = P.step_nbr + 8;
    while (t < (tf - dt / 2) && guard-- > 0) {
        const double step = (t + dt > tf) ? (tf - t) : dt;
#pragma unroll
        for (int k = 0; k < S; k++) Xk[k] = X[k];
        Lane<Mdl>::rk4(P, sw0, sw1, t, X, step);
#pragma unroll
        for (int c = 0; c < NC; c++) g1[c] = Mdl::event_fn(P, sw0, sw1, t + step, X, c);
        for (int e = 0; e < E; e++) {
            const int ch = (int)((chans >> (4 * e)) & 15u);
            const double lv = level[e];
            const double a0 = pick(g0, ch) - lv, a1 = pick(g1, ch) - lv;
            if (a0 == a0 && a1 == a1 && (a0 < 0.0) != (a1 < 0.0)) {
                double a = 0.0, c = step, ga = a0, gc = a1;
                for (int r = 0; r < refine; r++) {
                    const double th = a + (c - a) * (ga / (ga - gc));
                    double Y[S];
#pragma unroll
                    for (int k = 0; k < S; k++) Y[k] = Xk[k];
                    Lane<Mdl>::rk4(P, sw0, sw1, t, Y, th);
                    const double gt = Mdl::event_fn(P, sw0, sw1, t + th, Y, ch) - lv;
                    const bool same = (gt < 0.0) == (ga < 0.0);
                    a = same ? th : a;
                    ga = same ? gt : ga;
                    c = same ? c : th;
                    gc = same ? gc : gt;
                }
                const double th = a + (c - a) * (ga / (ga - gc));
                sink(t + th, (a0 < 0.0) ? e + 1 : -(e + 1), t, Xk, th);
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) g0[c] = g1[c];
        t += dt;
    }
}

template <class Mdl, class ZRead>
__device__ __forceinline__ void segment_events(const ModelParams &P, const ProblemDev &pb, const ZRead &z, int i, int E, unsigned chans,
                                               const double *__restrict__ level, int refine, int cap, double *__restrict__ tev,
                                               int *__restrict__ id, int *__restrict__ count, double *__restrict__ xev)
{
    static_assert(!has_custom_traj<Mdl>::value, "the events of a model with its own ComputeTraj need a definition of their own");
    constexpr int S = Mdl::S;
    double X[S];
    const SegmentSpan<Mdl> sp(P, pb, z, i, X);
    const double sw0 = sp.sw0, sw1 = sp.sw1;
    int found = 0;      // events so far (those beyond cap are counted, not stored)
    integrate_events<Mdl>(P, sw0, sw1, sp.t1, sp.t2, X, E, chans, level, refine,
                          [&](double te, int ev, double tk, const double (&Xk)[S], double th) {
        const bool st = found < cap;
        if (st) {
            tev[found] = te;
            id[found] = ev;
        }
        const bool sx = st && xev != nullptr;
        if (sx) {
            double Y[S];
#pragma unroll
            for (int k = 0; k < S; k++) Y[k] = Xk[k];
            Lane<Mdl>::rk4(P, sw0, sw1, tk, Y, th);
            double *row = xev + (long)found * S;
#pragma unroll
            for (int k = 0; k < S; k++) row[k] = Y[k];
        }
        found++;
    });
    *count = found;
}

template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void events_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                            const double *__restrict__ Z, int E, unsigned chans,
                                                            const double *__restrict__ levels, int refine, int cap,
                                                            double *__restrict__ tev, int *__restrict__ id,
                                                            int *__restrict__ count, double *__restrict__ Xev)
{
    static_assert(INTEG == 0, "events are located along the fixed-step integrator only");
    row_lane<PERPROB>(P, pb, B, pb.M, Z, [&](const ModelParams &Pq, const ProblemDev &pq, auto z, long b, int i, long T) {
        double *xe = Xev ? Xev + T * cap * Mdl::S : nullptr;
        segment_events<Mdl>(Pq, pq, z, i, E, chans, levels + b * E, refine, cap, tev + T * cap, id + T * cap, count + T, xe);
    });
}

// ---------------------------------------------------------------------------------------------
// K_move: shooting::Move(tf) (shooting.cpp:383-437) for a whole batch -- the state ON the stored solution z at a query time.
// Z[B][n], tq[B][K] -> Xq[B][K][S], optionally tout[B][K] (the time actually reached).  One lane = (row, query), T = b K + k
// (row_lane with K items per row).
// The lane forms the timeline with the shared prologue (Timeline: row b's own blocks under PERPROB), clamps the query to
// [tl(0), tl(M)] the way the reference does (:407-409: out of range -- and NaN, every comparison false -- goes to tl(M)),
// walks to the segment whose end is the first at or past the target (:416-424; the bound seg < M-1 is never reached by a finite
// ordered timeline, it keeps a NaN or disordered one inside row b), starts from THAT node's state z[S seg .. S seg + S) and
// integrates tl(seg) -> target with integrate_with: the model's ComputeTraj, a full step_nbr-step (or adaptive) integration
// whatever the distance.  So a query equal to an interior node time integrates the whole previous segment, and q == tl(0) is
// a zero-length integration that returns z[0 .. S) bit for bit.  isJac is dropped as in the reference (:440-444).
// Its segment is found by a search and ends at the query, so it spells the prologue out instead of taking a SegmentSpan.
// Fixed-step lanes of a wave all take step_nbr steps whatever their segment: the search adds no divergence to the loop.
// A lane's row is S consecutive doubles and consecutive lanes own adjacent rows (direct stores, like K_trace: a wave writes one
// contiguous 64 S 8-byte span).
// ---------------------------------------------------------------------------------------------
template <class Mdl, int INTEG, class ZRead>
__device__ __forceinline__ void segment_move(const ModelParams &P, const ProblemDev &pb, const ZRead &z, double q,
                                             double *__restrict__ xq, double *__restrict__ tout)
{
    constexpr int S = Mdl::S;
    const int M = pb.M;
    const Timeline<ZRead> tl{pb, z};
    const double t0 = tl.nt(0), te = tl.nt(M);
    const double target = (q >= t0 && q <= te) ? q : te;
    int seg = 0;
    while (seg < M - 1 && tl.nt(seg + 1) < target) seg++;
    const double t1 = tl.nt(seg);
    double sw0 = tl.template switching_time<Mdl>(P.sw0, pb.sw_node0), sw1 = tl.template switching_time<Mdl>(P.sw1, pb.sw_node1);
    double X[S];
    segment_start(z, S * seg, X);
    Lane<Mdl>::template integrate_with<INTEG>(P, sw0, sw1, t1, target, X);     // shooting.cpp:433 Move(t1, X1, t_f)
#pragma unroll
    for (int k = 0; k < S; k++) xq[k] = X[k];
    const bool st = tout != nullptr;
    if (st) *tout = target;
}

template <class Mdl, int WPE, int INTEG = 0, bool PERPROB = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, WPE))) void move_lane_kernel(ModelParams P, ProblemDev pb, int B,
                                                          const double *__restrict__ Z, int K, const double *__restrict__ tq,
                                                          double *__restrict__ Xq, double *__restrict__ tout)
{
    row_lane<PERPROB>(P, pb, B, K, Z, [&](const ModelParams &Pq, const ProblemDev &pq, auto z, long, int, long T) {
        double *to = tout ? tout + T : nullptr;
        segment_move<Mdl, INTEG>(Pq, pq, z, tq[T], Xq + T * Mdl::S, to);
    });
}

#ifdef SOCP_DEFINE_COMMON
// FREE nodes of a re-grid's target structure, bit j of word j / 64 = node j is FREE: a kernel argument, so the host's mode table is
// read before socp_regrid_batch_dev returns and nothing is copied from pageable memory (M2 <= 255 -> 256 bits).
struct RegridFree {
    unsigned long long w[4];
};

// K_regrid_pack: the unknown vector of the target structure from the moved node states (shooting.cpp:228-243, the layout of
// InitShooting(vt, vX)):  Z2[b][S j + c] = Xm[b][j][c] for j < M2, then the FREE node times T2[b][j_r] AS GIVEN (not clamped),
// r-th FREE node in node order.  One lane per entry of Z2, consecutive lanes on consecutive doubles; one store under one predicate.
__global__ __launch_bounds__(64) void regrid_pack_kernel(int B, int S, int M2, int n2, RegridFree fr, const double *__restrict__ Xm,
                                                         const double *__restrict__ T2, double *__restrict__ Z2)
{
    const long T = (long)blockIdx.x * 64 + threadIdx.x;              // = b * n2 + e
    if (T >= (long)B * n2) return;
    const long b = T / n2;
    const int e = (int)(T - b * n2);
    const int r = e - S * M2;                                        // >= 0: the r-th FREE node's time
    int node = 0;
    for (int j = 0, seen = 0; j <= M2; j++) {
        const bool is_free = (fr.w[j >> 6] >> (j & 63)) & 1ull;
        node = (is_free && seen == r) ? j : node;
        seen += is_free ? 1 : 0;
    }
    const double *src = r < 0 ? Xm + b * (long)(M2 + 1) * S + e : T2 + b * (long)(M2 + 1) + node;
    Z2[T] = *src;
}
#endif

}  // namespace socp
