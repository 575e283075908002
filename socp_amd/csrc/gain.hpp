// gain.hpp -- K_gain_blocks and K_gain_sweep: the neighbouring-extremal feedback gains of B unknown vectors (socp_gain_batch; the
// definition is the comment of the entry points in include/socp_hip.h, tests/gain_reference.py restates it in Python).
//
// K_gain_blocks is fields_group_kernel<Mdl, true, ...> (fields.hpp) cut into BLOCKS of `stride` steps: the S columns of one
// (row, segment) sit in S NEIGHBOURING lanes (group_lane), lane c carries the state as S dual numbers whose derivative parts are
// column c of the transition matrix SINCE THE LAST SAMPLE.  At a sample lane 0 stores the loop's t and the value state, every lane
// re-seeds its derivative parts to the unit column e_c (the value parts are never touched: the value trajectory is the
// reference-order residual's), the block's steps follow, and lane c stores column c of the block Psi_q.  The loop over the samples
// is wave-uniform, the residual-shaped per-lane step loop sits inside it, as in fields_group_kernel; the lanes never meet.  The
// register budget is that kernel's: five RK4 arrays of 2 S doubles, one wave per SIMD on Goddard (profiles/gain_kernel_meta.txt).
//
// K_gain_sweep turns the blocks into gains: D NEIGHBOURING lanes per row of the batch, lane r holds row r of W = E Psi_last ... Psi_q
// in S registers.  It walks (segment, sample) downward, W <- W Psi (each product rounded, the sum sequential from the first
// product, m ascending), stores row r of Wq, column entries of A_p into the elimination's staging matrix and of -A_x into Kp, which is
// the elimination's right-hand side in place.  The lanes of a group read the same Psi entries in the same instruction, so a
// block travels once per group.  No register array is indexed by a run-time value (exact_jacobian.hpp), every store site is ONE
// block under ONE computed predicate (segment_residual's note).
#pragma once
#include "fields.hpp"

namespace socp {

template <class Mdl, bool PERPROB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void gain_blocks_kernel(ModelParams P, ProblemDev pb, int B,
                                                             const double *__restrict__ Z, int stride, int cap,
                                                             double *__restrict__ tq, double *__restrict__ Xq,
                                                             int *__restrict__ count, double *__restrict__ Psi)
{
    static_assert(!has_custom_traj<Mdl>::value, "the gains of a model with its own ComputeTraj need a definition of their own");
    constexpr int S = Mdl::S;
    constexpr int G = S;                                              // one lane per column
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
    dual_start(X0, c, X);
    // the loop of Lane::integrate, its condition carried in `act` (fields_group_kernel)
    const long T = L.T;
    const bool live = L.live;
    const double t1 = sp.t1, t2 = sp.t2, sw0 = sp.sw0, sw1 = sp.sw1;
    const double dt = (t2 - t1) / Pq.step_nbr;
    double t = t1;
    int guard = Pq.step_nbr + 8;
    bool act = t < (t2 - dt / 2) && guard-- > 0;
    bool go = true;                 // this lane has a block to take: the first one always (a segment without a step: Psi_0 = I)
    int ns = 0;                     // blocks so far (those beyond cap are counted, not stored)
    // one iteration per BLOCK, wave-uniform
    while (__any(go)) {
        const bool keep = go && live && ns < cap;
        const long slot = T * cap + ns;
        // sample ns: the loop's own t and the value state at the start of step ns * stride
        const bool s0 = keep && c == 0;
        if (s0) tq[slot] = t;
        const bool sx = s0 && Xq != nullptr;
        if (sx) {
            double *out = Xq + slot * S;
#pragma unroll
            for (int j = 0; j < S; j++) out[j] = X[j].v;
        }
        // the re-seed: (X[j].v, j == c ? 1.0 : +0.0)
#pragma unroll
        for (int j = 0; j < S; j++) X[j].d = go ? (j == c ? 1.0 : 0.0) : X[j].d;
        int left = stride;
        while (go && act && left > 0) {
            const double step = (t + dt > t2) ? (t2 - t) : dt;
            dual_rk4<Mdl>(Pq, sw0, sw1, t, X, step);
            t += dt;
            act = t < (t2 - dt / 2) && guard-- > 0;
            left--;
        }
        // column c of Psi_ns (row-major: row r of X, column c -- the layout of Phi)
        const bool sp_ = keep && Psi != nullptr;
        if (sp_) {
            double *out = Psi + slot * (S * S) + c;
#pragma unroll
            for (int r = 0; r < S; r++) out[r * S] = X[r].d;
        }
        ns += go ? 1 : 0;
        go = go && act;
    }
    const bool sm = live && c == 0;
    if (sm) count[T] = ns;
}

// one group of D neighbouring lanes per ROW of the batch (group_lane with one slab per row).  A: the staging matrices of the
// elimination, [B][M][cap][D * D] column-major
template <class Mdl>
__global__ __launch_bounds__(64) void gain_sweep_kernel(ProblemDev pb, int B, int cap, const int *__restrict__ count,
                                                        const double *__restrict__ Psi, double *__restrict__ Wq, double *__restrict__ A,
                                                        double *__restrict__ Kp)
{
    constexpr int S = Mdl::S;
    constexpr int D = Mdl::D;
    const GroupLane L = group_lane(B, 1, D);
    const int r = L.c;
    const int M = pb.M;
    // row r of the selector E of the final boundary rows: e_{D + r} when final component r is FREE, else e_r
    const int unit = pb.mode_x[M * D + r] == 1 ? D + r : r;
    // a segment that counted more blocks than cap stores (rounding gave its loop a step beyond step_nbr) leaves the chain of
    // products incomplete: the row's W starts from NaN and every sample of it reports a failed elimination
    bool whole = true;
    for (int i = 0; i < M; i++) whole = whole && count[L.b * M + i] <= cap;
    const double one = whole ? 1.0 : __builtin_nan("");
    double W[S];
#pragma unroll
    for (int j = 0; j < S; j++) W[j] = j == unit ? one : 0.0;
    for (int i = M - 1; i >= 0; i--) {
        const long seg = L.b * M + i;
        const int nq = count[seg] < cap ? count[seg] : cap;
        for (int q = nq - 1; q >= 0; q--) {
            const long slot = seg * cap + q;
            const double *ps = Psi + slot * (S * S);
            // W'[r][j] = sum_m W[r][m] Psi[m][j], m ascending, from the first product
            double V[S];
#pragma unroll
            for (int j = 0; j < S; j++) V[j] = W[0] * ps[j];
#pragma unroll
            for (int m = 1; m < S; m++) {
#pragma unroll
                for (int j = 0; j < S; j++) V[j] = V[j] + W[m] * ps[m * S + j];
            }
#pragma unroll
            for (int j = 0; j < S; j++) W[j] = V[j];
            const bool st = L.live;
            if (st) {
                double *a = A + slot * (D * D) + r, *k = Kp + slot * (D * D) + r;
#pragma unroll
                for (int cc = 0; cc < D; cc++) {
                    a[cc * D] = W[D + cc];
                    k[cc * D] = -W[cc];
                }
            }
            const bool sw = L.live && Wq != nullptr;
            if (sw) {
                double *w = Wq + slot * (D * S) + r * S;
#pragma unroll
                for (int j = 0; j < S; j++) w[j] = W[j];
            }
        }
    }
}

}  // namespace socp
