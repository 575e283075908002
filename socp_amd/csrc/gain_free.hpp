// gain_free.hpp -- K_gain_free_blocks and K_gain_free_sweep: the neighbouring-extremal feedback gains of B unknown vectors whose FINAL
// TIME IS FREE (socp_gain_free_batch; the definition is the comment of the entry points in include/socp_hip.h,
// tests/gain_free_reference.py restates it in Python).
//
// K_gain_free_blocks has exact_jacobian_kernel's group shape (exact_jacobian.hpp) with gain_blocks_kernel's block loop (gain.hpp): the
// S + 1 columns of one (row, segment) sit in S + 1 NEIGHBOURING lanes, lane c < S carries column c of the transition matrix since the
// last sample, lane S -- the LENGTH lane -- the derivative with respect to the segment's length L = t2 - t1 since the last sample.  ONE
// text for every lane: t2 = (t2, 1.0) in the length lane and (t2, +0.0) in the others, so t, dt and the step are dual numbers in all
// of them, h F is the full dual product, and the loop condition and the clamp read value parts: a group never diverges.  At a sample
// the derivative parts of the STATE re-seed (e_c in lane c, +0.0 in the length lane); those of t and dt do not -- the clamped last step
// t2 - t needs dt/dL.  After the block lane c stores column c of Psi_q, the length lane stores l_q.  After the last block of the LAST
// segment the state re-seeds once more and every lane evaluates hamiltonian_t on it at t2: lane c stores entry c of grad H(X_f).
//
// K_gain_free_sweep turns the blocks into gains: D + 1 NEIGHBOURING lanes per row of the batch, lanes r < D hold the terminal rows,
// lane D the H row; each lane keeps W[S] and one border entry wtau.  Downward over (segment, sample): first
// wtau <- wtau + w_i (W . l_q), then W <- W Psi_q (gain_sweep_kernel's product).  The bordered matrix [A_p | wtau] goes into the
// elimination's staging matrix, -A_x into Ke, which is the elimination's right-hand side in place.  No register array is indexed by a
// run-time value, every store site is ONE block under ONE computed predicate (segment_residual's note).
#pragma once
#include "exact_jacobian.hpp"
#include "gain.hpp"

namespace socp {

template <class Mdl, bool PERPROB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void gain_free_blocks_kernel(ModelParams P, ProblemDev pb, int B,
                                                                  const double *__restrict__ Z, int stride, int cap,
                                                                  double *__restrict__ tq, double *__restrict__ Xq,
                                                                  int *__restrict__ count, double *__restrict__ Psi,
                                                                  double *__restrict__ Len, double *__restrict__ gradH)
{
    static_assert(!has_custom_traj<Mdl>::value && !has_custom_final<Mdl>::value && !has_switching_state<Mdl>::value,
                  "the gains of such a model need a definition of their own");
    constexpr int S = Mdl::S;
    constexpr int G = S + 1;                                          // one lane per column: S state columns and the length
    static_assert(G <= 64, "a group fits one wavefront");
    const GroupLane L = group_lane(B, pb.M, G);
    const double *zr = Z + L.b * pb.n;
    auto z = [=](int k) -> double { return zr[k]; };
    ModelParams Pq = P;
    ProblemDev pq = pb;
    if constexpr (PERPROB) load_problem_block(pb, L.b, Pq, pq);
    const int c = L.c;
    const bool len = c == S;                                          // the length lane
    double X0[S];
    const SegmentSpan<Mdl> sp(Pq, pq, z, L.i, X0);
    Dual X[S];
    dual_start(X0, c, X);                                             // the length lane: c == S, no unit entry
    // the loop of fixed_steps_dual, its condition carried in `act` (gain_blocks_kernel)
    const long T = L.T;
    const bool live = L.live;
    const double t1 = sp.t1, t2 = sp.t2, sw0 = sp.sw0, sw1 = sp.sw1;
    const Dual t2d(t2, len ? 1.0 : 0.0);
    const Dual dt = (t2d - Dual(t1, 0.0)) / (double)Pq.step_nbr;
    Dual t(t1, 0.0);
    int guard = Pq.step_nbr + 8;
    bool act = t.v < (t2 - dt.v / 2) && guard-- > 0;
    bool go = true;                 // this lane has a block to take: the first one always (a segment without a step: Psi_0 = I, l_0 = 0)
    int ns = 0;                     // blocks so far (those beyond cap are counted, not stored)
    // one iteration per BLOCK, wave-uniform
    while (__any(go)) {
        const bool keep = go && live && ns < cap;
        const long slot = T * cap + ns;
        // sample ns: the loop's own t and the value state at the start of step ns * stride
        const bool s0 = keep && c == 0;
        if (s0) tq[slot] = t.v;
        const bool sx = s0 && Xq != nullptr;
        if (sx) {
            double *out = Xq + slot * S;
#pragma unroll
            for (int j = 0; j < S; j++) out[j] = X[j].v;
        }
        // the re-seed: (X[j].v, j == c ? 1.0 : +0.0); t and dt keep their derivative parts
#pragma unroll
        for (int j = 0; j < S; j++) X[j].d = go ? (j == c ? 1.0 : 0.0) : X[j].d;
        int left = stride;
        while (go && act && left > 0) {
            const Dual step = (t.v + dt.v > t2) ? (t2d - t) : dt;
            dual_rk4<Mdl>(Pq, sw0, sw1, t, X, step);
            t = t + dt;
            act = t.v < (t2 - dt.v / 2) && guard-- > 0;
            left--;
        }
        // a state lane: column c of Psi_ns (row-major: row r of X, column c); the length lane: l_ns, S consecutive doubles
        double *out = len ? Len + slot * S : Psi + slot * (S * S) + c;
        const int pitch = len ? 1 : S;
        if (keep) {
#pragma unroll
            for (int r = 0; r < S; r++) out[r * pitch] = X[r].d;
        }
        ns += go ? 1 : 0;
        go = go && act;
    }
    const bool sm = live && c == 0;
    if (sm) count[T] = ns;
    // the H row of the backward sweep: grad H at the final state, entry c from lane c
    if (L.i == pq.M - 1) {
#pragma unroll
        for (int j = 0; j < S; j++) X[j].d = j == c ? 1.0 : 0.0;
        const Dual H = Mdl::template hamiltonian_t<Dual>(Pq, sw0, sw1, t2, X);
        const bool sh = live && !len;
        if (sh) gradH[L.b * S + c] = H.d;
    }
}

// one group of D + 1 neighbouring lanes per ROW of the batch (group_lane with one slab per row).  A: the staging matrices of the
// elimination, [B][M][cap][(D + 1) * (D + 1)] column-major; Ke: its right-hand sides, [B][M][cap][D][D + 1]
template <class Mdl>
__global__ __launch_bounds__(64) void gain_free_sweep_kernel(ProblemDev pb, int B, int cap, const int *__restrict__ count,
                                                             const double *__restrict__ Psi, const double *__restrict__ Len,
                                                             const double *__restrict__ gradH, double *__restrict__ Wq,
                                                             double *__restrict__ A, double *__restrict__ Ke)
{
    constexpr int S = Mdl::S;
    constexpr int D = Mdl::D;
    constexpr int D1 = D + 1;
    static_assert(D1 <= 64, "a group fits one wavefront");
    const GroupLane L = group_lane(B, 1, D1);
    const int r = L.c;
    const int M = pb.M;
    const bool hrow = r == D;
    // rows r < D: row r of the selector E of the final boundary rows (gain_sweep_kernel); row D: grad H(X_f)
    const int unit = hrow ? -1 : (pb.mode_x[M * D + r] == 1 ? D + r : r);
    // a segment that counted more blocks than cap stores leaves the chain of products incomplete: the row's W starts from NaN
    bool whole = true;
    for (int i = 0; i < M; i++) whole = whole && count[L.b * M + i] <= cap;
    const double nan = __builtin_nan("");
    const double one = whole ? 1.0 : nan;
    const double *gh = gradH + L.b * S;
    double W[S];
#pragma unroll
    for (int j = 0; j < S; j++) W[j] = hrow ? (whole ? gh[j] : nan) : (j == unit ? one : 0.0);
    double wtau = 0.0;
    for (int i = M - 1; i >= 0; i--) {
        const long seg = L.b * M + i;
        const int nq = count[seg] < cap ? count[seg] : cap;
        // the weight of t_f in the segment's length (time_weight: the exact Jacobian's)
        const double wi = time_weight(pb, i + 1, M) - time_weight(pb, i, M);
        for (int q = nq - 1; q >= 0; q--) {
            const long slot = seg * cap + q;
            const double *ps = Psi + slot * (S * S);
            const double *ln = Len + slot * S;
            // wtau' = wtau + w_i (sum_m W[m] l[m]), m ascending, from the first product; skipped when w_i == 0
            double dot = W[0] * ln[0];
#pragma unroll
            for (int m = 1; m < S; m++) dot = dot + W[m] * ln[m];
            wtau = wi != 0.0 ? wtau + wi * dot : wtau;
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
                double *a = A + slot * (D1 * D1) + r, *k = Ke + slot * (D1 * D) + r;
#pragma unroll
                for (int cc = 0; cc < D; cc++) {
                    a[cc * D1] = W[D + cc];
                    k[cc * D1] = -W[cc];
                }
                a[D * D1] = wtau;
            }
            const bool sw = L.live && Wq != nullptr;
            if (sw) {
                double *w = Wq + slot * (D1 * (S + 1)) + r * (S + 1);
#pragma unroll
                for (int j = 0; j < S; j++) w[j] = W[j];
                w[S] = wtau;
            }
        }
    }
}

}  // namespace socp
