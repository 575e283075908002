// kernels_branch.hip -- the kernels of socp_branch_batch (include/socp_hip.h): pseudo-arclength continuation of a whole batch, one
// round per (expand, residual, Jacobian, assemble, elimination, update) with the per-row state machine on the device.
// Built ONCE with -ffp-contract=off, for both flavours (like kernels_group.hip): every operation is one IEEE rounding, in the order
// socp_hip.h writes down.  A throughput-flavour context differs from a reference-order one through the model's own launches only
// (residual, Jacobian): the continuation layer -- these kernels and the elimination -- adds no deviation of its own, so what a
// throughput path deviates by is bounded by what its residual deviates by.
// Model-independent: the trajectories run through the model's own launch table (residual, fdjac, var_jacobian), the elimination is
// kernels_tangent.hip's.  Every per-row scalar is written by an ordinary store from plain C++.
#include "launch.hpp"

namespace socp {
namespace {

constexpr int kNone = 0, kStart = 1, kBad = 2, kAccept = 3, kReject = 4, kCorrect = 5;      // the case of a row in a round

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000LL); }

// the moved value of the addressed entry and the step taken: h = e |theta|, or e when theta == 0.0 (as socp_tangent_batch)
__device__ __forceinline__ double moved(double theta, double e, double &h)
{
    h = theta == 0.0 ? e : e * fabs(theta);
    return theta + h;
}

// ---- K_branch_expand: one workgroup per block row r = kk B + b (kk = 0: theta of the row's evaluation point, kk = 1: theta moved) --
// The first round also sets the row's state from Z and its blocks, and its outputs to "nothing recorded".
__global__ __launch_bounds__(64) void branch_expand_kernel(ModelParams P, ProblemDev pb, int nparams, int B, BranchArgs A, int first,
                                                           const double *__restrict__ Z, BranchState S, BranchOut O,
                                                           double *__restrict__ wP, double *__restrict__ wT, double *__restrict__ wX,
                                                           double *__restrict__ wZ)
{
    const long r = blockIdx.x;
    const int kk = (int)(r / B);
    const long b = r - (long)kk * B;
    if (kk > 1) return;
    const int stride = nparams + 2, nodes = pb.M + 1, nx = nodes * 2 * pb.dim, n = pb.n, n1 = n + 1;
    const double *sp = pb.pp_params ? pb.pp_params + b * pb.pp_stride : nullptr;
    const double *st = pb.pp_time ? pb.pp_time + b * nodes : pb.time;
    const double *sx = pb.pp_xnode ? pb.pp_xnode + b * (long)nx : pb.xnode;
    double lambda;
    if (first) {
        double theta0;
        if (A.kind == 0) theta0 = sp ? sp[A.index] : (A.index < nparams ? P.p[A.index] : (A.index == nparams ? P.sw0 : P.sw1));
        else if (A.kind == 1) theta0 = st[A.index];
        else theta0 = sx[A.index];
        lambda = theta0 / A.wtheta;
    } else {
        lambda = S.v[b * n1 + n];
    }
    const double theta = lambda * A.wtheta;
    double hth;
    const double thm = moved(theta, A.e, hth);
    const double mine = kk ? thm : theta;
    for (int k = threadIdx.x; k < stride; k += 64) {
        double v = sp ? sp[k] : (k < nparams ? P.p[k] : (k == nparams ? P.sw0 : P.sw1));
        if (A.kind == 0 && A.index == k) v = mine;
        wP[r * stride + k] = v;
    }
    for (int k = threadIdx.x; k < nodes; k += 64) {
        double v = st[k];
        if (A.kind == 1 && A.index == k) v = mine;
        wT[r * nodes + k] = v;
    }
    for (int k = threadIdx.x; k < nx; k += 64) {
        double v = sx[k];
        if (A.kind == 2 && A.index == k) v = mine;
        wX[r * nx + k] = v;
    }
    for (int k = threadIdx.x; k < n; k += 64) wZ[r * n + k] = first ? Z[b * n + k] : S.v[b * n1 + k];
    if (kk) return;
    if (threadIdx.x == 0) {
        S.hth[b] = hth;
        if (b == 0) *S.live = 0;
    }
    if (!first) return;
    for (int k = threadIdx.x; k < n1; k += 64) {
        const double v = k < n ? Z[b * n + k] : lambda;
        S.v[b * n1 + k] = v; S.y[b * n1 + k] = v; S.t[b * n1 + k] = 0.0;
    }
    const long cap = A.cap;
    for (long k = threadIdx.x; k < cap * n1; k += 64) O.Y[b * cap * n1 + k] = qnan();
    for (long k = threadIdx.x; k < cap; k += 64) { O.ttheta[b * cap + k] = qnan(); O.rnorm[b * cap + k] = qnan(); }
    if (O.zgoal)
        for (int k = threadIdx.x; k < n; k += 64) O.zgoal[b * n + k] = qnan();
    if (threadIdx.x == 0) {
        S.h[b] = A.h0; S.k[b] = 0; S.rn[b] = qnan(); S.kase[b] = kNone; S.info[b] = 0;
        O.count[b] = 0; O.nfold[b] = 0; O.ifold[b] = -1; O.status[b] = 0; O.nreject[b] = 0; O.hlast[b] = A.h0;
    }
}

// ---- K_branch_assemble: one workgroup per row: rn, the row's case, the bordered matrix column-major and the right-hand side -------
__global__ __launch_bounds__(256) void branch_assemble_kernel(int B, int n, BranchArgs A, int first, const double *__restrict__ F,
                                                              const double *__restrict__ J, BranchState S, const int *__restrict__ status,
                                                              double *__restrict__ Mx, double *__restrict__ rhs)
{
    __shared__ double smax[4];
    __shared__ int sbad[4];
    __shared__ int skase;
    const long b = blockIdx.x;
    const int n1 = n + 1, tid = threadIdx.x;
    const double *F0 = F + b * n, *F1 = F + ((long)B + b) * n;
    // rn = max |F0_i|, a NaN when an entry is one (an infinite entry makes the maximum infinite): maxima commute, so any order
    double m = 0.0;
    int bad = 0;
    for (int i = tid; i < n; i += 256) {
        const double a = fabs(F0[i]);
        if (a != a) bad = 1;
        else if (a > m) m = a;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double m2 = __shfl_xor(m, s);
        const int b2 = __shfl_xor(bad, s);
        if (m2 > m) m = m2;
        bad |= b2;
    }
    if ((tid & 63) == 0) { smax[tid >> 6] = m; sbad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) { if (smax[w] > m) m = smax[w]; bad |= sbad[w]; }
        const double rn = bad ? qnan() : m;
        const bool finite = fabs(rn) < INFINITY;
        int kase;
        if (status[b] != 0) kase = kNone;
        else if (first) kase = finite ? kStart : kBad;
        else if (rn <= A.ftol) kase = kAccept;
        else if (!finite || S.k[b] == A.max_corr) kase = kReject;
        else kase = kCorrect;
        S.rn[b] = rn; S.kase[b] = kase;
        skase = kase;
    }
    __syncthreads();
    const bool correct = skase == kCorrect;
    const double hth = S.hth[b], *Jb = J + b * (long)n * n, *t = S.t + b * n1;
    double *Mb = Mx + b * (long)n1 * n1;
    for (int e = tid; e < n1 * n1; e += 256) {
        const int j = e / n1, i = e - j * n1;
        double v;
        if (i < n) v = j < n ? Jb[i + (long)j * n] : ((F1[i] - F0[i]) / hth) * A.wtheta;
        else v = first ? (j == n ? (double)A.dir : 0.0) : t[j];
        Mb[e] = v;
    }
    for (int i = tid; i < n1; i += 256) rhs[b * n1 + i] = i < n ? (correct ? -F0[i] : 0.0) : (correct ? 0.0 : 1.0);
}

// ---- K_branch_update: one thread per row: the norms, the distance guard, the transitions, the records, fold, goal and step control --
__global__ __launch_bounds__(64) void branch_update_kernel(int B, int n, BranchArgs A, BranchState S, BranchOut O, const double *__restrict__ X)
{
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (O.status[b] != 0) return;                                 // a finished row changes nothing any more
    const int n1 = n + 1, kase = S.kase[b], info = S.info[b];
    double *v = S.v + b * n1, *y = S.y + b * n1, *t = S.t + b * n1;
    const double *x = X + b * n1;
    double h = S.h[b];
    int k = S.k[b], status = 0;
    bool predict = false, reject = kase == kReject;
    if (kase == kBad) {
        status = 5;
    } else if (kase == kStart || kase == kAccept) {
        for (int i = 0; i < n1; i++) y[i] = v[i];
        double s = 0.0;
        for (int i = 0; i < n1; i++) s = s + x[i] * x[i];
        const bool singular = info != 0 || s == 0.0 || !(fabs(s) < INFINITY);
        const long idx = O.count[b], at = b * A.cap + idx;
        const double theta = v[n] * A.wtheta;
        for (int i = 0; i < n; i++) O.Y[at * n1 + i] = v[i];
        O.Y[at * n1 + n] = theta;
        O.rnorm[at] = S.rn[b];
        O.count[b] = (int)idx + 1;
        if (singular) {
            status = 4;                                           // ttheta of this point stays NaN
        } else {
            const double root = sqrt(s), told = t[n];
            for (int i = 0; i < n1; i++) t[i] = x[i] / root;
            const double tnew = t[n];
            O.ttheta[at] = tnew;
            if (kase == kStart) {
                h = A.h0;
                predict = true;
            } else {
                if (signbit(tnew) != signbit(told)) {
                    O.nfold[b] = O.nfold[b] + 1;
                    if (O.ifold[b] < 0) O.ifold[b] = (int)idx;
                }
                if (k <= A.kfast) { const double g = h * A.grow; h = g < A.hmax ? g : A.hmax; }
                bool reached = false;
                if (A.have_goal) {
                    const double *prev = O.Y + (at - 1) * n1;
                    const double tp = prev[n], a = tp - A.goal, c = theta - A.goal;
                    reached = c == 0.0 || (a != 0.0 && (a < 0.0) != (c < 0.0));
                    if (reached && O.zgoal) {
                        const double w = (A.goal - tp) / (theta - tp);
                        for (int i = 0; i < n; i++) { const double d = v[i] - prev[i]; O.zgoal[b * n + i] = prev[i] + w * d; }
                    }
                }
                if (reached) status = 1;
                else if (idx + 1 == A.cap) status = 2;
                else predict = true;
            }
        }
    } else if (kase == kCorrect) {
        double s = 0.0;
        for (int i = 0; i < n1; i++) s = s + x[i] * x[i];
        const double dn = sqrt(s);
        if (info != 0 || !(dn <= h)) {
            reject = true;                                        // the distance guard: Newton may not leave the step's ball
        } else {
            for (int i = 0; i < n1; i++) v[i] = v[i] + x[i];
            k += 1;
        }
    }
    if (reject) {
        O.nreject[b] = O.nreject[b] + 1;
        h = h / 2;
        if (h < A.hmin) status = 3;
        else predict = true;
    }
    if (predict) {
        for (int i = 0; i < n1; i++) { const double step = h * t[i]; v[i] = y[i] + step; }
        k = 0;
    }
    S.h[b] = h; S.k[b] = k;
    O.hlast[b] = h;
    O.status[b] = status;
    if (status == 0) atomicAdd(S.live, 1);
}

}  // namespace

hipError_t branch_expand(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int nparams, int B, const BranchArgs &A,
                                           int first, const double *Z, const BranchState &S, const BranchOut &O, double *wP, double *wT,
                                           double *wX, double *wZ)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(branch_expand_kernel, dim3((unsigned)(2 * (long)B)), dim3(64), 0, st, P, pb, nparams, B, A, first, Z, S, O, wP, wT, wX, wZ);
    return hipGetLastError();
}

hipError_t branch_assemble(hipStream_t st, int B, int n, const BranchArgs &A, int first, const double *F, const double *J,
                                             const BranchState &S, const int *status, double *Mx, double *rhs)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(branch_assemble_kernel, dim3((unsigned)B), dim3(256), 0, st, B, n, A, first, F, J, S, status, Mx, rhs);
    return hipGetLastError();
}

hipError_t branch_update(hipStream_t st, int B, int n, const BranchArgs &A, const BranchState &S, const BranchOut &O,
                                           const double *X)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(branch_update_kernel, dim3((unsigned)(((long)B + 63) / 64)), dim3(64), 0, st, B, n, A, S, O, X);
    return hipGetLastError();
}

}  // namespace socp
