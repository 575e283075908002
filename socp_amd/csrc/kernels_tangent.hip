// kernels_tangent.hip -- the kernels of socp_tangent_batch (include/socp_hip.h): the expanded block rows of the parameter
// differences, the right-hand sides, and the batched dense linear solve with several right-hand sides.
// Built TWICE (socp_amd/csrc/Makefile): without -DSOCP_TANGENT_FAST and with -ffp-contract=off for reference-order contexts --
// every operation of the elimination is then a single IEEE rounding, in the order socp_hip.h writes down -- and with
// -DSOCP_TANGENT_FAST and -ffp-contract=fast for throughput-flavour contexts (the updates become fused multiply-adds).
// Model-independent: the trajectories of a tangent run through the model's own launch table (residual, fdjac, var_jacobian).
#include <climits>

#include "launch.hpp"

namespace socp {
namespace {

// ---- K_tangent_expand: one workgroup per block row r = kk B + b (kk = 0: row b's own block, kk = k + 1: direction k moved) -------
// the moved value of an addressed entry and the step taken: h = e |theta|, or e when theta == 0.0 (MINPACK fdjac1's rule)
__device__ __forceinline__ double moved(double theta, double e, double &h)
{
    h = theta == 0.0 ? e : e * fabs(theta);
    return theta + h;
}

__global__ __launch_bounds__(64) void tangent_expand_kernel(ModelParams P, ProblemDev pb, int nparams, int B, int K, TangentDirs dirs, double e,
                                                            const double *__restrict__ Z, double *__restrict__ wP, double *__restrict__ wT,
                                                            double *__restrict__ wX, double *__restrict__ wZ, double *__restrict__ wH)
{
    const long r = blockIdx.x;
    const int kk = (int)(r / B);
    const long b = r - (long)kk * B;
    if (kk > K) return;
    const int stride = nparams + 2, nodes = pb.M + 1, nx = nodes * 2 * pb.dim, n = pb.n;
    const int kind = kk > 0 ? dirs.kind[kk - 1] : -1, index = kk > 0 ? dirs.index[kk - 1] : -1;
    const double *sp = pb.pp_params ? pb.pp_params + b * pb.pp_stride : nullptr;
    const double *st = pb.pp_time ? pb.pp_time + b * nodes : pb.time;
    const double *sx = pb.pp_xnode ? pb.pp_xnode + b * (long)nx : pb.xnode;
    double *hk = wH + b * K + (kk > 0 ? kk - 1 : 0);                // written by the thread that moves the entry
    double h;
    for (int k = threadIdx.x; k < stride; k += 64) {
        double v = sp ? sp[k] : (k < nparams ? P.p[k] : (k == nparams ? P.sw0 : P.sw1));
        if (kind == 0 && index == k) { v = moved(v, e, h); *hk = h; }
        wP[r * stride + k] = v;
    }
    for (int k = threadIdx.x; k < nodes; k += 64) {
        double v = st[k];
        if (kind == 1 && index == k) { v = moved(v, e, h); *hk = h; }
        wT[r * nodes + k] = v;
    }
    for (int k = threadIdx.x; k < nx; k += 64) {
        double v = sx[k];
        if (kind == 2 && index == k) { v = moved(v, e, h); *hk = h; }
        wX[r * nx + k] = v;
    }
    for (int k = threadIdx.x; k < n; k += 64) wZ[r * n + k] = Z[b * n + k];
}

// ---- K_tangent_diff: G[b][k][i] = (F[(k+1) B + b][i] - F[b][i]) / h[b][k];  -G into the right-hand sides, G into Fp unless null ----
__global__ __launch_bounds__(256) void tangent_diff_kernel(int B, int K, int n, const double *__restrict__ F, const double *__restrict__ H,
                                                           double *__restrict__ rhs, double *__restrict__ Fp)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * K * n) return;
    const long bk = e / n;
    const int i = (int)(e - bk * n), k = (int)(bk % K);
    const long b = bk / K;
    const double g = (F[(((long)k + 1) * B + b) * n + i] - F[b * n + i]) / H[bk];
    rhs[e] = -g;
    if (Fp) Fp[e] = g;
}

// ---- K_linsolve: Gaussian elimination with partial pivoting and K right-hand sides, one problem per TEAM of W wavefronts ----------
// (a, i) <- the larger of two pivot candidates, the lower index among equal ones.  Candidates are never NaN (a NaN entry below the
// diagonal enters as -1.0: the sequential search `if (|a_ik| > best)` never takes it), so the rule is associative and commutative
// and the result does not depend on how the candidates are spread over lanes.
__device__ __forceinline__ void pivot_max(double &a, int &i, double a2, int i2)
{
    if (a2 > a || (a2 == a && i2 < i)) { a = a2; i = i2; }
}

__device__ __forceinline__ void wave_pivot_max(double &a, int &i)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double a2 = __shfl_xor(a, m);
        const int i2 = __shfl_xor(i, m);
        pivot_max(a, i, a2, i2);
    }
}

// A[B][n*n] column-major, Y[B][K][n], info[B].  The matrix and the right-hand sides of a team form ONE column-major array of
// n + K columns; element (i, j) of it is
//   IN_LDS   mat[i + j lda], copied in once, lda = n | 1: the row swap and the pivot row walk along a row, stride lda doubles, and an
//            odd stride visits all 32 eight-byte banks before it repeats; the column operations have stride 1
//   !IN_LDS  A / Y themselves in HBM; the pivot row and the multiplier column of a step are staged in LDS, so that the update
//            reads each matrix entry once and writes it once
// Threads of a team: tt = 0 .. 64 W - 1; for the updates row slot r = tt % RL and column worker cw = tt / RL (RL = 16 when n <= 16
// -- four such teams share a workgroup -- else 64).  Every barrier is reached by every thread of the workgroup: a team that has
// failed, or has no problem, skips the work between them.
// b: the team's problem, live: whether it has one
template <bool IN_LDS>
__device__ __forceinline__ void linsolve_team(long b, bool live, int n, int K, int W, int RL, int lda, double *A, double *Y, int *info)
{
    extern __shared__ double sm[];
    const int NT = W * 64, team = threadIdx.x / NT, tt = threadIdx.x - team * NT, lane = tt & 63, wave = tt >> 6;
    const int r = tt % RL, cw = tt / RL, NCW = NT / RL, nc = n + K;
    double *Ab = A + (live ? b : 0) * (long)n * n, *Yb = Y + (live ? b : 0) * (long)K * n;
    const int team_doubles = (IN_LDS ? lda * nc : nc + n) + kLinsolveScratch;
    double *mat = sm + (long)team * team_doubles;                 // IN_LDS: the array; else prow[nc] then lcol[n]
    double *prow = mat, *lcol = mat + nc;
    double *redv = mat + (team_doubles - kLinsolveScratch);
    int *redi = reinterpret_cast<int *>(redv + 4), *flag = redi + 4;
    auto at = [&](int i, int j) -> double & {
        if constexpr (IN_LDS) return mat[i + j * lda];
        else return j < n ? Ab[i + (long)j * n] : Yb[i + (long)(j - n) * n];
    };

    if (tt == 0) *flag = 0;
    if constexpr (IN_LDS) {
        if (live)
            for (int j = wave; j < nc; j += W)
                for (int i = lane; i < n; i += 64) mat[i + j * lda] = j < n ? Ab[i + (long)j * n] : Yb[i + (long)(j - n) * n];
    }
    __syncthreads();

    int failed = 0;                                               // info of a failed team: k + 1; the same in all its threads
    for (int k = 0; k < n; k++) {
        bool act = live && !failed;
        // pivot search: best = |a_kk|, p = k, then the first strictly larger |a_ik| below; a NaN a_kk stays (and fails the step)
        double best = -1.0, dkk = 0.0;
        int p = INT_MAX;
        if (act) {
            dkk = fabs(at(k, k));
            for (int i = k + tt; i < n; i += NT) {
                double a = fabs(at(i, k));
                if (a != a) a = -1.0;
                pivot_max(best, p, a, i);
            }
        }
        wave_pivot_max(best, p);
        if (W > 1) {
            if (lane == 0) { redv[wave] = best; redi[wave] = p; }
            __syncthreads();
            best = redv[0]; p = redi[0];
            for (int w = 1; w < W; w++) pivot_max(best, p, redv[w], redi[w]);
        }
        if (dkk != dkk) { best = dkk; p = k; }
        if (act && (!(best > 0.0) || best == INFINITY)) { failed = k + 1; act = false; }
        if (act && p != k)
            for (int j = tt; j < nc; j += NT) {
                const double x = at(k, j), y = at(p, j);
                at(k, j) = y; at(p, j) = x;
            }
        __syncthreads();
        // multipliers l_i = a_ik / a_kk, kept in column k
        if (act) {
            const double akk = at(k, k);
            for (int i = k + 1 + tt; i < n; i += NT) {
                const double l = at(i, k) / akk;
                at(i, k) = l;
                if constexpr (!IN_LDS) lcol[i] = l;
            }
            if constexpr (!IN_LDS)
                for (int j = k + 1 + tt; j < nc; j += NT) prow[j] = at(k, j);
        }
        __syncthreads();
        // a_ij <- a_ij - l_i a_kj and y_i <- y_i - l_i y_k for i, j > k
        if (act)
            for (int i = k + 1 + r; i < n; i += RL) {
                const double l = IN_LDS ? at(i, k) : lcol[i];
                for (int j = k + 1 + cw; j < nc; j += NCW) {
                    const double akj = IN_LDS ? at(k, j) : prow[j];
                    at(i, j) = at(i, j) - l * akj;
                }
            }
        __syncthreads();
    }

    // back substitution: x_k = y_k / a_kk, then y_i <- y_i - a_ik x_k for i < k
    const bool act = live && !failed;
    for (int k = n - 1; k >= 0; k--) {
        if (act) {
            const double akk = at(k, k);
            for (int c = tt; c < K; c += NT) at(k, n + c) = at(k, n + c) / akk;
        }
        __syncthreads();
        if (act)
            for (int c = cw; c < K; c += NCW) {
                const double xk = at(k, n + c);
                for (int i = r; i < k; i += RL) at(i, n + c) = at(i, n + c) - at(i, k) * xk;
            }
        __syncthreads();
    }

    if (live) {
        if (failed) {
            const double nan = __longlong_as_double(0x7FF8000000000000LL);
            for (int e = tt; e < K * n; e += NT) Yb[e] = nan;
        } else {
            for (int c = wave; c < K; c += W)
                for (int i = lane; i < n; i += 64) {
                    const double x = at(i, n + c);
                    if (!(fabs(x) < INFINITY)) *flag = 1;
                    if constexpr (IN_LDS) Yb[i + (long)c * n] = x;
                }
        }
    }
    __syncthreads();
    if (live && tt == 0) info[b] = failed ? failed : (*flag ? n + 1 : 0);
}

template <bool IN_LDS>
__global__ __launch_bounds__(256) void linsolve_kernel(long B, int n, int K, int W, int T, int RL, int lda, double *A, double *Y, int *info)
{
    const long b = (long)blockIdx.x * T + threadIdx.x / (W * 64);
    linsolve_team<IN_LDS>(b, b < B, n, K, W, RL, lda, A, Y, info);
}

#ifndef SOCP_TANGENT_FAST
// the problems are the slots [B][cap]; slot q of b holds one iff q < count[b], the others are neither read nor written
template <bool IN_LDS>
__global__ __launch_bounds__(256) void linsolve_slots_kernel(long B, int cap, const int *__restrict__ count, int n, int K, int W, int T, int RL,
                                                             int lda, double *A, double *Y, int *info)
{
    const long b = (long)blockIdx.x * T + threadIdx.x / (W * 64);
    const bool in = b < B * cap;
    const long seg = in ? b / cap : 0;
    linsolve_team<IN_LDS>(b, in && b - seg * cap < count[seg], n, K, W, RL, lda, A, Y, info);
}
#endif

}  // namespace

#ifdef SOCP_TANGENT_FAST
#define SOCP_TANGENT_NAME(name) name##_fast
#else
#define SOCP_TANGENT_NAME(name) name
#endif

hipError_t SOCP_TANGENT_NAME(tangent_expand)(hipStream_t st, const ModelParams &P, const ProblemDev &pb, int nparams, int B, int K,
                                             const TangentDirs &dirs, double e, const double *Z, double *wP, double *wT, double *wX,
                                             double *wZ, double *wH)
{
    if (B <= 0 || K <= 0) return hipSuccess;
    hipLaunchKernelGGL(tangent_expand_kernel, dim3((unsigned)((long)B * (K + 1))), dim3(64), 0, st, P, pb, nparams, B, K, dirs, e, Z, wP, wT,
                       wX, wZ, wH);
    return hipGetLastError();
}

hipError_t SOCP_TANGENT_NAME(tangent_diff)(hipStream_t st, int B, int K, int n, const double *F, const double *H, double *rhs, double *Fp)
{
    if (B <= 0 || K <= 0 || n <= 0) return hipSuccess;
    const long total = (long)B * K * n;
    hipLaunchKernelGGL(tangent_diff_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, B, K, n, F, H, rhs, Fp);
    return hipGetLastError();
}

// team geometry from n (see the kernel); LDS path when the teams of a workgroup fit kLinsolveLdsBytes
hipError_t SOCP_TANGENT_NAME(linsolve)(hipStream_t st, int B, int n, int K, double *A, double *Y, int *info)
{
    if (B <= 0) return hipSuccess;
    const int W = linsolve_waves(n), T = linsolve_teams(n), RL = n <= 16 ? 16 : 64, lda = n | 1;
    const unsigned grid = (unsigned)(((long)B + T - 1) / T), block = (unsigned)(T * W * 64);
    const size_t lds_in = sizeof(double) * T * ((size_t)lda * (n + K) + kLinsolveScratch);
    if (lds_in <= (size_t)kLinsolveLdsBytes) {
        hipLaunchKernelGGL(linsolve_kernel<true>, dim3(grid), dim3(block), lds_in, st, (long)B, n, K, W, T, RL, lda, A, Y, info);
    } else {
        if (!linsolve_fits(n, K)) return hipErrorInvalidValue;
        const size_t lds = sizeof(double) * T * ((size_t)2 * n + K + kLinsolveScratch);
        hipLaunchKernelGGL(linsolve_kernel<false>, dim3(grid), dim3(block), lds, st, (long)B, n, K, W, T, RL, lda, A, Y, info);
    }
    return hipGetLastError();
}

#ifndef SOCP_TANGENT_FAST
hipError_t linsolve_slots(hipStream_t st, int B, int cap, const int *count, int n, int K, double *A, double *Y, int *info)
{
    if (B <= 0 || cap <= 0) return hipSuccess;
    const int W = linsolve_waves(n), T = linsolve_teams(n), RL = n <= 16 ? 16 : 64, lda = n | 1;
    const long slots = (long)B * cap;
    const unsigned grid = (unsigned)((slots + T - 1) / T), block = (unsigned)(T * W * 64);
    const size_t lds_in = sizeof(double) * T * ((size_t)lda * (n + K) + kLinsolveScratch);
    if (lds_in <= (size_t)kLinsolveLdsBytes) {
        hipLaunchKernelGGL(linsolve_slots_kernel<true>, dim3(grid), dim3(block), lds_in, st, (long)B, cap, count, n, K, W, T, RL, lda, A, Y, info);
    } else {
        if (!linsolve_fits(n, K)) return hipErrorInvalidValue;
        const size_t lds = sizeof(double) * T * ((size_t)2 * n + K + kLinsolveScratch);
        hipLaunchKernelGGL(linsolve_slots_kernel<false>, dim3(grid), dim3(block), lds, st, (long)B, cap, count, n, K, W, T, RL, lda, A, Y, info);
    }
    return hipGetLastError();
}
#endif

}  // namespace socp
