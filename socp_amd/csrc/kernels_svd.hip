// kernels_svd.hip -- the kernels of socp_svd_batch_dev / socp_singular_batch (include/socp_hip.h): the column norms of a batch of
// Jacobians, and the batched singular values by one-sided Jacobi rotations on the ROWS of each matrix.
// Built TWICE (socp_amd/csrc/Makefile): without -DSOCP_SVD_FAST and with -ffp-contract=off for reference-order contexts -- every
// operation is then a single IEEE rounding, the sums in the order socp_hip.h writes down -- and with -DSOCP_SVD_FAST and
// -ffp-contract=fast for throughput-flavour contexts (the sums and the rotations become fused multiply-adds).
// Model-independent: the Jacobians come from the model's own launch table (residual, fdjac, var_jacobian).
#include <atomic>
#include <cfloat>

#include "launch.hpp"

namespace socp {
namespace {

// ---- K_colscale: one thread per column (b, j): colnorm = sqrt(sum_i J_ij^2), the sum in the order i = 0 .. n-1; a zero becomes 1;
// J_ij <- J_ij / colnorm.  scale == 0: only colnorm = 1 is written.  colnorm may be null
__global__ __launch_bounds__(256) void colscale_kernel(long cols, int n, int scale, double *__restrict__ J, double *__restrict__ colnorm)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= cols) return;
    double norm = 1.0;
    if (scale) {
        double *col = J + e * n;
        double acc = 0.0;
        for (int i = 0; i < n; i++) acc = acc + col[i] * col[i];
        norm = sqrt(acc);
        if (norm == 0.0) norm = 1.0;
        for (int i = 0; i < n; i++) col[i] = col[i] / norm;
    }
    if (colnorm) colnorm[e] = norm;
}

// ---- K_svd: one matrix per TEAM of L lanes, T teams per workgroup; the matrix lives in LDS ---------------------------------------
// Row p of the matrix (entries A[p + i n]) is mat[p ld + 0 .. n-1], ld = n | 1.  A lane owns a pair (p, q) of a step: it walks both
// rows with i, so at one instruction the lanes of a wavefront read mat[p ld + i] for DIFFERENT p and the same i -- addresses ld
// doubles apart, and an odd ld visits every eight-byte bank before it repeats.  The three sums of a pair are sequential in one
// lane (no cross-lane reduction, so their order is the header's); the pairs of a step are disjoint, so a step needs no
// synchronisation inside and one barrier behind it.
// Scratch per team behind its matrix: sig[n] (the row norms, then the ranks) and kSvdFlags doubles holding the ints
//   [0 .. 2] "a pair of this team rotated" of sweep k in word k % 3 (cleared two sweeps ahead, so no barrier is spent on it)
//   [3]      "an entry is not finite"
// and, for the whole workgroup, in team 0's flags [4 .. 6]: "a team is still iterating" after sweep k, in word 4 + k % 3.
// Every thread reaches every barrier: a team that is finished (or has no matrix) idles through the steps of the others, and the
// sweep loop ends for the whole workgroup as soon as no team iterates, at the latest after max_sweeps.
// vt_mode: 0 no vectors, 1 Vt[B][n][n], 2 only the row of the smallest singular value, Vt[B][n].
__global__ __launch_bounds__(128) void svd_kernel(long B, int n, int ld, int L, int T, int max_sweeps, int vt_mode, const double *__restrict__ A,
                           double *__restrict__ sigma, double *__restrict__ Vt, int *__restrict__ sweeps, int *__restrict__ info)
{
    extern __shared__ double sm[];
    const int team = threadIdx.x / L, tt = threadIdx.x - team * L;
    const long b = (long)blockIdx.x * T + team;
    const bool live = b < B;                                        // (blockDim = L T: every thread has a team)
    const int team_doubles = n * ld + n + kSvdFlags;
    double *mat = sm + (long)team * team_doubles, *sig = mat + n * ld;
    int *flag = reinterpret_cast<int *>(sig + n), *wg = reinterpret_cast<int *>(sm + n * ld + n) + 4;
    const double *Ab = A + (live ? b : 0) * (long)n * n;
    const int m = n + (n & 1), half = m / 2, nn = n * n;

    if (live)
        for (int e = tt; e < 2 * kSvdFlags; e += L) flag[e] = 0;
    __syncthreads();
    if (live) {
        bool bad = false;
        for (int e = tt; e < nn; e += L) {                          // consecutive lanes read consecutive doubles of A
            const double v = Ab[e];
            const int i = e / n, p = e - i * n;
            mat[p * ld + i] = v;
            if (!(fabs(v) < INFINITY)) bad = true;
        }
        if (bad) flag[3] = 1;
    }
    __syncthreads();

    const double tol = (double)n * DBL_EPSILON;
    int my_info = -1, my_sweeps = 0;                                // -1: iterating; the same in all threads of a team
    if (!live) my_info = 0;
    else if (flag[3]) my_info = 2;

    for (int sweep = 1; sweep <= max_sweeps; sweep++) {
        const int w = sweep % 3, wnext = (sweep + 1) % 3;
        const bool act = my_info < 0;
        if (tt == 0) flag[wnext] = 0;
        if (threadIdx.x == 0) wg[wnext] = 0;
        bool rotated = false;
        for (int s = 0; s < m - 1; s++) {
            if (act)
                for (int k = tt; k < half; k += L) {
                    int a, c;
                    if (k == 0) { a = m - 1; c = s; }
                    else { a = (s + k) % (m - 1); c = (s - k + m - 1) % (m - 1); }
                    const int p = a < c ? a : c, q = a < c ? c : a;
                    if (q >= n) continue;                           // the phantom row of an odd n
                    double *__restrict__ wp = mat + p * ld, *__restrict__ wq = mat + q * ld;      // p != q: the rows do not overlap, so
                    double alpha = 0.0, beta = 0.0, gamma = 0.0;                                  // the loads of several i may go ahead
#pragma unroll 4
                    for (int i = 0; i < n; i++) {
                        const double x = wp[i], y = wq[i];
                        alpha = alpha + x * x;
                        beta = beta + y * y;
                        gamma = gamma + x * y;
                    }
                    if (gamma == 0.0 || fabs(gamma) <= (tol * sqrt(alpha)) * sqrt(beta)) continue;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll 4
                    for (int i = 0; i < n; i++) {
                        const double x = wp[i], y = wq[i];
                        wp[i] = cs * x - sn * y;
                        wq[i] = sn * x + cs * y;
                    }
                    rotated = true;
                }
            if (s == m - 2 && rotated) flag[w] = 1;
            __syncthreads();
        }
        if (act) {
            my_sweeps = sweep;
            if (!flag[w]) my_info = 0;
            else if (sweep == max_sweeps) my_info = 1;
            else wg[w] = 1;
        }
        __syncthreads();
        if (!wg[w]) break;                                          // the same word in every thread of the workgroup
    }

    // finish: row norms (the same sequential sum), ranks by counting, the normalised rows with their sign
    const bool ok = live && my_info != 2;
    if (ok)
        for (int p = tt; p < n; p += L) {
            const double *wp = mat + p * ld;
            double acc = 0.0;
            for (int i = 0; i < n; i++) acc = acc + wp[i] * wp[i];
            sig[p] = sqrt(acc);
        }
    __syncthreads();
    // a lane owns the rows tt and tt + L: L >= n / 2 (svd_lanes), so these are all
    int rank[2] = {0, 0};
    double sp[2] = {0.0, 0.0};
    if (ok) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int p = tt + r * L;
            if (p >= n) continue;
            const double s = sig[p];
            int cnt = 0;
            for (int q = 0; q < n; q++) {
                const double o = sig[q];
                cnt += (o > s || (o == s && q < p)) ? 1 : 0;
            }
            rank[r] = cnt; sp[r] = s;
        }
    }
    __syncthreads();
    if (ok) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int p = tt + r * L;
            if (p >= n) continue;
            const double s = sp[r];
            sigma[b * n + rank[r]] = s;
            sig[p] = (double)rank[r];
            if (vt_mode == 0 || (vt_mode == 2 && rank[r] != n - 1)) continue;
            double *wp = mat + p * ld;
            double big = -1.0, at_big = 0.0;
            for (int i = 0; i < n; i++) {
                const double v = s == 0.0 ? 0.0 : wp[i] / s;
                wp[i] = v;
                if (fabs(v) > big) { big = fabs(v); at_big = v; }   // the first among equals
            }
            if (at_big < 0.0)
                for (int i = 0; i < n; i++) wp[i] = -wp[i];
        }
    }
    __syncthreads();
    if (live) {
        if (tt == 0) { info[b] = my_info; sweeps[b] = my_sweeps; }
        const double nan = __longlong_as_double(0x7FF8000000000000LL);
        if (!ok)
            for (int e = tt; e < n; e += L) sigma[b * n + e] = nan;
        if (vt_mode == 1) {
            double *out = Vt + b * (long)nn;
            for (int e = tt; e < nn; e += L) {                      // consecutive lanes write consecutive doubles of a row
                const int p = e / n, i = e - p * n;
                if (ok) out[(long)((int)sig[p]) * n + i] = mat[p * ld + i];
                else out[e] = nan;
            }
        } else if (vt_mode == 2) {
            double *out = Vt + b * (long)n;
            if (!ok) {
                for (int e = tt; e < n; e += L) out[e] = nan;
            } else {
                for (int p = 0; p < n; p++)
                    if ((int)sig[p] == n - 1)
                        for (int i = tt; i < n; i += L) out[i] = mat[p * ld + i];
            }
        }
    }
}

// More than 64 KiB of dynamic LDS needs the kernel's limit raised, on the current device's copy of the kernel: remembered per device
hipError_t raise_lds_limit()
{
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 64 && ((raised.load(std::memory_order_acquire) >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(svd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSvdLdsBytes);
    if (e == hipSuccess && dev < 64) raised.fetch_or(1ull << dev, std::memory_order_release);
    return e;
}

}  // namespace

#ifdef SOCP_SVD_FAST
#define SOCP_SVD_NAME(name) name##_fast
#else
#define SOCP_SVD_NAME(name) name
#endif

hipError_t SOCP_SVD_NAME(svd_colscale)(hipStream_t st, int B, int n, int scale, double *J, double *colnorm)
{
    if (B <= 0 || n <= 0) return hipSuccess;
    const long cols = (long)B * n;
    hipLaunchKernelGGL(colscale_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, cols, n, scale, J, colnorm);
    return hipGetLastError();
}

hipError_t SOCP_SVD_NAME(svd)(hipStream_t st, int B, int n, const double *A, int max_sweeps, int vt_mode, double *sigma, double *Vt,
                              int *sweeps, int *info)
{
    if (B <= 0) return hipSuccess;
    if (!svd_fits(n)) return hipErrorInvalidValue;
    const int L = svd_lanes(n), T = svd_teams(n);
    const size_t lds = svd_lds_bytes(n);
    if (lds > 64 * 1024) {
        const hipError_t e = raise_lds_limit();
        if (e != hipSuccess) return e;
    }
    const unsigned grid = (unsigned)(((long)B + T - 1) / T);
    hipLaunchKernelGGL(svd_kernel, dim3(grid), dim3((unsigned)(L * T)), lds, st, (long)B, n, n | 1, L, T, max_sweeps, vt_mode, A, sigma, Vt,
                       sweeps, info);
    return hipGetLastError();
}

}  // namespace socp
