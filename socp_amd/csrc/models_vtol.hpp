// models_vtol.hpp -- device twin of the reference's `vtolUAV` waypoint model (vtolUAV.cpp:58-278) together
// with the penalty map its right-hand side reads (obstacle.cpp:155-319).
//
// State [x, y, z, vx, vy, vz ; p_x, p_y, p_z, p_vx, p_vy, p_vz], control dimension 3, state-only (modelOrder 0).
// The reference's map is a host object with file I/O; once its file has been read it is a table of boxes and
// ellipsoids and its gradient is closed-form arithmetic.  Here the table lives in a device buffer the context
// owns (socp_ctx_set_map): 7 doubles per obstacle -- type, centre xyz, radii xyz -- and the map's four scalars
// (phiObs, psiWP, muObs, sigmaWP) travel in the packed parameter block, because continuation chains vary muObs.
//
// The table is read through ModelParams::map / n_map, which arrive as kernel arguments, with the obstacle
// index a loop counter: address and trip count are wave-invariant by construction.  That alone gives scalar
// loads only in kernels that store nothing the compiler could confuse with the table; the pointer is therefore
// taken into the constant address space (MapTable below), and then every kernel reads the table through the
// scalar cache -- one read per wave, not per lane (scripts/vtol_table_loads.py counts it in the ISA).
//
// VtolExact: the reference's operation order, IEEE division and square root, no contraction; tanh is the
// device library's, so -- unlike Goddard's exp -- rows 6..8 of the RHS and the Hamiltonian are NOT bit-identical
// to the CPU path (every other row is).  Pinned to reference-generated vectors (tests/test_gpu_vtol.py).
// VtolFast: restructured; one exponential per box and axis serves 1 - tanh h and 1 - tanh^2 h.
// Both are held per component to a 240-bit evaluation within a derived bound (tests/test_gpu_vtol_pin.py).
//
// Upstream quirks kept on purpose: the ellipsoid gradient's `rad` omits the z term and its z component is zero;
// only the obstacle part of the map is live (the waypoint part is commented out upstream: psiWP multiplies zero);
// a position exactly on a box's centre plane makes the term NaN and the isnan reset then zeroes the WHOLE
// component; normV = 0 gives NaN in rows 9..11 (0 / 0) and nowhere else, in both flavours.
#pragma once
#include "dual.hpp"
#include "integrator.hpp"

namespace socp {

enum VtolParam {
    VP_UMAX = 0, VP_AMAX, VP_ALPHAT, VP_ALPHAV, VP_INVSIGMAXWP, VP_VD, VP_CA, VP_NWP_TOT, VP_NWP,
    VP_PHIOBS, VP_PSIWP, VP_MUOBS, VP_SIGMAWP, VP_COUNT
};

// The obstacle table as the kernels read it: a pointer into the CONSTANT address space.  The table is written by
// socp_ctx_set_map before a launch and by nothing during one, which is what that address space promises; with it a load whose
// address is wave-invariant goes to the scalar cache whatever the kernel stores elsewhere.  Through the plain global pointer
// the residual / FD-rows / dense kernels, which store to buffers the compiler cannot tell from the table, read it with
// vector loads of a uniform address instead (four VMEM instructions per wave, obstacle and RK4 stage).
typedef const __attribute__((address_space(4))) double *MapTable;
__device__ __forceinline__ MapTable map_table(const ModelParams &P) { return (MapTable)P.map; }

namespace vfast {
__device__ __forceinline__ double rcp(double x)
{
    const double r = __builtin_amdgcn_rcp(x);
    const double e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, __builtin_fma(e, e, e), r);
}
__device__ __forceinline__ double rsqrt(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    const double d = __builtin_fma(-(x * y), y, 1.0);
    return __builtin_fma(y * d, __builtin_fma(0.375, d, 0.5), y);
}
}  // namespace vfast

template <bool FAST>
struct VtolT {
    static constexpr int D = 6;
    static constexpr int S = 12;
    static constexpr int NU = 3;
    static constexpr bool kRefOrder = !FAST;
    static constexpr bool kCustomFinal = true;
    static constexpr bool kNoJacobi = true;          // socp_jacobi_batch is not offered for this model (plugin_impl.hpp)

    // vtolUAV.cpp:107-143
    __device__ static __forceinline__ void control_only(const ModelParams &P, double, double, double, const double (&X)[S], double (&u)[3])
    {
        const double a_max = P.p[VP_AMAX], u_max = P.p[VP_UMAX];
        u[0] = -X[9] / a_max;  u[1] = -X[10] / a_max;  u[2] = -X[11] / a_max;
        const double norm_u = sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        if (norm_u > u_max) {
            u[0] = u[0] / norm_u * u_max;
            u[1] = u[1] / norm_u * u_max;
            u[2] = u[2] / norm_u * u_max;
        }
    }

    // ---- observables (socp_observe_batch, include/socp_hip.h has the definitions) ---------------------------
    // clearance: the smallest level of any obstacle of the table, negative inside one.  Plain IEEE operations in the order written,
    // never contracted (the pragma), so both flavours give the same bits; no tanh.  A NaN level (an ellipsoid's centre) never
    // displaces the running minimum; an empty table gives +inf.  The table is read like map_exact reads it.
    __device__ static __forceinline__ double clearance(const ModelParams &P, double px, double py, double pz)
    {
#pragma clang fp contract(off)
        double cl = __builtin_inf();
        const MapTable tab = map_table(P);
        for (int i = 0; i < P.n_map; i++) {
            const MapTable o = tab + (long)i * kMapStride;
            const double type = o[0], x = o[1], y = o[2], z = o[3], radx = o[4], rady = o[5], radz = o[6];
            if (type == 0) {
                const double hx = px - x, hy = py - y, hz = pz - z;
                const double d = sqrt(hx*hx + hy*hy + hz*hz);
                const double level = d - d / sqrt(hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz);
                if (level < cl) cl = level;
            } else if (type == 1) {
                const double dx = px - x, dy = py - y, dz = pz - z;
                double m = fabs(dx) - radx;
                const double b = fabs(dy) - rady, c = fabs(dz) - radz;
                if (b > m) m = b;
                if (c > m) m = c;
                if (m < cl) cl = m;
            }
        }
        return cl;
    }
    static constexpr int kObservables = 3;
    static constexpr const char *kObservableNames[kObservables] = {"speed", "norm_u", "clearance"};
    __device__ static __forceinline__ void observe(const ModelParams &P, double, double, double, const double (&X)[S], const double (&u)[NU],
                                                  double (&y)[kObservables])
    {
        y[0] = sqrt(X[3]*X[3] + X[4]*X[4] + X[5]*X[5]);
        y[1] = sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        y[2] = clearance(P, X[0], X[1], X[2]);
    }

    // ---- reference-order map (obstacle.cpp:186-319) ------------------------------------------------------
    // WANT_F / WANT_G: the penalty value (Function) and / or its gradient (Gradient), as the reference's two loops
    template <bool WANT_F, bool WANT_G>
    __device__ static __forceinline__ void map_exact(const ModelParams &P, double px, double py, double pz, double &func, double (&grad)[3])
    {
        const double mu = P.p[VP_MUOBS];
        double f = 0, g0 = 0, g1 = 0, g2 = 0;
        const MapTable tab = map_table(P);
        for (int i = 0; i < P.n_map; i++) {
            const MapTable o = tab + (long)i * kMapStride;
            const double type = o[0], x = o[1], y = o[2], z = o[3], radx = o[4], rady = o[5], radz = o[6];
            if (type == 0) {
                const double hx = px - x, hy = py - y, hz = pz - z;
                const double d = sqrt(hx*hx + hy*hy + hz*hz);
                if constexpr (WANT_F) {
                    const double rad = d / sqrt(hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz);
                    const double h = (d - rad) / mu;
                    f = f + (1 - tanh(h)) / 2;
                }
                if constexpr (WANT_G) {
                    const double q = sqrt(hx*hx / radx / radx + hy*hy / rady / rady);
                    const double rad = d / q;                   // the z term is missing upstream (obstacle.cpp:258)
                    const double h = (d - rad) / mu;
                    const double rho2 = (radx*radx - rady*rady) / (radx*radx*rady*rady) / q / q / q;
                    const double th = tanh(h);
                    g0 = g0 - hx / d*(1 - hy*hy*rho2) / mu*(1 - th*th) / 2;
                    g1 = g1 - hy / d*(1 + hx*hx*rho2) / mu*(1 - th*th) / 2;
                    g2 = g2 - 0;
                }
            } else if (type == 1) {
                const double dx = px - x, dy = py - y, dz = pz - z;
                const double thx = tanh((fabs(dx) - radx) / mu);
                const double thy = tanh((fabs(dy) - rady) / mu);
                const double thz = tanh((fabs(dz) - radz) / mu);
                if constexpr (WANT_F) f = f + (1 - thx)*(1 - thy)*(1 - thz) / 8;
                if constexpr (WANT_G) {
                    g0 = g0 - dx / fabs(dx) / mu*(1 - thx*thx)*(1 - thy)*(1 - thz) / 8;
                    g1 = g1 - dy / fabs(dy) / mu*(1 - thy*thy)*(1 - thx)*(1 - thz) / 8;
                    g2 = g2 - dz / fabs(dz) / mu*(1 - thz*thz)*(1 - thx)*(1 - thy) / 8;
                }
            }
        }
        if (f != f) f = 0.0;
        if (g0 != g0) g0 = 0.0;
        if (g1 != g1) g1 = 0.0;
        if (g2 != g2) g2 = 0.0;
        // obstacle.cpp:155-181: the waypoint part is commented out upstream, its weight multiplies a zero
        const double phi = P.p[VP_PHIOBS], psi = P.p[VP_PSIWP];
        if constexpr (WANT_F) func = phi*f + psi*0.0;
        if constexpr (WANT_G) { grad[0] = phi*g0 + psi*0.0; grad[1] = phi*g1 + psi*0.0; grad[2] = phi*g2 + psi*0.0; }
    }

    // ---- restructured map ----------------------------------------------------------------------------------
    // e = exp(-2|h|) never overflows; with q = 1/(1 + e):  1 - tanh h = 2 e q (h >= 0) or 2 q (h < 0),  1 - tanh^2 h = 4 e q^2.
    // The three axes of a box share ONE reciprocal: every 1 + e lies in [1, 2].
    struct Axis { double e, w; bool pos; };      // w = 1 + e
    __device__ static __forceinline__ Axis axis(double h)
    {
        Axis a;
        a.pos = h >= 0;
        a.e = exp(-2.0 * fabs(h));
        a.w = 1.0 + a.e;
        return a;
    }
    template <bool WANT_F, bool WANT_G>
    __device__ static __forceinline__ void map_fast(const ModelParams &P, double px, double py, double pz, double &func, double (&grad)[3])
    {
        const double mu = P.p[VP_MUOBS];
        const double inv_mu = vfast::rcp(mu);
        const double nan = __builtin_nan("");
        double f = 0, g0 = 0, g1 = 0, g2 = 0;
        const MapTable tab = map_table(P);
        for (int i = 0; i < P.n_map; i++) {
            const MapTable o = tab + (long)i * kMapStride;
            const double type = o[0], x = o[1], y = o[2], z = o[3], radx = o[4], rady = o[5], radz = o[6];
            if (type == 0) {
                const double hx = px - x, hy = py - y, hz = pz - z;
                const double d2 = hx*hx + hy*hy + hz*hz;
                const double inv_d = vfast::rsqrt(d2);
                const double d = d2 * inv_d;
                const double ax = hx*hx*vfast::rcp(radx*radx), ay = hy*hy*vfast::rcp(rady*rady), az = hz*hz*vfast::rcp(radz*radz);
                if constexpr (WANT_F) {
                    const double h = (d - d * vfast::rsqrt(ax + ay + az)) * inv_mu;
                    const Axis a = axis(h);
                    const double q = vfast::rcp(a.w);
                    f += a.pos ? a.e * q : q;                                  // (1 - tanh h) / 2
                }
                if constexpr (WANT_G) {
                    const double iq = vfast::rsqrt(ax + ay);
                    const double h = (d - d * iq) * inv_mu;
                    const double rho2 = (radx*radx - rady*rady) * vfast::rcp(radx*radx*rady*rady) * (iq*iq*iq);
                    const Axis a = axis(h);
                    const double q = vfast::rcp(a.w);
                    const double s2 = 2.0 * a.e * q * q * inv_mu;             // (1 - tanh^2 h) / 2 / mu
                    g0 -= hx * inv_d * (1 - hy*hy*rho2) * s2;
                    g1 -= hy * inv_d * (1 + hx*hx*rho2) * s2;
                }
            } else if (type == 1) {
                const double dx = px - x, dy = py - y, dz = pz - z;
                const Axis a = axis((fabs(dx) - radx) * inv_mu), b = axis((fabs(dy) - rady) * inv_mu), c = axis((fabs(dz) - radz) * inv_mu);
                const double bc = b.w * c.w;
                const double r = vfast::rcp(a.w * bc);
                const double qa = r * bc, qb = r * (a.w * c.w), qc = r * (a.w * b.w);
                // m = (1 - tanh h) / 2
                const double ma = a.pos ? a.e * qa : qa, mb = b.pos ? b.e * qb : qb, mc = c.pos ? c.e * qc : qc;
                if constexpr (WANT_F) f += ma * mb * mc;
                if constexpr (WANT_G) {
                    // (1 - tanh^2 h) / 8 / mu * 4 = e q^2 / 2 / mu ... with the two other factors 2 m each: e q^2 m m' * 2 / mu
                    const double k = 2.0 * inv_mu;
                    const double sx = dx > 0 ? 1.0 : (dx < 0 ? -1.0 : nan);     // 0 / |0| is NaN upstream: the reset below needs it
                    const double sy = dy > 0 ? 1.0 : (dy < 0 ? -1.0 : nan);
                    const double sz = dz > 0 ? 1.0 : (dz < 0 ? -1.0 : nan);
                    g0 -= sx * (k * a.e * qa * qa) * (mb * mc);
                    g1 -= sy * (k * b.e * qb * qb) * (ma * mc);
                    g2 -= sz * (k * c.e * qc * qc) * (ma * mb);
                }
            }
        }
        if (f != f) f = 0.0;
        if (g0 != g0) g0 = 0.0;
        if (g1 != g1) g1 = 0.0;
        if (g2 != g2) g2 = 0.0;
        const double phi = P.p[VP_PHIOBS];
        if constexpr (WANT_F) func = phi * f;
        if constexpr (WANT_G) { grad[0] = phi * g0; grad[1] = phi * g1; grad[2] = phi * g2; }
    }

    template <bool WANT_F, bool WANT_G>
    __device__ static __forceinline__ void map_eval(const ModelParams &P, double px, double py, double pz, double &func, double (&grad)[3])
    {
        if constexpr (FAST) map_fast<WANT_F, WANT_G>(P, px, py, pz, func, grad);
        else map_exact<WANT_F, WANT_G>(P, px, py, pz, func, grad);
    }

    // vtolUAV.cpp:58-104
    __device__ static __forceinline__ void rhs(const ModelParams &P, double sw0, double sw1, double t, const double (&X)[S], double (&dX)[S])
    {
        const double vx = X[3], vy = X[4], vz = X[5], p_x = X[6], p_y = X[7], p_z = X[8], p_vx = X[9], p_vy = X[10], p_vz = X[11];
        const double a_max = P.p[VP_AMAX], ca = P.p[VP_CA], alphaV = P.p[VP_ALPHAV], Vd = P.p[VP_VD];
        double u[3], g[3], unused;
        control_only(P, sw0, sw1, t, X, u);
        map_eval<false, true>(P, X[0], X[1], X[2], unused, g);
        dX[0] = vx;  dX[1] = vy;  dX[2] = vz;
        dX[6] = 0 - g[0];  dX[7] = 0 - g[1];  dX[8] = 0 - g[2];
        if constexpr (FAST) {
            const double v2 = vx*vx + vy*vy + vz*vz;
            const double inv = vfast::rsqrt(v2);
            // rsqrt(0) is NaN: at rest normV is v2 itself, so rows 3..5 stay finite as upstream (rows 9..11 are NaN there, as upstream)
            const double normV = v2 > 0 ? v2 * inv : v2;
            dX[3] = a_max*u[0] - ca*vx*normV;
            dX[4] = a_max*u[1] - ca*vy*normV;
            dX[5] = a_max*u[2] - ca*vz*normV;
            // ca (p_v normV + v (p_v . v)/normV) - alphaV v (normV - Vd)/normV
            const double pv = (p_vx*vx + p_vy*vy + p_vz*vz) * inv;
            const double w = alphaV * (normV - Vd) * inv;
            dX[9]  = -p_x + ca*(p_vx*normV + vx*pv) - w*vx;
            dX[10] = -p_y + ca*(p_vy*normV + vy*pv) - w*vy;
            dX[11] = -p_z + ca*(p_vz*normV + vz*pv) - w*vz;
        } else {
            const double normV = sqrt(vx*vx + vy*vy + vz*vz);
            dX[3] = a_max*u[0] - ca*vx*normV;
            dX[4] = a_max*u[1] - ca*vy*normV;
            dX[5] = a_max*u[2] - ca*vz*normV;
            dX[9]  = -p_x + ca*( p_vx*(normV + vx*vx/normV) + p_vy*(vy*vx/normV) + p_vz*(vz*vx/normV) ) - alphaV*vx/normV*(normV - Vd);
            dX[10] = -p_y + ca*( p_vy*(normV + vy*vy/normV) + p_vx*(vx*vy/normV) + p_vz*(vz*vy/normV) ) - alphaV*vy/normV*(normV - Vd);
            dX[11] = -p_z + ca*( p_vz*(normV + vz*vz/normV) + p_vx*(vx*vz/normV) + p_vy*(vy*vz/normV) ) - alphaV*vz/normV*(normV - Vd);
        }
    }

    // vtolUAV.cpp:146-190
    __device__ static double hamiltonian(const ModelParams &P, double sw0, double sw1, double t, const double (&X)[S])
    {
        const double vx = X[3], vy = X[4], vz = X[5], p_x = X[6], p_y = X[7], p_z = X[8], p_vx = X[9], p_vy = X[10], p_vz = X[11];
        const double a_max = P.p[VP_AMAX], ca = P.p[VP_CA], alphaV = P.p[VP_ALPHAV], Vd = P.p[VP_VD];
        const double normV = sqrt(vx*vx + vy*vy + vz*vz);
        double u[3], g[3], obs = 0;
        control_only(P, sw0, sw1, t, X, u);
        const double norm_u = sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        map_eval<true, false>(P, X[0], X[1], X[2], obs, g);
        return P.p[VP_ALPHAT]*1
             + alphaV / 2*(normV - Vd)*(normV - Vd)
             + obs
             + a_max*a_max*norm_u*norm_u / 2
             + p_x*vx + p_y*vy + p_z*vz
             + (p_vx*(a_max*u[0] - ca*vx*normV) + p_vy*(a_max*u[1] - ca*vy*normV) + p_vz*(a_max*u[2] - ca*vz*normV));
    }

    // model.hpp:299-304 default: H(t, X-) - H(t, X+)
    __device__ static double switching_fn(const ModelParams &P, double sw0, double sw1, double t, const double (&X)[S], const double (&Xp)[S])
    {
        return hamiltonian(P, sw0, sw1, t, X) - hamiltonian(P, sw0, sw1, t, Xp);
    }

    // vtolUAV.cpp:217-258: a FREE component's transversality row carries the waypoint weights; FinalHFunction adds H alone
    __device__ static __forceinline__ double final_row(const ModelParams &P, int j, int mode, const double (&X)[S], const double *xd)
    {
        const double dxj = X[j] - xd[j];
        if (mode == 1) return X[j + D] - P.p[VP_INVSIGMAXWP]*(P.p[VP_NWP_TOT] - P.p[VP_NWP])*dxj - 0.02*dxj;
        return dxj;
    }
    __device__ static __forceinline__ double final_h_offset(const ModelParams &) { return 0.0; }

    // vtolUAV.cpp:268-278
    __device__ static __forceinline__ void switching_state(const ModelParams &P, double, int j, const double (&X)[S], const double (&Xp)[S],
                                                          const double *Xd, double &f_state, double &f_costate)
    {
        f_state = X[j] - Xp[j];
        f_costate = (X[j + D] - Xp[j + D]) - P.p[VP_INVSIGMAXWP]*(X[j] - Xd[j]);
    }

    // ---- the texts over a number type T (socp_fields_batch, socp_exact_jacobian_batch: T = Dual, dual.hpp) -------------------
    // control_only, map_exact, rhs (the reference-order arm), hamiltonian, switching_fn, final_row and switching_state operation
    // for operation, d_sqrt / d_abs / d_tanh for the functions; the parameters, the table and the literals stay plain doubles.
    // With T = double: the bits of the plain texts.  Decisions read value parts: the saturation differentiates the branch taken,
    // the NaN reset tests the value and zeroes the whole number (a NaN derivative under a finite value stays).  The quirks stay.
    template <class T>
    __device__ static __forceinline__ void control_t(const ModelParams &P, const T (&X)[S], T (&u)[3])
    {
        const double a_max = P.p[VP_AMAX], u_max = P.p[VP_UMAX];
        u[0] = -X[9] / a_max;  u[1] = -X[10] / a_max;  u[2] = -X[11] / a_max;
        const T norm_u = d_sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        if (d_val(norm_u) > u_max) {
            u[0] = u[0] / norm_u * u_max;
            u[1] = u[1] / norm_u * u_max;
            u[2] = u[2] / norm_u * u_max;
        }
    }

    template <bool WANT_F, bool WANT_G, class T>
    __device__ static __forceinline__ void map_exact_t(const ModelParams &P, const T &px, const T &py, const T &pz, T &func, T (&grad)[3])
    {
        const double mu = P.p[VP_MUOBS];
        T f = T(0.0), g0 = T(0.0), g1 = T(0.0), g2 = T(0.0);
        const MapTable tab = map_table(P);
        for (int i = 0; i < P.n_map; i++) {
            const MapTable o = tab + (long)i * kMapStride;
            const double type = o[0], x = o[1], y = o[2], z = o[3], radx = o[4], rady = o[5], radz = o[6];
            if (type == 0) {
                const T hx = px - x, hy = py - y, hz = pz - z;
                const T d = d_sqrt(hx*hx + hy*hy + hz*hz);
                if constexpr (WANT_F) {
                    const T rad = d / d_sqrt(hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz);
                    const T h = (d - rad) / mu;
                    f = f + (1 - d_tanh(h)) / 2;
                }
                if constexpr (WANT_G) {
                    const T q = d_sqrt(hx*hx / radx / radx + hy*hy / rady / rady);
                    const T rad = d / q;                        // the z term is missing upstream (obstacle.cpp:258)
                    const T h = (d - rad) / mu;
                    const T rho2 = (radx*radx - rady*rady) / (radx*radx*rady*rady) / q / q / q;
                    const T th = d_tanh(h);
                    g0 = g0 - hx / d*(1 - hy*hy*rho2) / mu*(1 - th*th) / 2;
                    g1 = g1 - hy / d*(1 + hx*hx*rho2) / mu*(1 - th*th) / 2;
                    g2 = g2 - 0;
                }
            } else if (type == 1) {
                const T dx = px - x, dy = py - y, dz = pz - z;
                const T thx = d_tanh((d_abs(dx) - radx) / mu);
                const T thy = d_tanh((d_abs(dy) - rady) / mu);
                const T thz = d_tanh((d_abs(dz) - radz) / mu);
                if constexpr (WANT_F) f = f + (1 - thx)*(1 - thy)*(1 - thz) / 8;
                if constexpr (WANT_G) {
                    g0 = g0 - dx / d_abs(dx) / mu*(1 - thx*thx)*(1 - thy)*(1 - thz) / 8;
                    g1 = g1 - dy / d_abs(dy) / mu*(1 - thy*thy)*(1 - thx)*(1 - thz) / 8;
                    g2 = g2 - dz / d_abs(dz) / mu*(1 - thz*thz)*(1 - thx)*(1 - thy) / 8;
                }
            }
        }
        if (d_val(f) != d_val(f)) f = T(0.0);
        if (d_val(g0) != d_val(g0)) g0 = T(0.0);
        if (d_val(g1) != d_val(g1)) g1 = T(0.0);
        if (d_val(g2) != d_val(g2)) g2 = T(0.0);
        const double phi = P.p[VP_PHIOBS], psi = P.p[VP_PSIWP];
        if constexpr (WANT_F) func = phi*f + psi*0.0;
        if constexpr (WANT_G) { grad[0] = phi*g0 + psi*0.0; grad[1] = phi*g1 + psi*0.0; grad[2] = phi*g2 + psi*0.0; }
    }

    template <class T>
    __device__ static __forceinline__ void rhs_t(const ModelParams &P, double, double, double, const T (&X)[S], T (&dX)[S])
    {
        const T vx = X[3], vy = X[4], vz = X[5], p_x = X[6], p_y = X[7], p_z = X[8], p_vx = X[9], p_vy = X[10], p_vz = X[11];
        const double a_max = P.p[VP_AMAX], ca = P.p[VP_CA], alphaV = P.p[VP_ALPHAV], Vd = P.p[VP_VD];
        T u[3], g[3], unused;
        control_t<T>(P, X, u);
        map_exact_t<false, true, T>(P, X[0], X[1], X[2], unused, g);
        dX[0] = vx;  dX[1] = vy;  dX[2] = vz;
        dX[6] = 0 - g[0];  dX[7] = 0 - g[1];  dX[8] = 0 - g[2];
        const T normV = d_sqrt(vx*vx + vy*vy + vz*vz);
        dX[3] = a_max*u[0] - ca*vx*normV;
        dX[4] = a_max*u[1] - ca*vy*normV;
        dX[5] = a_max*u[2] - ca*vz*normV;
        dX[9]  = -p_x + ca*( p_vx*(normV + vx*vx/normV) + p_vy*(vy*vx/normV) + p_vz*(vz*vx/normV) ) - alphaV*vx/normV*(normV - Vd);
        dX[10] = -p_y + ca*( p_vy*(normV + vy*vy/normV) + p_vx*(vx*vy/normV) + p_vz*(vz*vy/normV) ) - alphaV*vy/normV*(normV - Vd);
        dX[11] = -p_z + ca*( p_vz*(normV + vz*vz/normV) + p_vx*(vx*vz/normV) + p_vy*(vy*vz/normV) ) - alphaV*vz/normV*(normV - Vd);
    }

    template <class T>
    __device__ static __forceinline__ T hamiltonian_t(const ModelParams &P, double, double, double, const T (&X)[S])
    {
        const T vx = X[3], vy = X[4], vz = X[5], p_x = X[6], p_y = X[7], p_z = X[8], p_vx = X[9], p_vy = X[10], p_vz = X[11];
        const double a_max = P.p[VP_AMAX], ca = P.p[VP_CA], alphaV = P.p[VP_ALPHAV], Vd = P.p[VP_VD];
        const T normV = d_sqrt(vx*vx + vy*vy + vz*vz);
        T u[3], g[3], obs = T(0.0);
        control_t<T>(P, X, u);
        const T norm_u = d_sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]);
        map_exact_t<true, false, T>(P, X[0], X[1], X[2], obs, g);
        return P.p[VP_ALPHAT]*1
             + alphaV / 2*(normV - Vd)*(normV - Vd)
             + obs
             + a_max*a_max*norm_u*norm_u / 2
             + p_x*vx + p_y*vy + p_z*vz
             + (p_vx*(a_max*u[0] - ca*vx*normV) + p_vy*(a_max*u[1] - ca*vy*normV) + p_vz*(a_max*u[2] - ca*vz*normV));
    }

    // H(t, X-) - H(t, X+): the lanes of the next segment own -grad H(X+)
    static constexpr bool kSwitchingReadsXp = true;
    template <class T>
    __device__ static __forceinline__ T switching_fn_t(const ModelParams &P, double sw0, double sw1, double t, const T (&X)[S], const T (&Xp)[S])
    {
        return hamiltonian_t<T>(P, sw0, sw1, t, X) - hamiltonian_t<T>(P, sw0, sw1, t, Xp);
    }

    // final_row on T; final_h_offset stays plain
    template <class T>
    __device__ static __forceinline__ T final_row_t(const ModelParams &P, int j, int mode, const T (&X)[S], const double *xd)
    {
        const T dxj = X[j] - xd[j];
        if (mode == 1) return X[j + D] - P.p[VP_INVSIGMAXWP]*(P.p[VP_NWP_TOT] - P.p[VP_NWP])*dxj - 0.02*dxj;
        return dxj;
    }

    // switching_state with X on T and the node's unknowns Xp as the plain doubles they are: Xp enters only as -Xp[j] in f_state and
    // -Xp[j + D] in f_costate, which is what kSwitchingStateXpContinuous promises (exact_jacobian.hpp)
    static constexpr bool kSwitchingStateXpContinuous = true;
    template <class T>
    __device__ static __forceinline__ void switching_state_t(const ModelParams &P, double, int j, const T (&X)[S], const double (&Xp)[S],
                                                            const double *Xd, T &f_state, T &f_costate)
    {
        f_state = X[j] - Xp[j];
        f_costate = (X[j + D] - Xp[j + D]) - P.p[VP_INVSIGMAXWP]*(X[j] - Xd[j]);
    }
};

using VtolExact = VtolT<false>;
using VtolFast = VtolT<true>;

// vtolUAV.cpp:24-36 and obstacle.cpp:49-52 constructor defaults in VtolParam order; ModelInt uses data->stepNbr = 100
#define SOCP_VTOL_DEFAULTS {10, 0.3, 0.05, 0 * 0.05, 1. / 60, 1, 0 * 0.05, 0, 0, 1, 0.03, 1, 2.5}

}  // namespace socp
