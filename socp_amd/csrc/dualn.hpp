// dualn.hpp -- forward-mode numbers with W derivative parts (v, d[0 .. W)) in ONE lane, for symplectic_gradient
// (hamiltonian_model.hpp).  Component k of every rule is Dual's rule (dual.hpp; include/socp_hip.h, "DUAL NUMBERS") on (v, d[k]), one
// IEEE rounding per listed step; the translation unit that uses them is built with -ffp-contract=off, so nothing is fused.  The value
// part is computed ONCE, and so is every intermediate that reads value parts only (a quotient's q, a root's s + s).  The components
// never meet: what component k holds does not depend on W, nor on which other directions travel beside it -- a gradient may be cut
// into passes of any width and gives the same bits (tests/hamiltonian_model_reference.py restates the rules and checks just that).
// A plain double takes part through the mixed overloads, which DROP its zero derivative terms, as in dual.hpp.  There is no implicit
// conversion from double.
#pragma once
#include "dual.hpp"

namespace socp {

template <int W>
struct DualN {
    static_assert(W >= 1, "at least one derivative part");
    double v, d[W];
    __device__ __forceinline__ DualN() {}
    __device__ __forceinline__ explicit DualN(double c) : v(c)
    {
#pragma unroll
        for (int k = 0; k < W; k++) d[k] = 0.0;
    }
};

// a +- b, -a
template <int W> __device__ __forceinline__ DualN<W> operator+(const DualN<W> &a, const DualN<W> &b)
{
    DualN<W> r;
    r.v = a.v + b.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] + b.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator-(const DualN<W> &a, const DualN<W> &b)
{
    DualN<W> r;
    r.v = a.v - b.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] - b.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator-(const DualN<W> &a)
{
    DualN<W> r;
    r.v = -a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = -a.d[k];
    return r;
}
// a b = (a.v b.v, (a.d b.v) + (a.v b.d))
template <int W> __device__ __forceinline__ DualN<W> operator*(const DualN<W> &a, const DualN<W> &b)
{
    DualN<W> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const double l = a.d[k] * b.v;
        const double m = a.v * b.d[k];
        r.d[k] = l + m;
    }
    return r;
}
// a / b: q = a.v / b.v; (q, (a.d - q b.d) / b.v)
template <int W> __device__ __forceinline__ DualN<W> operator/(const DualN<W> &a, const DualN<W> &b)
{
    DualN<W> r;
    const double q = a.v / b.v;
    r.v = q;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const double m = q * b.d[k];
        r.d[k] = (a.d[k] - m) / b.v;
    }
    return r;
}
// a plain double c: its zero derivative terms are dropped, not computed
template <int W> __device__ __forceinline__ DualN<W> operator+(double c, const DualN<W> &a)
{
    DualN<W> r;
    r.v = c + a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator+(const DualN<W> &a, double c)
{
    DualN<W> r;
    r.v = a.v + c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator-(double c, const DualN<W> &a)
{
    DualN<W> r;
    r.v = c - a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = -a.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator-(const DualN<W> &a, double c)
{
    DualN<W> r;
    r.v = a.v - c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator*(double c, const DualN<W> &a)
{
    DualN<W> r;
    r.v = c * a.v;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = c * a.d[k];
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator*(const DualN<W> &a, double c)
{
    DualN<W> r;
    r.v = a.v * c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] * c;
    return r;
}
template <int W> __device__ __forceinline__ DualN<W> operator/(const DualN<W> &a, double c)
{
    DualN<W> r;
    r.v = a.v / c;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.d[k] / c;
    return r;
}
// c / a: q = c / a.v; (q, (-(q a.d)) / a.v)
template <int W> __device__ __forceinline__ DualN<W> operator/(double c, const DualN<W> &a)
{
    DualN<W> r;
    const double q = c / a.v;
    r.v = q;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const double m = q * a.d[k];
        r.d[k] = (-m) / a.v;
    }
    return r;
}

// the value a comparison reads
template <int W> __device__ __forceinline__ double d_val(const DualN<W> &a) { return a.v; }
// |a| acts on all parts: every d flips when v < 0
template <int W> __device__ __forceinline__ DualN<W> d_abs(const DualN<W> &a)
{
    DualN<W> r;
    r.v = fabs(a.v);
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = a.v < 0.0 ? -a.d[k] : a.d[k];
    return r;
}
// sqrt a: s = sqrt(a.v); (s, a.d / (s + s)), the derivatives +0.0 when s == 0
template <int W> __device__ __forceinline__ DualN<W> d_sqrt(const DualN<W> &a)
{
    DualN<W> r;
    const double s = sqrt(a.v);
    const double s2 = s + s;
    r.v = s;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const double q = a.d[k] / s2;
        r.d[k] = s == 0.0 ? 0.0 : q;
    }
    return r;
}
// exp a: e = exp_glibc(a.v); (e, e a.d)
template <int W> __device__ __forceinline__ DualN<W> d_exp(const DualN<W> &a)
{
    DualN<W> r;
    const double e = exp_glibc(a.v);
    r.v = e;
#pragma unroll
    for (int k = 0; k < W; k++) r.d[k] = e * a.d[k];
    return r;
}

}  // namespace socp
