// dual.hpp -- forward-mode dual numbers (v, d) for socp_fields_batch.  The rules are those of include/socp_hip.h ("DUAL NUMBERS"),
// one IEEE rounding per listed step; the translation unit that uses them is built with -ffp-contract=off, so nothing is fused.
// A plain double (a parameter, a literal, t, h) takes part through the mixed overloads below, which DROP its zero derivative terms
// instead of computing them: (c * a).d is c * a.d, not a.d * c + a.v * 0.  The two differ in the sign of a zero and on a
// non-finite value, so a right-hand side written over T must keep a plain double plain wherever the definition does
// (tests/fields_reference.py restates the same text on the same rules).  There is no implicit conversion from double.
// The d_* helpers are overloaded on double too: a right-hand side templated on T then reads the same with T = double, where it
// must give the bits of the model's rhs.
#pragma once
#include "dev_common.hpp"
#include "exp_glibc.hpp"

namespace socp {

struct Dual {
    double v, d;
    __device__ __forceinline__ Dual() {}
    __device__ __forceinline__ explicit Dual(double c) : v(c), d(0.0) {}
    __device__ __forceinline__ Dual(double val, double der) : v(val), d(der) {}
};

// a +- b, -a
__device__ __forceinline__ Dual operator+(const Dual &a, const Dual &b) { return Dual(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ Dual operator-(const Dual &a, const Dual &b) { return Dual(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ Dual operator-(const Dual &a) { return Dual(-a.v, -a.d); }
// a b = (a.v b.v, (a.d b.v) + (a.v b.d))
__device__ __forceinline__ Dual operator*(const Dual &a, const Dual &b)
{
    const double l = a.d * b.v;
    const double r = a.v * b.d;
    return Dual(a.v * b.v, l + r);
}
// a / b: q = a.v / b.v; (q, (a.d - q b.d) / b.v)
__device__ __forceinline__ Dual operator/(const Dual &a, const Dual &b)
{
    const double q = a.v / b.v;
    const double m = q * b.d;
    return Dual(q, (a.d - m) / b.v);
}
// a plain double c: its zero derivative terms are dropped, not computed
__device__ __forceinline__ Dual operator+(double c, const Dual &a) { return Dual(c + a.v, a.d); }
__device__ __forceinline__ Dual operator+(const Dual &a, double c) { return Dual(a.v + c, a.d); }
__device__ __forceinline__ Dual operator-(double c, const Dual &a) { return Dual(c - a.v, -a.d); }
__device__ __forceinline__ Dual operator-(const Dual &a, double c) { return Dual(a.v - c, a.d); }
__device__ __forceinline__ Dual operator*(double c, const Dual &a) { return Dual(c * a.v, c * a.d); }
__device__ __forceinline__ Dual operator*(const Dual &a, double c) { return Dual(a.v * c, a.d * c); }
__device__ __forceinline__ Dual operator/(const Dual &a, double c) { return Dual(a.v / c, a.d / c); }
// c / a: q = c / a.v; (q, (-(q a.d)) / a.v)
__device__ __forceinline__ Dual operator/(double c, const Dual &a)
{
    const double q = c / a.v;
    const double m = q * a.d;
    return Dual(q, (-m) / a.v);
}

// the value a comparison reads
__device__ __forceinline__ double d_val(double a) { return a; }
__device__ __forceinline__ double d_val(const Dual &a) { return a.v; }
// |a| acts on both parts: d flips when v < 0
__device__ __forceinline__ double d_abs(double a) { return fabs(a); }
__device__ __forceinline__ Dual d_abs(const Dual &a) { return Dual(fabs(a.v), a.v < 0.0 ? -a.d : a.d); }
// sqrt a: s = sqrt(a.v); (s, a.d / (s + s)), the derivative +0.0 when s == 0
__device__ __forceinline__ double d_sqrt(double a) { return sqrt(a); }
__device__ __forceinline__ Dual d_sqrt(const Dual &a)
{
    const double s = sqrt(a.v);
    const double q = a.d / (s + s);
    return Dual(s, s == 0.0 ? 0.0 : q);
}
// exp a: e = exp_glibc(a.v); (e, e a.d)
__device__ __forceinline__ double d_exp(double a) { return exp_glibc(a); }
__device__ __forceinline__ Dual d_exp(const Dual &a)
{
    const double e = exp_glibc(a.v);
    return Dual(e, e * a.d);
}
// tanh a: th = tanh(a.v), the device library's; (th, (1.0 - th th) a.d)
__device__ __forceinline__ double d_tanh(double a) { return tanh(a); }
__device__ __forceinline__ Dual d_tanh(const Dual &a)
{
    const double th = tanh(a.v);
    return Dual(th, (1.0 - th * th) * a.d);
}

}  // namespace socp
