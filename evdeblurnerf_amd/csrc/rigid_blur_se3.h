// SE(3) exponential of the rigid blur kernel and its analytic derivative (SE3Field.get_transform / warp, RigidBody.exp_se3 / exp_so3,
// utils/rigid_warping.py:18-49,72-110), one (ray, motion) at a time.  With rot = rho, trans = tau, theta = |rho| + 1e-10 the reference's
//     R x = x + sin(theta) W x + (1 - cos(theta)) W W x,   p = (theta I + (1 - cos(theta)) W + (theta - sin(theta)) W W) tau / theta,   W = skew(rho / theta)
// is, in rho and tau themselves,
//     R x = x + A rho x x + B rho x (rho x x),   p = tau + B rho x tau + C rho x (rho x tau)
//     A = sin(theta) / theta,  B = (1 - cos(theta)) / theta^2,  C = (theta - sin(theta)) / theta^3.
// B is formed as 2 sin^2(theta / 2) / theta^2; C and the two remainders the derivatives need,
//     D = (1/2 - B) / theta^2,  E = (1/6 - C) / theta^2,
// by their series below theta = 1 (RB_SERIES_BELOW; six terms: the first one left out is below 2e-10 of the value) and directly above.
// Then A' = theta (C - B), B' = theta (2 D - C), C' = theta (3 E - D) have no cancelling difference at any theta.  The reference's float32
// autograd differentiates 1 - cos(theta) and theta - sin(theta) as written and loses up to 8e-5 of a gradient's norm at theta ~ 1e-4.
// Templated on the scalar so that a host program can run the same text in double.
#pragma once

#include <cmath>

#ifndef RB_HD
#ifdef __HIPCC__
#define RB_HD __host__ __device__ __forceinline__
#else
#define RB_HD inline
#endif
#endif

namespace evd {

#define RB_SERIES_BELOW 1.0

RB_HD float rb_sin(float x) { return sinf(x); }
RB_HD double rb_sin(double x) { return sin(x); }
RB_HD float rb_sqrt(float x) { return sqrtf(x); }
RB_HD double rb_sqrt(double x) { return sqrt(x); }

template <typename T>
RB_HD void rb_cross(const T a[3], const T b[3], T o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename T>
RB_HD T rb_dot(const T a[3], const T b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

template <typename T>
struct RbCoef {
    T n, theta, A, B, C, D, E;
};

template <typename T>
RB_HD RbCoef<T> rb_coef(const T rho[3]) {
    RbCoef<T> c;
    c.n = rb_sqrt(rb_dot(rho, rho));
    c.theta = c.n + (T)1.0e-10;
    const T t = c.theta * c.theta;
    const T sh = rb_sin((T)0.5 * c.theta), st = rb_sin(c.theta);
    c.A = st / c.theta;
    c.B = (T)2 * sh * sh / t;
    if (c.theta < (T)RB_SERIES_BELOW) {
        c.C = (T)(1.0 / 6) + t * ((T)(-1.0 / 120) + t * ((T)(1.0 / 5040) + t * ((T)(-1.0 / 362880) + t * ((T)(1.0 / 39916800) + t * (T)(-1.0 / 6227020800.0)))));
        c.D = (T)(1.0 / 24) + t * ((T)(-1.0 / 720) + t * ((T)(1.0 / 40320) + t * ((T)(-1.0 / 3628800) + t * ((T)(1.0 / 479001600) + t * (T)(-1.0 / 87178291200.0)))));
        c.E = (T)(1.0 / 120) + t * ((T)(-1.0 / 5040) + t * ((T)(1.0 / 362880) + t * ((T)(-1.0 / 39916800) + t * ((T)(1.0 / 6227020800.0) + t * (T)(-1.0 / 1307674368000.0)))));
    } else {
        c.C = (c.theta - st) / (t * c.theta);
        c.D = ((T)0.5 - c.B) / t;
        c.E = ((T)(1.0 / 6) - c.C) / t;
    }
    return c;
}

// origin' = R o + p, direction' = R d (the reference's R (o + d) + p - (R o + p))
template <typename T>
RB_HD void rb_warp(const T rho[3], const T tau[3], const T o[3], const T d[3], T yo[3], T yd[3]) {
    const RbCoef<T> c = rb_coef(rho);
    T c1[3], c2[3], s1[3], s2[3], e1[3], e2[3];
    rb_cross(rho, o, c1);
    rb_cross(rho, c1, c2);
    rb_cross(rho, tau, s1);
    rb_cross(rho, s1, s2);
    rb_cross(rho, d, e1);
    rb_cross(rho, e1, e2);
    for (int k = 0; k < 3; ++k) {
        yo[k] = (o[k] + tau[k]) + (c.A * c1[k] + c.B * (c2[k] + s1[k]) + c.C * s2[k]);
        yd[k] = d[k] + (c.A * e1[k] + c.B * e2[k]);
    }
}

// cotangents go (of origin') and gd (of direction') -> d rho, d tau, d o, d d
template <typename T>
RB_HD void rb_warp_bwd(const T rho[3], const T tau[3], const T o[3], const T d[3], const T go[3], const T gd[3], T drho[3], T dtau[3],
                       T d_o[3], T d_d[3]) {
    const RbCoef<T> c = rb_coef(rho);
    T c1[3], c2[3], s1[3], s2[3], e1[3], e2[3], q[3], q2[3], qd[3], qd2[3], u[3], w[3];
    rb_cross(rho, o, c1);
    rb_cross(rho, c1, c2);
    rb_cross(rho, tau, s1);
    rb_cross(rho, s1, s2);
    rb_cross(rho, d, e1);
    rb_cross(rho, e1, e2);
    rb_cross(go, rho, q);
    rb_cross(q, rho, q2);
    rb_cross(gd, rho, qd);
    rb_cross(qd, rho, qd2);
    T accA[3], accB[3], accC[3];
    // d/d rho at fixed A, B, C
    rb_cross(o, go, accA);
    rb_cross(d, gd, u);
    for (int k = 0; k < 3; ++k) accA[k] += u[k];
    rb_cross(c1, go, accB);
    rb_cross(o, q, u);
    for (int k = 0; k < 3; ++k) accB[k] += u[k];
    rb_cross(e1, gd, u);
    rb_cross(d, qd, w);
    for (int k = 0; k < 3; ++k) accB[k] += u[k] + w[k];
    rb_cross(tau, go, u);
    for (int k = 0; k < 3; ++k) accB[k] += u[k];
    rb_cross(s1, go, accC);
    rb_cross(tau, q, u);
    for (int k = 0; k < 3; ++k) accC[k] += u[k];
    const T dA = rb_dot(c1, go) + rb_dot(e1, gd);
    const T dB = rb_dot(c2, go) + rb_dot(e2, gd) + rb_dot(s1, go);
    const T dC = rb_dot(s2, go);
    const T dtheta = c.theta * ((c.C - c.B) * dA + ((T)2 * c.D - c.C) * dB + ((T)3 * c.E - c.D) * dC);
    const T dn = c.n > (T)0 ? dtheta / c.n : (T)0;          // d |rho| / d rho = rho / |rho|, zero at rho = 0 as torch's norm
    for (int k = 0; k < 3; ++k) {
        drho[k] = (c.A * accA[k] + c.B * accB[k] + c.C * accC[k]) + dn * rho[k];
        dtau[k] = go[k] + (c.B * q[k] + c.C * q2[k]);
        d_o[k] = go[k] + (c.A * q[k] + c.B * q2[k]);
        d_d[k] = gd[k] + (c.A * qd[k] + c.B * qd2[k]);
    }
}

}  // namespace evd
