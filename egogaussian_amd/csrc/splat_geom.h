// splat_geom.h -- the per-Gaussian geometry, written once: the row-vector transforms, quaternion -> rotation, the raw-parameter
// activation, the covariance chain  L0 = R(q) diag(mod s),  [L = M L0],  Sigma = L L^T  forward and backward, and the EWA projection.
// Callers: preprocess.hip (preprocess_one, pp_bwd_one, k_mark_visible) and cov3d.hip (k_cov3d_forward, k_cov3d_backward) -- the stand-alone
// covariance producer and the object rotation inside the rasterizer are this one text, so the covariance (hence radii, rectangles, sort
// order) and its gradients cannot drift apart between them.  The host compiler reads the header too (tests/splat_geom_host.cpp): no HIP types,
// nothing is loaded or stored but the caller's arrays.
// The translation units are compiled with -ffp-contract=off and every expression keeps the order of oracle/raster_oracle.c.
//   build_rotation / build_scaling_rotation / strip_symmetric     /root/reference/utils/general_utils.py:110-156
//   covariance activation and its object-rotated variant          /root/reference/scene/gaussian_model.py:29-33,46-63
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGS_GEOM_HD __host__ __device__ inline __attribute__((always_inline))
#define EGS_GEOM_UNROLL _Pragma("unroll")
#else
#define EGS_GEOM_HD inline
#define EGS_GEOM_UNROLL
#endif

// Row-vector convention: the reference stores matrices transposed (scene/cameras.py:67-69), out_j = sum_i p_i m[4 i + j] + m[12 + j].
EGS_GEOM_HD void xform43(const float* p, const float* m, float* o) {
    o[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    o[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    o[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
}
EGS_GEOM_HD void xform44(const float* p, const float* m, float* o) {
    o[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    o[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    o[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
    o[3] = m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15];
}

EGS_GEOM_HD void quat_to_rot(const float* q, float* R) {                 // quaternion (w, x, y, z) used as given
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - r * z); R[2] = 2.f * (x * z + r * y);
    R[3] = 2.f * (x * y + r * z); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - r * x);
    R[6] = 2.f * (x * z - r * y); R[7] = 2.f * (y * z + r * x); R[8] = 1.f - 2.f * (x * x + y * y);
}

EGS_GEOM_HD void mat3_mul(const float* A, const float* B, float* C) {    // C = A B
    EGS_GEOM_UNROLL
    for (int i = 0; i < 3; i++)
        EGS_GEOM_UNROLL
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Raw parameters: the model's activations -- exp on the scales, normalisation of the quaternion
// (/root/reference/scene/gaussian_model.py:36-44) -- applied in place of separate PyTorch launches.  `qinv` returns 1/|q_raw| for the
// backward (1 when the quaternion is used as given).
EGS_GEOM_HD void activate_scale_rot(bool log_scales, bool raw_quats, float* s, float* q, float& qinv) {
    if (log_scales) { s[0] = expf(s[0]); s[1] = expf(s[1]); s[2] = expf(s[2]); }
    qinv = 1.f;
    if (raw_quats) {
        qinv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        q[0] *= qinv; q[1] *= qinv; q[2] *= qinv; q[3] *= qinv;
    }
}

// The covariance factor of activated scales s and quaternion q: L0 = R diag(mod s), and L = M L0 for a `rotated` row (M: the object
// rotation, nine floats, row-major; not read otherwise), L = L0 for any other.  Everything the backward needs again is kept.
struct CovFactor { float R[9], sc[3], L0[9], L[9]; };
EGS_GEOM_HD void cov_factor(const float* s, float mod, const float* q, bool rotated, const float* M, CovFactor& f) {
    quat_to_rot(q, f.R);
    f.sc[0] = mod * s[0]; f.sc[1] = mod * s[1]; f.sc[2] = mod * s[2];
    EGS_GEOM_UNROLL
    for (int i = 0; i < 3; i++)
        EGS_GEOM_UNROLL
        for (int k = 0; k < 3; k++) f.L0[3 * i + k] = f.R[3 * i + k] * f.sc[k];
    if (rotated) mat3_mul(M, f.L0, f.L);
    else {
        EGS_GEOM_UNROLL
        for (int k = 0; k < 9; k++) f.L[k] = f.L0[k];
    }
}
// Sigma = L L^T, six unique entries (00,01,02,11,12,22)
EGS_GEOM_HD void cov_from_factor(const float* L, float* c6) {
    c6[0] = L[0] * L[0] + L[1] * L[1] + L[2] * L[2];
    c6[1] = L[0] * L[3] + L[1] * L[4] + L[2] * L[5];
    c6[2] = L[0] * L[6] + L[1] * L[7] + L[2] * L[8];
    c6[3] = L[3] * L[3] + L[4] * L[4] + L[5] * L[5];
    c6[4] = L[3] * L[6] + L[4] * L[7] + L[5] * L[8];
    c6[5] = L[6] * L[6] + L[7] * L[7] + L[8] * L[8];
}

// The chain backwards, from the six gradients g6 of Sigma (off-diagonal slots: the sum of both symmetric entries) to the parameters:
//   gL  = 2 mult Gs L     (mult: the caller's row-0 multiplier, the reference's duplicated-index gradient -- covariance.py)
//   dM  = gL L0^T         (a rotated row's nine terms of dL/dM, formed only when want_dM; zero otherwise)
//   gL0 = M^T gL          (gL itself for a row that is not rotated)
//   dscale: d/d scale, times the scale when log_scales (d/d log-scale = d/d scale * scale; s holds the ACTIVATED scales)
//   gq: d/d quaternion, taken back through q = q_raw / |q_raw| when raw_quats (q holds the ACTIVATED quaternion, qinv = 1/|q_raw|)
// f, s, mod, q, qinv, rotated, M: what the forward was given and made.  The caller decides what of this it stores and where.
struct CovGrad { float gL[9], dM[9], gL0[9], dscale[3], gq[4]; };
EGS_GEOM_HD void cov_factor_backward(const CovFactor& f, const float* s, float mod, const float* q, float qinv, bool rotated, const float* M,
                                     const float* g6, float mult, bool want_dM, bool log_scales, bool raw_quats, CovGrad& o) {
    const float Gs[9] = { g6[0], 0.5f * g6[1], 0.5f * g6[2], 0.5f * g6[1], g6[3], 0.5f * g6[4], 0.5f * g6[2], 0.5f * g6[4], g6[5] };
    EGS_GEOM_UNROLL
    for (int a = 0; a < 3; a++)
        EGS_GEOM_UNROLL
        for (int k = 0; k < 3; k++)
            o.gL[3 * a + k] = (Gs[3 * a] * f.L[k] + Gs[3 * a + 1] * f.L[3 + k] + Gs[3 * a + 2] * f.L[6 + k]) * (2.f * mult);
    EGS_GEOM_UNROLL
    for (int k = 0; k < 9; k++) { o.dM[k] = 0.f; o.gL0[k] = o.gL[k]; }
    if (rotated) {
        EGS_GEOM_UNROLL
        for (int a = 0; a < 3; a++)
            EGS_GEOM_UNROLL
            for (int b = 0; b < 3; b++) {
                if (want_dM) o.dM[3 * a + b] = o.gL[3 * a] * f.L0[3 * b] + o.gL[3 * a + 1] * f.L0[3 * b + 1] + o.gL[3 * a + 2] * f.L0[3 * b + 2];
                o.gL0[3 * a + b] = M[a] * o.gL[b] + M[3 + a] * o.gL[3 + b] + M[6 + a] * o.gL[6 + b];
            }
    }
    float gR[9];
    EGS_GEOM_UNROLL
    for (int k = 0; k < 3; k++) {
        const float ds = mod * (o.gL0[k] * f.R[k] + o.gL0[3 + k] * f.R[3 + k] + o.gL0[6 + k] * f.R[6 + k]);
        o.dscale[k] = log_scales ? ds * s[k] : ds;
        EGS_GEOM_UNROLL
        for (int a = 0; a < 3; a++) gR[3 * a + k] = o.gL0[3 * a + k] * f.sc[k];
    }
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    o.gq[0] = 2.f * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
    o.gq[1] = 2.f * (y * gR[1] + z * gR[2] + y * gR[3] - 2.f * x * gR[4] - r * gR[5] + z * gR[6] + r * gR[7] - 2.f * x * gR[8]);
    o.gq[2] = 2.f * (-2.f * y * gR[0] + x * gR[1] + r * gR[2] + x * gR[3] + z * gR[5] - r * gR[6] + z * gR[7] - 2.f * y * gR[8]);
    o.gq[3] = 2.f * (-2.f * z * gR[0] - r * gR[1] + x * gR[2] + r * gR[3] - 2.f * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7]);
    if (raw_quats) {                                                     // back through q = q_raw / |q_raw|
        const float dot = q[0] * o.gq[0] + q[1] * o.gq[1] + q[2] * o.gq[2] + q[3] * o.gq[3];
        EGS_GEOM_UNROLL
        for (int k = 0; k < 4; k++) o.gq[k] = (o.gq[k] - q[k] * dot) * qinv;
    }
}

// EWA projection: cov2D = (J R) Sigma (J R)^T, J the perspective Jacobian at the clamped camera-space point, R the rotation part of the
// world->view matrix V.  Everything the forward and backward share: camera-space point, clamped Jacobian rows (J R), Sigma*m, cov2D (a, b, c).
struct Ewa {
    float t[3], tx, ty, txtz, tytz, limx, limy, fx, fy;
    float m0[3], m1[3], S0[3], S1[3], a, b, c;
};
EGS_GEOM_HD void ewa_project(const float* p, const float* c6, const float* V, int W, int H, float tanfovx, float tanfovy, Ewa& e) {
    xform43(p, V, e.t);
    e.fx = (float)W / (2.f * tanfovx); e.fy = (float)H / (2.f * tanfovy);
    e.limx = 1.3f * tanfovx; e.limy = 1.3f * tanfovy;
    e.txtz = e.t[0] / e.t[2]; e.tytz = e.t[1] / e.t[2];
    e.tx = fminf(e.limx, fmaxf(-e.limx, e.txtz)) * e.t[2];
    e.ty = fminf(e.limy, fmaxf(-e.limy, e.tytz)) * e.t[2];
    float j00 = e.fx / e.t[2], j02 = -(e.fx * e.tx) / (e.t[2] * e.t[2]);
    float j11 = e.fy / e.t[2], j12 = -(e.fy * e.ty) / (e.t[2] * e.t[2]);
    EGS_GEOM_UNROLL
    for (int k = 0; k < 3; k++) {
        e.m0[k] = j00 * V[4 * k + 0] + j02 * V[4 * k + 2];
        e.m1[k] = j11 * V[4 * k + 1] + j12 * V[4 * k + 2];
    }
    e.S0[0] = c6[0] * e.m0[0] + c6[1] * e.m0[1] + c6[2] * e.m0[2];
    e.S0[1] = c6[1] * e.m0[0] + c6[3] * e.m0[1] + c6[4] * e.m0[2];
    e.S0[2] = c6[2] * e.m0[0] + c6[4] * e.m0[1] + c6[5] * e.m0[2];
    e.S1[0] = c6[0] * e.m1[0] + c6[1] * e.m1[1] + c6[2] * e.m1[2];
    e.S1[1] = c6[1] * e.m1[0] + c6[3] * e.m1[1] + c6[4] * e.m1[2];
    e.S1[2] = c6[2] * e.m1[0] + c6[4] * e.m1[1] + c6[5] * e.m1[2];
    e.a = e.m0[0] * e.S0[0] + e.m0[1] * e.S0[1] + e.m0[2] * e.S0[2] + 0.3f;
    e.b = e.m0[0] * e.S1[0] + e.m0[1] * e.S1[1] + e.m0[2] * e.S1[2];
    e.c = e.m1[0] * e.S1[0] + e.m1[1] * e.S1[1] + e.m1[2] * e.S1[2] + 0.3f;
}
