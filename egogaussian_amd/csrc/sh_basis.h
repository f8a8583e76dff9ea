// sh_basis.h -- the real spherical-harmonics basis of degree 0..3, written once: the constants, the colour of a view direction, and its
// derivatives with respect to the coefficients and to the direction.  Callers: the inline M = 1 path of preprocess.hip (preprocess_one,
// pp_bwd_one) and the wave-tiled kernels of sh.hip.  Coefficient rows are [k][channel], k = 0 .. (D + 1)^2 - 1 active of M stored.
// The translation units are compiled with -ffp-contract=off and every expression keeps the order of oracle/raster_oracle.c.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __constant__ float kC0 = 0.28209479177387814f;
__device__ __constant__ float kC1 = 0.4886025119029199f;
__device__ __constant__ float kC2[5] = { 1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                         -1.0925484305920792f, 0.5462742152960396f };
__device__ __constant__ float kC3[7] = { -0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                         0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                         -0.5900435899266435f };

// The unit view direction (x, y, z) of position p seen from campos, and inv = 1 / |p - campos|.
__device__ __forceinline__ void sh_view_dir(const float* p, const float* campos, float& x, float& y, float& z, float& inv) {
    const float d0[3] = { p[0] - campos[0], p[1] - campos[1], p[2] - campos[2] };
    inv = 1.f / sqrtf(d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2]);
    x = d0[0] * inv; y = d0[1] * inv; z = d0[2] * inv;
}

__device__ __forceinline__ float sh_channel(int deg, const float* sh, int ch, float x, float y, float z) {
#define SH(k) sh[(k) * 3 + ch]
    float v = kC0 * SH(0);
    if (deg > 0) {
        v = v - kC1 * y * SH(1) + kC1 * z * SH(2) - kC1 * x * SH(3);
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            v = v + kC2[0] * xy * SH(4) + kC2[1] * yz * SH(5) + kC2[2] * (2.f * zz - xx - yy) * SH(6) +
                kC2[3] * xz * SH(7) + kC2[4] * (xx - yy) * SH(8);
            if (deg > 2) {
                v = v + kC3[0] * y * (3.f * xx - yy) * SH(9) + kC3[1] * xy * z * SH(10) +
                    kC3[2] * y * (4.f * zz - xx - yy) * SH(11) + kC3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * SH(12) +
                    kC3[4] * x * (4.f * zz - xx - yy) * SH(13) + kC3[5] * z * (xx - yy) * SH(14) +
                    kC3[6] * x * (xx - 3.f * yy) * SH(15);
            }
        }
    }
#undef SH
    return v + 0.5f;
}

// The three channels of a row, clamped at 0 -> rgb; returns the clamp bits (bit ch: the channel was negative).
__device__ __forceinline__ uint32_t sh_colour(int deg, const float* sh, float x, float y, float z, float* rgb) {
    uint32_t cl = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float v = sh_channel(deg, sh, ch, x, y, z);
        if (v < 0.f) cl |= 1u << ch;
        rgb[ch] = fmaxf(v, 0.f);
    }
    return cl;
}

// One channel of the colour backward: g = dL/dcolour[ch] (zero where the forward clamped) -> gsh[k][ch] for the active coefficients, zeros
// for k = (D + 1)^2 .. M - 1, and gdir += dcolour/d(x, y, z) * g.  `gsh` may be the row `sh` itself (k_sh_backward forms the gradient in
// place in its LDS row): every read of the channel's coefficients comes before the first write.
__device__ __forceinline__ void sh_channel_backward(int D, int M, const float* sh, float* gsh, int ch, float x, float y, float z, float g,
                                                    float* gdir) {
#define SH(k) sh[(k) * 3 + ch]
#define GSH(k) gsh[(k) * 3 + ch]
    float dx_ = 0.f, dy_ = 0.f, dz_ = 0.f;
    if (D > 0) {
        dx_ = -kC1 * SH(3); dy_ = -kC1 * SH(1); dz_ = kC1 * SH(2);
        if (D > 1) {
            dx_ += kC2[0] * y * SH(4) + kC2[2] * 2.f * -x * SH(6) + kC2[3] * z * SH(7) + kC2[4] * 2.f * x * SH(8);
            dy_ += kC2[0] * x * SH(4) + kC2[1] * z * SH(5) + kC2[2] * 2.f * -y * SH(6) + kC2[4] * 2.f * -y * SH(8);
            dz_ += kC2[1] * y * SH(5) + kC2[2] * 4.f * z * SH(6) + kC2[3] * x * SH(7);
            if (D > 2) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                dx_ += kC3[0] * SH(9) * 6.f * xy + kC3[1] * SH(10) * yz + kC3[2] * SH(11) * -2.f * xy +
                       kC3[3] * SH(12) * -6.f * xz + kC3[4] * SH(13) * (-3.f * xx + 4.f * zz - yy) +
                       kC3[5] * SH(14) * 2.f * xz + kC3[6] * SH(15) * 3.f * (xx - yy);
                dy_ += kC3[0] * SH(9) * 3.f * (xx - yy) + kC3[1] * SH(10) * xz +
                       kC3[2] * SH(11) * (-3.f * yy + 4.f * zz - xx) + kC3[3] * SH(12) * -6.f * yz +
                       kC3[4] * SH(13) * -2.f * xy + kC3[5] * SH(14) * -2.f * yz + kC3[6] * SH(15) * -6.f * xy;
                dz_ += kC3[1] * SH(10) * xy + kC3[2] * SH(11) * 8.f * yz + kC3[3] * SH(12) * 3.f * (2.f * zz - xx - yy) +
                       kC3[4] * SH(13) * 8.f * xz + kC3[5] * SH(14) * (xx - yy);
            }
        }
    }
    gdir[0] += dx_ * g; gdir[1] += dy_ * g; gdir[2] += dz_ * g;
    GSH(0) = kC0 * g;
    if (D > 0) {
        GSH(1) = -kC1 * y * g; GSH(2) = kC1 * z * g; GSH(3) = -kC1 * x * g;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;   // (again: not held live across the reads)
            GSH(4) = kC2[0] * xy * g; GSH(5) = kC2[1] * yz * g; GSH(6) = kC2[2] * (2.f * zz - xx - yy) * g;
            GSH(7) = kC2[3] * xz * g; GSH(8) = kC2[4] * (xx - yy) * g;
            if (D > 2) {
                GSH(9) = kC3[0] * y * (3.f * xx - yy) * g; GSH(10) = kC3[1] * xy * z * g;
                GSH(11) = kC3[2] * y * (4.f * zz - xx - yy) * g;
                GSH(12) = kC3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * g;
                GSH(13) = kC3[4] * x * (4.f * zz - xx - yy) * g; GSH(14) = kC3[5] * z * (xx - yy) * g;
                GSH(15) = kC3[6] * x * (xx - 3.f * yy) * g;
            }
        }
    }
    for (int k = (D + 1) * (D + 1); k < M; k++) GSH(k) = 0.f;         // coefficients above the active degree
#undef SH
#undef GSH
}

// dL/d(unit direction) -> dL/dposition, added to gpos: the projection onto the tangent plane of the direction, times inv.
__device__ __forceinline__ void sh_dir_to_pos(float x, float y, float z, float inv, const float* gdir, float* gpos) {
    const float dot = x * gdir[0] + y * gdir[1] + z * gdir[2];
    gpos[0] += (gdir[0] - x * dot) * inv; gpos[1] += (gdir[1] - y * dot) * inv; gpos[2] += (gdir[2] - z * dot) * inv;
}

}  // namespace
