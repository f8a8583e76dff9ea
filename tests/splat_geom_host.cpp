// Host driver of egogaussian_amd/csrc/splat_geom.h for tests/test_splat_geom_cpu.py: the per-Gaussian geometry the kernels of preprocess.hip and
// cov3d.hip run on the device, compiled by the host compiler.  Arrays are raw float32 files; float arguments are given as their bit patterns.
//   splat_geom_host project IN OUT N W H TANFOVX TANFOVY MOD
//       IN: means [N,3], scales [N,3], quaternions [N,4], view matrix [16].  Scales and quaternions are used as given (no activation flag), the
//       way preprocess_one calls the header.  OUT: covariance [N,6], camera-space depth [N], cov2D (a, b, c) [N,3].
//   splat_geom_host chain IN OUT N LOG MOD MULT HAS_M HAS_SEL
//       IN: scaling [N,3], quaternions [N,4], dL/dcov [N,6], then M [9] if HAS_M, then the selection [N] (0 / 1 as float32) if HAS_SEL.
//       Forward and backward the way k_cov3d_forward / k_cov3d_backward call the header: always normalising and chaining through the
//       normalisation, LOG scales, row 0 of a rotated set multiplied by MULT.  OUT: covariance [N,6], dL/dscaling [N,3], dL/dquaternion [N,4],
//       each row's nine dL/dM terms [N,9] (the kernel sums them per workgroup; the test in float64).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#include "../egogaussian_amd/csrc/splat_geom.h"

static float from_bits(const char* s) { const uint32_t b = (uint32_t)strtoul(s, nullptr, 10); float f; memcpy(&f, &b, 4); return f; }

static bool read_floats(const char* path, std::vector<float>& x) {
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(x.data(), sizeof(float), x.size(), f) == x.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %zu floats from %s\n", x.size(), path);
    return ok;
}
static bool write_floats(const char* path, const std::vector<float>& x) {
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(x.data(), sizeof(float), x.size(), f) == x.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot write %s\n", path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc == 10 && !strcmp(argv[1], "project")) {
        const size_t n = (size_t)atol(argv[4]);
        const int W = atoi(argv[5]), H = atoi(argv[6]);
        const float tanfovx = from_bits(argv[7]), tanfovy = from_bits(argv[8]), mod = from_bits(argv[9]);
        std::vector<float> in(n * 10 + 16), out(n * 10);
        if (!read_floats(argv[2], in)) return 2;
        const float* means = in.data(); const float* scales = means + 3 * n; const float* rots = scales + 3 * n; const float* V = rots + 4 * n;
        for (size_t i = 0; i < n; i++) {
            float s[3] = { scales[3 * i], scales[3 * i + 1], scales[3 * i + 2] };
            float q[4] = { rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3] };
            float qinv; activate_scale_rot(false, false, s, q, qinv);
            CovFactor f; cov_factor(s, mod, q, false, nullptr, f);
            float* c6 = out.data() + 6 * i;
            cov_from_factor(f.L, c6);
            Ewa e; ewa_project(means + 3 * i, c6, V, W, H, tanfovx, tanfovy, e);
            out[6 * n + i] = e.t[2];
            out[7 * n + 3 * i] = e.a; out[7 * n + 3 * i + 1] = e.b; out[7 * n + 3 * i + 2] = e.c;
        }
        return write_floats(argv[3], out) ? 0 : 2;
    }
    if (argc == 10 && !strcmp(argv[1], "chain")) {
        const size_t n = (size_t)atol(argv[4]);
        const bool log_scaling = atoi(argv[5]) != 0, has_M = atoi(argv[8]) != 0, has_sel = atoi(argv[9]) != 0;
        const float mod = from_bits(argv[6]), row0_mult = from_bits(argv[7]);
        std::vector<float> in(n * 13 + (has_M ? 9 : 0) + (has_sel ? n : 0)), out(n * 22);
        if (!read_floats(argv[2], in)) return 2;
        const float* scaling = in.data(); const float* rotation = scaling + 3 * n; const float* dcov = rotation + 4 * n;
        const float* M = has_M ? dcov + 6 * n : nullptr;
        const float* sel = has_sel ? dcov + 6 * n + (has_M ? 9 : 0) : nullptr;
        for (size_t i = 0; i < n; i++) {
            float q[4] = { rotation[4 * i], rotation[4 * i + 1], rotation[4 * i + 2], rotation[4 * i + 3] };
            float s3[3] = { scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2] };
            float inv; activate_scale_rot(log_scaling, true, s3, q, inv);
            const bool moved = M && (!sel || sel[i] != 0.f);
            CovFactor f; cov_factor(s3, mod, q, moved, M, f);
            cov_from_factor(f.L, out.data() + 6 * i);
            const float mult = (moved && i == 0) ? row0_mult : 1.f;
            CovGrad g; cov_factor_backward(f, s3, mod, q, inv, moved, M, dcov + 6 * i, mult, true, log_scaling, true, g);
            for (int k = 0; k < 3; k++) out[6 * n + 3 * i + k] = g.dscale[k];
            for (int k = 0; k < 4; k++) out[9 * n + 4 * i + k] = g.gq[k];
            for (int k = 0; k < 9; k++) out[13 * n + 9 * i + k] = g.dM[k];
        }
        return write_floats(argv[3], out) ? 0 : 2;
    }
    fprintf(stderr, "usage: splat_geom_host project IN OUT N W H TANFOVX TANFOVY MOD | chain IN OUT N LOG MOD MULT HAS_M HAS_SEL\n");
    return 2;
}
