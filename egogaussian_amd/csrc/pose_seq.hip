// pose_seq.hip -- the object pose sequence on the device (include/egs_raster.h egs_pose_sequence):
//   egs_pose_head        the frame's pose in the rasterizer's form, A12 = [A | b] and M9, from the table and the trainable pose
//   egs_pose_tail        dL/dA12, dL/dM9 -> dL/dpose, the pose's Adam step, the frame's table row, the accumulated rows from it on
//   egs_pose_accumulate  the accumulated rows from scratch
//   egs_pose_interpolate stage 4: the rows of the held-out dynamic frames, one wave per gap (its own section below)
// Replaces what the object stages do on the host around every dynamic iteration (/root/reference/trainers/fine_obj.py:97-126,216-224: the
// `.data` reload, get_obj_trans_rot, get_accum_T_seq / get_accum_R_seq over all keys) and the dozen tiny torch launches each way of
// motion.ObjectMotion.compose() inside a captured step.  egogaussian_amd/poses.py holds the torch statement of every formula here.
//
// Mapping.  Each launch is ONE wave.  The work is a few hundred flops on at most K x 12 floats: every lane evaluates the same expressions
// on the same values (uniform loads, no LDS, no barrier) and lane 0 stores; the only cross-lane traffic is the accumulation's row fetch
// (accumulate_from) and the four Adam coefficients.  The arithmetic is float64 -- a wave issues the 36 multiply-adds of a 3x4 product in
// well under a microsecond -- and each stored float is rounded once.
// Accumulation order: a sequential chain over the rows.  The carry of row j is the float32 row j - 1 AS STORED, so a chain started at any
// row continues bit for bit what a full accumulation gives (the tail's suffix == egs_pose_accumulate on the rows both write).
// Rows outside [0, K) in the frame word mean "none": nothing outside the table is addressed whatever the word holds.
#include "egs_common.h"
#include <math.h>

namespace {

struct PoseSeq {
    int K;
    float* rel; uint8_t* valid; float* accum; float* pose; float* m; float* v; float* step; const float* lr;
    float b1, b2, eps;
};

struct Affine { double a[12]; };          // row-major 3x4 [A | b]

__device__ __forceinline__ Affine affine_identity() {
    Affine r;
#pragma unroll
    for (int k = 0; k < 12; k++) r.a[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
    return r;
}

__device__ __forceinline__ Affine affine_load(const float* __restrict__ p) {
    Affine r;
#pragma unroll
    for (int k = 0; k < 12; k++) r.a[k] = (double)p[k];
    return r;
}

// the row as it is stored: every entry rounded to float32
__device__ __forceinline__ Affine affine_round(const Affine& x) {
    Affine r;
#pragma unroll
    for (int k = 0; k < 12; k++) r.a[k] = (double)(float)x.a[k];
    return r;
}

__device__ __forceinline__ void affine_store(float* __restrict__ p, const Affine& x) {
#pragma unroll
    for (int k = 0; k < 12; k++) p[k] = (float)x.a[k];
}

// T o C: the pose T applied after C -- [R_T A_C | R_T b_C + t_T]
__device__ __forceinline__ Affine affine_mul(const Affine& T, const Affine& C) {
    Affine r;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = T.a[4 * i] * C.a[j];
            s = fma(T.a[4 * i + 1], C.a[4 + j], s);
            s = fma(T.a[4 * i + 2], C.a[8 + j], s);
            r.a[4 * i + j] = j == 3 ? s + T.a[4 * i + 3] : s;
        }
    return r;
}

// The 6-D map (utils/geometry_utils.py:69-89): r6 = (3,2) row-major, a1 / a2 its columns; R's columns are b1, b2, b3.
struct Rot6 { double a1[3], a2[3], b1[3], b2[3], u[3], n1, n2, d; };
#define POSE_NORM_FLOOR 1e-12

__device__ __forceinline__ double dot3(const double* a, const double* b) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// s.a1, s.a2 given: the rest of s, and R
__device__ __forceinline__ void rot6_from(Rot6& s, double* R /*[9] row-major*/) {
    s.n1 = fmax(sqrt(dot3(s.a1, s.a1)), POSE_NORM_FLOOR);
#pragma unroll
    for (int i = 0; i < 3; i++) s.b1[i] = s.a1[i] / s.n1;
    s.d = dot3(s.b1, s.a2);
#pragma unroll
    for (int i = 0; i < 3; i++) s.u[i] = s.a2[i] - s.d * s.b1[i];
    s.n2 = fmax(sqrt(dot3(s.u, s.u)), POSE_NORM_FLOOR);
#pragma unroll
    for (int i = 0; i < 3; i++) s.b2[i] = s.u[i] / s.n2;
    double b3[3];
    cross3(s.b1, s.b2, b3);
#pragma unroll
    for (int i = 0; i < 3; i++) { R[3 * i] = s.b1[i]; R[3 * i + 1] = s.b2[i]; R[3 * i + 2] = b3[i]; }
}

__device__ __forceinline__ void rot6_forward(const float* r6, Rot6& s, double* R /*[9] row-major*/) {
#pragma unroll
    for (int i = 0; i < 3; i++) { s.a1[i] = (double)r6[2 * i]; s.a2[i] = (double)r6[2 * i + 1]; }
    rot6_from(s, R);
}

// y = x / max(|x|, floor) backwards: through the norm only while it is above the floor (torch's clamp_min)
__device__ __forceinline__ void normalize_backward(const double* y, double n, const double* gy, double* gx) {
    const double c = n > POSE_NORM_FLOOR ? dot3(y, gy) : 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) gx[i] = (gy[i] - y[i] * c) / n;
}

// G = dL/dR [9] row-major -> dL/dr6 [6] in r6's layout
__device__ __forceinline__ void rot6_backward(const Rot6& s, const double* G, double* g6) {
    double g1[3], g2[3], g3[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { g1[i] = G[3 * i]; g2[i] = G[3 * i + 1]; g3[i] = G[3 * i + 2]; }
    cross3(s.b2, g3, t);                                            // b3 = b1 x b2:  dL/db1 += b2 x g3,  dL/db2 += g3 x b1
#pragma unroll
    for (int i = 0; i < 3; i++) g1[i] += t[i];
    cross3(g3, s.b1, t);
#pragma unroll
    for (int i = 0; i < 3; i++) g2[i] += t[i];
    double gu[3], ga1[3], ga2[3];
    normalize_backward(s.b2, s.n2, g2, gu);                         // b2 = normalize(u)
    const double gd = -dot3(gu, s.b1);                              // u = a2 - d b1
#pragma unroll
    for (int i = 0; i < 3; i++) { ga2[i] = gu[i] + gd * s.b1[i]; g1[i] += gd * s.a2[i] - s.d * gu[i]; }      // d = b1 . a2
    normalize_backward(s.b1, s.n1, g1, ga1);                        // b1 = normalize(a1)
#pragma unroll
    for (int i = 0; i < 3; i++) { g6[2 * i] = ga1[i]; g6[2 * i + 1] = ga2[i]; }
}

struct FrameWord { int fixed_row, train_row, reload; };
__device__ __forceinline__ FrameWord frame_word(const int32_t* __restrict__ w, int K) {
    FrameWord f = { w[0], w[1], w[2] };
    if (f.fixed_row < 0 || f.fixed_row >= K) f.fixed_row = -1;
    if (f.train_row < 0 || f.train_row >= K) f.train_row = -1;
    return f;
}

// accum[j] for j in [j0, K): carry = the stored row j0 - 1 (identity for j0 == 0); `first` (may be NULL): row j0's relative pose in
// registers, already rounded, valid -- the row the tail has just written
// Memory: the rows are fetched 64 at a time, lane l the row base + l (one round trip per 64 rows instead of two per row: a chain that
// loads each row as it reaches it spends 0.45 us per row on load latency alone, 136 us at K = 300); the chain then reads row i's twelve
// floats out of lane i (a uniform lane select).
// Arithmetic: the four columns of the carry are independent of each other -- column c of T o C needs column c of C only -- so lane l
// carries column l & 3 (three doubles) and computes 9 of the 36 multiply-adds; lanes 0 .. 3 store their column of every row.  One wave's
// float64 issue rate is what bounds the chain: with every lane carrying all twelve entries a row cost 0.27 us.  The operations per entry
// are those of affine_mul in its order: same bits.
__device__ __forceinline__ void accumulate_from(const PoseSeq& q, int j0, const Affine* first, bool lane0) {
    const int lane = (int)threadIdx.x, c = lane & 3;
    double cc[3];                                                    // column c of the carry
#pragma unroll
    for (int m = 0; m < 3; m++) cc[m] = j0 > 0 ? (double)q.accum[12 * (size_t)(j0 - 1) + 4 * m + c] : (m == c ? 1.0 : 0.0);
#pragma unroll 1
    for (int base = j0; base < q.K; base += EGS_WAVE) {
        const int mine = base + lane, n = min(EGS_WAVE, q.K - base);
        float r[12];
        int ok = 0;
#pragma unroll
        for (int k = 0; k < 12; k++) r[k] = 0.f;
        if (mine < q.K) {
            ok = q.valid[mine] != 0;
#pragma unroll
            for (int k = 0; k < 12; k++) r[k] = q.rel[12 * (size_t)mine + k];
        }
        if (first && base == j0 && lane == 0) {                      // (already rounded: the conversion is exact)
            ok = 1;
#pragma unroll
            for (int k = 0; k < 12; k++) r[k] = (float)first->a[k];
        }
#pragma unroll 1
        for (int i = 0; i < n; i++) {                                // i is uniform: the lane selects are scalar reads
            if (__builtin_amdgcn_readlane(ok, i)) {
                double T[12], nc[3];
#pragma unroll
                for (int k = 0; k < 12; k++) T[k] = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(r[k]), i));
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    double s = T[4 * m] * cc[0];
                    s = fma(T[4 * m + 1], cc[1], s);
                    s = fma(T[4 * m + 2], cc[2], s);
                    nc[m] = (double)(float)(c == 3 ? s + T[4 * m + 3] : s);      // the row as stored: rounded to float32
                }
#pragma unroll
                for (int m = 0; m < 3; m++) cc[m] = nc[m];
            }
            if (lane < 4) {
#pragma unroll
                for (int m = 0; m < 3; m++) q.accum[12 * (size_t)(base + i) + 4 * m + c] = (float)cc[m];
            }
        }
    }
}

__global__ __launch_bounds__(EGS_WAVE) void k_pose_head(PoseSeq q, const int32_t* __restrict__ word, float* __restrict__ A12, float* __restrict__ M9) {
    const bool lane0 = threadIdx.x == 0;
    const FrameWord f = frame_word(word, q.K);
    if (f.train_row < 0) {                                          // a fixed pose: bit copies, no product with a unit R_t
        float a[12];
#pragma unroll
        for (int k = 0; k < 12; k++) a[k] = f.fixed_row >= 0 ? q.accum[12 * (size_t)f.fixed_row + k] : ((k == 0 || k == 5 || k == 10) ? 1.f : 0.f);
        if (lane0) {
#pragma unroll
            for (int k = 0; k < 12; k++) A12[k] = a[k];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) M9[3 * i + j] = a[4 * i + j];
        }
        return;
    }
    float p[9];
    if (f.reload) {                                                 // fine_obj.py:118-119: the frame's stored pose becomes the parameters
        const float* __restrict__ row = q.rel + 12 * (size_t)f.train_row;
#pragma unroll
        for (int i = 0; i < 3; i++) { p[i] = row[4 * i + 3]; p[3 + 2 * i] = row[4 * i]; p[4 + 2 * i] = row[4 * i + 1]; }
        if (lane0) {
#pragma unroll
            for (int k = 0; k < 9; k++) q.pose[k] = p[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) p[k] = q.pose[k];
    }
    Rot6 s; Affine T;
    double R[9];
    rot6_forward(p + 3, s, R);
#pragma unroll
    for (int i = 0; i < 3; i++) { T.a[4 * i] = R[3 * i]; T.a[4 * i + 1] = R[3 * i + 1]; T.a[4 * i + 2] = R[3 * i + 2]; T.a[4 * i + 3] = (double)p[i]; }
    const Affine F = f.fixed_row >= 0 ? affine_load(q.accum + 12 * (size_t)f.fixed_row) : affine_identity();
    const Affine C = affine_mul(T, F);
    if (lane0) {
        affine_store(A12, C);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) M9[3 * i + j] = (float)C.a[4 * i + j];       // M = R_t R_f: the rotation block of the product
    }
}

__global__ __launch_bounds__(EGS_WAVE) void k_pose_tail(PoseSeq q, const int32_t* __restrict__ word, const float* __restrict__ grad21,
                                                        float* __restrict__ dpose, const uint32_t* __restrict__ skip) {
    if (skip && *skip) return;                                      // the frame behind these gradients overflowed: no step at all
    const bool lane0 = threadIdx.x == 0;
    const unsigned lane = threadIdx.x;
    const FrameWord f = frame_word(word, q.K);
    if (f.train_row < 0) return;                                    // a fixed-pose frame: torch's Adam skips a parameter without a gradient
    float p[9], m[9], v[9], g[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { p[k] = q.pose[k]; m[k] = q.m[k]; v[k] = q.v[k]; }
    Rot6 s;
    double R[9];
    rot6_forward(p + 3, s, R);
    const Affine F = f.fixed_row >= 0 ? affine_load(q.accum + 12 * (size_t)f.fixed_row) : affine_identity();
    double G[9];                                                    // dL/dR_t = dL/dA A_f^T + dL/db b_f^T + dL/dM R_f^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) t = fma((double)grad21[4 * i + k], F.a[4 * j + k], t);
            t = fma((double)grad21[4 * i + 3], F.a[4 * j + 3], t);
#pragma unroll
            for (int k = 0; k < 3; k++) t = fma((double)grad21[12 + 3 * i + k], F.a[4 * j + k], t);
            G[3 * i + j] = t;
        }
    double g6[6];
    rot6_backward(s, G, g6);
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = grad21[4 * i + 3];           // dL/dt = dL/db
#pragma unroll
    for (int k = 0; k < 6; k++) g[3 + k] = (float)g6[k];
    // the coefficients: lanes 0 .. 3 run the four double-precision pow() side by side -- the expressions of k_adam / egs_adam_tick
    const int grp = (lane >> 1) & 1, second = lane & 1;
    const double st = (double)q.step[grp] + 1.0;
    const double bc = 1.0 - pow((double)(second ? q.b2 : q.b1), st);
    const float coef = second ? (float)(1.0 / sqrt(bc)) : (float)((double)q.lr[grp] / bc);
    const float ss_t = __shfl(coef, 0), ib_t = __shfl(coef, 1), ss_r = __shfl(coef, 2), ib_r = __shfl(coef, 3);
    const float st_t = (float)((double)q.step[0] + 1.0), st_r = (float)((double)q.step[1] + 1.0);
#pragma unroll
    for (int k = 0; k < 9; k++) egs_adam1(p[k], g[k], m[k], v[k], q.b1, q.b2, q.eps, k < 3 ? ss_t : ss_r, k < 3 ? ib_t : ib_r);
    // the frame's table row: get_obj_trans_rot of the stepped pose
    Affine T;
    rot6_forward(p + 3, s, R);
#pragma unroll
    for (int i = 0; i < 3; i++) { T.a[4 * i] = R[3 * i]; T.a[4 * i + 1] = R[3 * i + 1]; T.a[4 * i + 2] = R[3 * i + 2]; T.a[4 * i + 3] = (double)p[i]; }
    T = affine_round(T);
    if (lane0) {
#pragma unroll
        for (int k = 0; k < 9; k++) { q.pose[k] = p[k]; q.m[k] = m[k]; q.v[k] = v[k]; if (dpose) dpose[k] = g[k]; }
        q.step[0] = st_t; q.step[1] = st_r;
        affine_store(q.rel + 12 * (size_t)f.train_row, T);
        q.valid[f.train_row] = 1;
    }
    accumulate_from(q, f.train_row, &T, lane0);
}

__global__ __launch_bounds__(EGS_WAVE) void k_pose_accumulate(PoseSeq q) { accumulate_from(q, 0, nullptr, threadIdx.x == 0); }

// ---- stage 4: the poses of the held-out frames inside the dynamic phases (/root/reference/trainers/interpolate_pose.py:28-63) --------------
// A gap is n consecutive rows of the NEW table that end at a key of the OLD one; all n receive the pose M whose n-th power the reference
// fits to the key's pose T by `iters` steps of plain gradient descent from the identity: loss = mean over the 16 entries of (M^n - T)^2,
// M = [R(r6) | t].  What the later stages consume is the END POINT of that descent (for a short gap and a small motion it has not
// converged), so the descent itself runs here: one wave per gap, the parameters in float64 registers from the first iteration to the
// last, no memory traffic inside the loop.
// The wave.  All factors are the same matrix, so dL/dM = sum over k = 1 .. n of (M^(k-1))^T G (M^(n-k))^T with G = dL/dM^n.  Lane k - 1
// forms term k from powers it builds itself: the running square M, M^2, M^4 .. is the same in every lane and each lane multiplies the
// squares its two exponents select (at most five each, n <= 32).  The bottom row of every factor is (0 0 0 1): only the top three rows
// of G reach the top three rows of a term, so a term is twelve numbers.  They are summed over the wave by an xor butterfly -- a + b
// and b + a are the same double, so every lane ends with the same twelve sums, in an order that depends on nothing but n -- and every
// lane takes the same step.  No LDS, no barrier.
// M^n itself is the product of the squares n's bits select, not the reference's left-to-right chain: in float64 the two differ in the
// sixteenth place.
#define POSE_GAP_MAX 32

// A <- A o S where bit `b` of e is set (per lane)
__device__ __forceinline__ void power_step(Affine& A, const Affine& S, int e, int b) {
    if ((e >> b) & 1) A = affine_mul(A, S);
}

// M^a, M^b per lane and M^n (n uniform) from one run of squarings; exponents in [0, 32]
__device__ __forceinline__ void affine_powers(const Affine& M, int a, int b, int n, Affine& A, Affine& B, Affine& P) {
    Affine S = M;
    A = affine_identity(); B = affine_identity(); P = affine_identity();
#pragma unroll
    for (int bit = 0; bit < 6; bit++) {
        if (bit < 5) { power_step(A, S, a, bit); power_step(B, S, b, bit); }
        power_step(P, S, n, bit);
        if (bit < 5) S = affine_mul(S, S);
    }
}

__device__ __forceinline__ Affine affine_from(const double* R, const double* t) {
    Affine M;
#pragma unroll
    for (int i = 0; i < 3; i++) { M.a[4 * i] = R[3 * i]; M.a[4 * i + 1] = R[3 * i + 1]; M.a[4 * i + 2] = R[3 * i + 2]; M.a[4 * i + 3] = t[i]; }
    return M;
}

__device__ __forceinline__ double wave_sum_all(double v) {
#pragma unroll
    for (int m = 1; m < EGS_WAVE; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(EGS_WAVE) void k_pose_interpolate(const float* __restrict__ from_rel, int K_from, float* __restrict__ to_rel,
                                                               uint8_t* __restrict__ to_valid, int K_to, const int32_t* __restrict__ gaps, int G,
                                                               int iters, float lr_f, float* __restrict__ residual, int32_t* __restrict__ status) {
    const int lane = (int)threadIdx.x;
    // every wave reads ALL the words first: one bad gap and no wave writes anything
    int bad = 0;
    for (int g = lane; g < G; g += EGS_WAVE) {
        const int first = gaps[3 * (size_t)g], n = gaps[3 * (size_t)g + 1], old_row = gaps[3 * (size_t)g + 2];
        bad |= n < 2 || n > POSE_GAP_MAX || first < 0 || first > K_to - n || old_row < 0 || old_row >= K_from;
    }
    bad = __any(bad);
    if (blockIdx.x == 0 && lane == 0) *status = bad ? 1 : 0;
    if (bad) return;
    const int first = gaps[3 * (size_t)blockIdx.x], n = gaps[3 * (size_t)blockIdx.x + 1], old_row = gaps[3 * (size_t)blockIdx.x + 2];
    const Affine T = affine_load(from_rel + 12 * (size_t)old_row);
    const bool member = lane < n;                                   // lane l forms term k = l + 1: exponents l and n - 1 - l
    const int ea = member ? lane : 0, eb = member ? n - 1 - lane : 0;
    const double lr = (double)lr_f;
    double t[3] = { 0.0, 0.0, 0.0 }, R[9];
    Rot6 s;
#pragma unroll
    for (int i = 0; i < 3; i++) { s.a1[i] = i == 0 ? 1.0 : 0.0; s.a2[i] = i == 1 ? 1.0 : 0.0; }
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
        rot6_from(s, R);
        const Affine M = affine_from(R, t);
        Affine A, B, P;
        affine_powers(M, ea, eb, n, A, B, P);
        // G = dL/dP over the top three rows = 2 (P - T) / 16; the reference's early exit on the float32 product: isclose(rtol 1e-7, atol 1e-9)
        double Gm[12];
        bool met = true;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            Gm[k] = (P.a[k] - T.a[k]) * 0.125;
            met = met && fabs((double)(float)P.a[k] - T.a[k]) <= 1e-9 + 1e-7 * fabs(T.a[k]);
        }
        // the term: X = A_R^T G [3x4], Y = X B^T restricted to the top three rows -- columns 0 .. 2 dL/dR, column 3 dL/dt
        double X[12], Y[12];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int l = 0; l < 4; l++) X[4 * i + l] = fma(A.a[8 + i], Gm[8 + l], fma(A.a[4 + i], Gm[4 + l], A.a[i] * Gm[l]));
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++)
                Y[4 * i + j] = fma(X[4 * i + 3], B.a[4 * j + 3], fma(X[4 * i + 2], B.a[4 * j + 2], fma(X[4 * i + 1], B.a[4 * j + 1], X[4 * i] * B.a[4 * j])));
            Y[4 * i + 3] = X[4 * i + 3];
        }
#pragma unroll
        for (int k = 0; k < 12; k++) Y[k] = wave_sum_all(member ? Y[k] : 0.0);
        double GR[9], g6[6];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) GR[3 * i + j] = Y[4 * i + j];
        rot6_backward(s, GR, g6);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            t[i] = t[i] - lr * Y[4 * i + 3];
            s.a1[i] = s.a1[i] - lr * g6[2 * i];
            s.a2[i] = s.a2[i] - lr * g6[2 * i + 1];
        }
        if (met) break;                                             // (tested on the product before the step, left after it: the reference's order)
    }
    rot6_from(s, R);
    const Affine M = affine_from(R, t);
    Affine A, B, P;
    affine_powers(M, 0, 0, n, A, B, P);
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < 12; k++) { const double d = fabs(P.a[k] - T.a[k]); r = (d > r || d != d) ? d : r; }      // (a NaN stays one)
    if (member) {
        affine_store(to_rel + 12 * (size_t)(first + lane), M);
        to_valid[first + lane] = 1;
    }
    if (lane == 0) residual[blockIdx.x] = (float)r;
}

bool pose_seq_args(const egs_pose_sequence* s, PoseSeq& q) {
    if (!s || s->K < 1 || !s->rel || !s->valid || !s->accum || !s->pose || !s->exp_avg || !s->exp_avg_sq || !s->step || !s->lr) return false;
    q.K = s->K; q.rel = s->rel; q.valid = s->valid; q.accum = s->accum; q.pose = s->pose; q.m = s->exp_avg; q.v = s->exp_avg_sq;
    q.step = s->step; q.lr = s->lr; q.b1 = s->beta1; q.b2 = s->beta2; q.eps = s->eps;
    return true;
}

}  // namespace

extern "C" {

int egs_pose_head(const egs_pose_sequence* seq, const int32_t* frame_word, float* A12, float* M9, void* stream) {
    PoseSeq q;
    if (!pose_seq_args(seq, q) || !frame_word || !A12 || !M9) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_pose_head, dim3(1), dim3(EGS_WAVE), 0, (hipStream_t)stream, q, frame_word, A12, M9);
    return (int)hipGetLastError();
}

int egs_pose_tail(const egs_pose_sequence* seq, const int32_t* frame_word, const float* grad21, float* dpose, const uint32_t* skip_flag, void* stream) {
    PoseSeq q;
    if (!pose_seq_args(seq, q) || !frame_word || !grad21) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_pose_tail, dim3(1), dim3(EGS_WAVE), 0, (hipStream_t)stream, q, frame_word, grad21, dpose, skip_flag);
    return (int)hipGetLastError();
}

int egs_pose_accumulate(const egs_pose_sequence* seq, void* stream) {
    PoseSeq q;
    if (!pose_seq_args(seq, q)) return EGS_ERR_ARG;
    hipLaunchKernelGGL(k_pose_accumulate, dim3(1), dim3(EGS_WAVE), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

int egs_pose_interpolate(const egs_pose_sequence* from, const egs_pose_sequence* to, const int32_t* gaps, int n_gaps, int iters, float lr,
                         float* residual, int32_t* status, void* stream) {
    PoseSeq qf, qt;
    if (!pose_seq_args(from, qf) || !pose_seq_args(to, qt) || !gaps || !residual || !status || n_gaps < 1 || iters < 0) return EGS_ERR_ARG;
    if (n_gaps > 65535) return EGS_ERR_RANGE;
    hipLaunchKernelGGL(k_pose_interpolate, dim3(n_gaps), dim3(EGS_WAVE), 0, (hipStream_t)stream, (const float*)qf.rel, qf.K, qt.rel, qt.valid, qt.K,
                       gaps, n_gaps, iters, lr, residual, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    int32_t refused = 0;                                            // the words live on the device: the verdict on them is read back
    e = hipMemcpyAsync(&refused, status, sizeof(refused), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return refused ? EGS_ERR_RANGE : 0;
}

}  // extern "C"
