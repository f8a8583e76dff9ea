// lpips.hip -- LPIPS (VGG-16) of two 8-bit images (include/egs_raster.h egs_lpips_forward; egogaussian_amd/lpips.py lpips_vgg is the torch
// statement): the evaluation pass's third figure and its only dense contraction.  Activations are float32 NHWC, the two images a batch of 2,
// so a weight is read once for both and both pass through the same arithmetic in the same order (an identical pair gives exact zeros).
//
//   k_lpips_input     the two planar uint8 images (what egs_eval_metrics writes) and `keep` -> (kept ? byte / 255 : 0 - mean) / std, NHWC with
//                     the channels padded 3 -> 4 by zeros (the padded weights' fourth row is zero as well).
//   k_conv3x3_relu    3x3 convolution, stride 1, zero padding 1, bias, ReLU as an implicit GEMM on the matrix pipe: M = the 128 pixels of an
//                     8 x 16 tile, N = 64 output channels, K = 9 * Cin walked in chunks of KC input channels.  Per chunk the workgroup stages
//                     the tile with its one-pixel halo (10 x 18 pixels x KC channels, zeros outside the image) and the weight chunk
//                     [9][KC][64] in LDS; each of its four waves owns 32 pixels (two tile rows) x 64 channels = two 32x32 accumulators and
//                     issues v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: exact f32 products, no xf32 / bf16 rounding of the features);
//                     each chunk's sum is formed by itself and then added to the running total (blocked summation).
//                     Lane maps of that form (pinned by tests/test_gpu_lpips.py's single-layer cases): lane l holds A[m = l & 31][k = l >> 5]
//                     and B[k = l >> 5][n = l & 31]; accumulator register r of lane l is C[m = 8 (r >> 2) + 4 (l >> 5) + (r & 3)][n = l & 31].
//                     K runs tap-major, channel-minor (k = tap * Cin + c): the order of the packed weights [9 Cin, Cout].
//   k_lpips_tap       one wave per 2 x 2 quad of a tap's map, both images: per pixel the two channel norms, sum_c w[c] (x / (|x| + eps) -
//                     y / (|y| + eps))^2, added over the wave's pixels in float64; one float64 partial per workgroup (no float atomics); at
//                     the first four taps the quad's channel-wise maximum is the pooled map the next block reads (floor: a quad that hangs
//                     over the edge contributes to the tap and writes no pooled pixel).
//   k_lpips_finish    one wave: the partials of each tap in a fixed order in float64, / (H_k W_k), the five taps and their sum into
//                     rows[cursor[0]], cursor[0] + 1 -- egs_eval_metrics' cursor semantics.
// Every address is formed from the sizes passed in; pixels outside a map are masked (loads replaced by zeros, stores skipped), never read.
#include "egs_common.h"

#define LP_TH 8                   // tile rows
#define LP_TW 16                  // tile columns
#define LP_NT 64                  // output channels per workgroup
#define LP_HP ((LP_TH + 2) * (LP_TW + 2))       // pixels of a tile with its halo: 180
#define LP_EPS 1e-10f
#define LP_QUADS_PER_WAVE 8

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_lpips_input(int H, int W, const uint8_t* __restrict__ q_x, const uint8_t* __restrict__ q_y,
                                                     const float* __restrict__ keep, float* __restrict__ out /*[2,H,W,4]*/) {
    const size_t n = (size_t)H * (size_t)W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint8_t* __restrict__ q = blockIdx.y ? q_y : q_x;
    const bool kept = keep ? keep[p] >= 0.5f : true;
    const float mean[3] = {-.030f, -.088f, -.188f}, sd[3] = {.458f, .448f, .450f};
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float u = kept ? (float)q[(size_t)c * n + p] / 255.f : 0.f;          // true division: what the statement's byte / 255 is
        v[c] = (u - mean[c]) / sd[c];
    }
    reinterpret_cast<float4*>(out)[(size_t)blockIdx.y * n + p] = make_float4(v[0], v[1], v[2], 0.f);
}

// grid: (tiles_x * tiles_y, Cout / 64, n images); block: 256.  KC: input channels per chunk (Cin % KC == 0): 16, or 4 for the first layer.
template <int KC>
__global__ __launch_bounds__(256) void k_conv3x3_relu(int H, int W, int Cin, int Cout, int tiles_x, const float* __restrict__ in /*[n,H,W,Cin]*/,
                                                      const float* __restrict__ wk /*[9 Cin, Cout]*/, const float* __restrict__ bias,
                                                      float* __restrict__ out /*[n,H,W,Cout]*/) {
    constexpr int PS = KC + 1;                         // LDS pixel stride (odd: neighbouring pixels fall into different banks)
    __shared__ float s_in[LP_HP * PS];
    __shared__ __attribute__((aligned(16))) float s_w[9 * KC * LP_NT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * LP_TH, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * LP_TW;
    const int n0 = (int)blockIdx.y * LP_NT;
    const size_t img = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const int m = lane & 31, kh = lane >> 5;           // this lane's A row (pixel of the wave's 32) and k half
    const int py = wv * 2 + (m >> 4), px = m & 15;     // the pixel's place in the tile
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }

    for (int c0 = 0; c0 < Cin; c0 += KC) {
        // ---- stage: the haloed tile of channels c0 .. c0 + KC - 1 (zeros outside the image) and the weight chunk ----
        constexpr int V4 = KC / 4;                     // float4 per pixel
        for (int i = tid; i < LP_HP * V4; i += 256) {
            const int hp = i / V4, v4 = i - hp * V4;
            const int y = ty0 - 1 + hp / (LP_TW + 2), x = tx0 - 1 + hp % (LP_TW + 2);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < H && x >= 0 && x < W)
                v = *reinterpret_cast<const float4*>(in + (img + (size_t)y * W + x) * (size_t)Cin + c0 + v4 * 4);
            float* d = s_in + hp * PS + v4 * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        for (int i = tid; i < 9 * KC * (LP_NT / 4); i += 256) {
            const int row = i / (LP_NT / 4), v4 = i - row * (LP_NT / 4);          // row = tap * KC + c
            const int tap = row / KC, c = row - tap * KC;
            const float4 v = *reinterpret_cast<const float4*>(wk + ((size_t)tap * Cin + c0 + c) * (size_t)Cout + n0 + v4 * 4);
            *reinterpret_cast<float4*>(s_w + row * LP_NT + v4 * 4) = v;
        }
        __syncthreads();
        // ---- contract: 9 taps x KC / 2 steps of k = 2, into accumulators of this chunk alone.  Blocked summation: one chain over all of
        // K = 4608 carried 8 x the rounding error of a blocked float32 convolution (2.4e-6 against 2.9e-7 at 512 -> 512 channels); chunk
        // sums of 9 KC products added to a running total keep both chains short, for 32 additions per lane and chunk. ----
        f32x16 part0, part1;
#pragma unroll
        for (int r = 0; r < 16; r++) { part0[r] = 0.f; part1[r] = 0.f; }
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const float* a_p = s_in + ((py + tap / 3) * (LP_TW + 2) + px + tap % 3) * PS + kh;
            const float* b_p = s_w + (tap * KC + kh) * LP_NT + m;
#pragma unroll
            for (int c = 0; c < KC; c += 2) {
                const float a = a_p[c], b0 = b_p[c * LP_NT], b1 = b_p[c * LP_NT + 32];
                part0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, part0, 0, 0, 0);
                part1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, part1, 0, 0, 0);
            }
        }
        acc0 += part0; acc1 += part1;
        __syncthreads();
    }
    // ---- epilogue: bias, ReLU, NHWC store (lanes 0..31 of a register are 32 consecutive channels of one pixel) ----
    const float bs0 = bias[n0 + m], bs1 = bias[n0 + 32 + m];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int mm = 8 * (r >> 2) + 4 * kh + (r & 3);
        const int y = ty0 + wv * 2 + (mm >> 4), x = tx0 + (mm & 15);
        if (y < H && x < W) {
            float* o = out + (img + (size_t)y * W + x) * (size_t)Cout + n0 + m;
            o[0] = fmaxf(acc0[r] + bs0, 0.f);
            o[32] = fmaxf(acc1[r] + bs1, 0.f);
        }
    }
}

// grid: ceil(quads / (4 * LP_QUADS_PER_WAVE)); block: 256 (four waves, each LP_QUADS_PER_WAVE consecutive quads).  C % 64 == 0, C <= 512.
__global__ __launch_bounds__(256) void k_lpips_tap(int H, int W, int C, const float* __restrict__ f /*[2,H,W,C]*/, const float* __restrict__ lin /*[C]*/,
                                                   float* __restrict__ pooled /*[2,H/2,W/2,C] or NULL*/, double* __restrict__ partial) {
    __shared__ double s_part[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int J = C >> 6;
    const int qw = (W + 1) >> 1, qh = (H + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    const size_t nq = (size_t)qw * (size_t)qh, plane = (size_t)H * (size_t)W;
    float wl[8];
#pragma unroll
    for (int j = 0; j < 8; j++) wl[j] = j < J ? lin[j * 64 + lane] : 0.f;
    double sum = 0.0;
    const size_t q0 = ((size_t)blockIdx.x * 4 + wv) * LP_QUADS_PER_WAVE;
    for (int k = 0; k < LP_QUADS_PER_WAVE; k++) {
        const size_t q = q0 + k;
        if (q >= nq) break;                                                      // wave-uniform
        const int qy = (int)(q / (size_t)qw), qx = (int)(q % (size_t)qw);
        float mx[8], my[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { mx[j] = 0.f; my[j] = 0.f; }                // features are ReLU outputs: 0 is the maximum's identity
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int y = qy * 2 + (s >> 1), x = qx * 2 + (s & 1);
            if (y >= H || x >= W) continue;                                      // wave-uniform
            const float* __restrict__ fx = f + ((size_t)y * W + x) * (size_t)C;
            const float* __restrict__ fy = fx + plane * (size_t)C;
            float vx[8], vy[8], sx = 0.f, sy = 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                vx[j] = j < J ? fx[j * 64 + lane] : 0.f; vy[j] = j < J ? fy[j * 64 + lane] : 0.f;
                sx = fmaf(vx[j], vx[j], sx); sy = fmaf(vy[j], vy[j], sy);
                mx[j] = fmaxf(mx[j], vx[j]); my[j] = fmaxf(my[j], vy[j]);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { sx += __shfl_xor(sx, d, 64); sy += __shfl_xor(sy, d, 64); }
            const float dx = sqrtf(sx) + LP_EPS, dy = sqrtf(sy) + LP_EPS;        // eps outside the root
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) { const float e = vx[j] / dx - vy[j] / dy; t = fmaf(wl[j], e * e, t); }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
            sum += (double)t;
        }
        if (pooled && qy < Hp && qx < Wp) {
            float* px = pooled + ((size_t)qy * Wp + qx) * (size_t)C;
            float* py = px + (size_t)Hp * (size_t)Wp * (size_t)C;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j < J) { px[j * 64 + lane] = mx[j]; py[j * 64 + lane] = my[j]; }
        }
    }
    if (lane == 0) s_part[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

struct LpipsFinish { unsigned begin[5], count[5]; double pixels[5]; };

__global__ __launch_bounds__(64) void k_lpips_finish(LpipsFinish fin, const double* __restrict__ partial, double* __restrict__ rows, int capacity,
                                                     int32_t* __restrict__ cursor) {
    const unsigned lane = threadIdx.x;
    double tap[5], total = 0.0;
    for (int k = 0; k < 5; k++) {
        double s = 0.0;
        for (unsigned i = lane; i < fin.count[k]; i += 64) s += partial[fin.begin[k] + i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        tap[k] = s / fin.pixels[k];
        total += tap[k];
    }
    if (lane == 0) {
        const int32_t at = cursor[0];
        if (at >= 0 && at < capacity) {
            double* r = rows + (size_t)at * 6;
            for (int k = 0; k < 5; k++) r[k] = tap[k];
            r[5] = total;
        }
        cursor[0] = at + 1;                 // also past a full array: the host sees the overrun
    }
}

// ---- host: the layer table and the workspace layout ---------------------------------------------------------------------------------
const int kConvCin[13]  = {4, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kConvCout[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kBlockConvs[5] = {2, 2, 3, 3, 3};
const int kTapC[5] = {64, 128, 256, 512, 512};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
unsigned tap_workgroups(int h, int w) {
    const size_t nq = (size_t)((w + 1) / 2) * (size_t)((h + 1) / 2);
    return (unsigned)((nq + 4 * LP_QUADS_PER_WAVE - 1) / (4 * LP_QUADS_PER_WAVE));
}

struct LpipsLayout { size_t input, a, b, tap[5], partial, total; unsigned part_begin[5], part_count[5]; int h[5], w[5]; };

// H, W in [16, 8192] (checked by the callers): every product below stays far inside size_t and the partial counts inside 32 bits
LpipsLayout lpips_layout(int H, int W) {
    LpipsLayout L;
    size_t at = 0;
    const size_t hw = (size_t)H * (size_t)W;
    L.input = at; at = align256(at + 2 * hw * 4 * sizeof(float));
    L.a = at; at = align256(at + 2 * hw * 64 * sizeof(float));                                  // conv1_1's output is the largest non-tap map
    L.b = at; at = align256(at + 2 * (size_t)(H / 2) * (size_t)(W / 2) * 64 * sizeof(float));   // the pooled maps, and conv{3,4,5}_2's outputs
    unsigned parts = 0;
    for (int k = 0; k < 5; k++) {
        L.h[k] = H >> k; L.w[k] = W >> k;
        L.tap[k] = at; at = align256(at + 2 * (size_t)L.h[k] * (size_t)L.w[k] * (size_t)kTapC[k] * sizeof(float));
        L.part_begin[k] = parts; L.part_count[k] = tap_workgroups(L.h[k], L.w[k]); parts += L.part_count[k];
    }
    L.partial = at; at = align256(at + (size_t)parts * sizeof(double));
    L.total = at;
    return L;
}

bool lpips_size_ok(int H, int W) { return H >= 16 && W >= 16; }

int launch_conv(int n, int H, int W, int Cin, int Cout, const float* in, const float* wk, const float* bias, float* out, hipStream_t stream) {
    const int tiles_x = (W + LP_TW - 1) / LP_TW, tiles_y = (H + LP_TH - 1) / LP_TH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(Cout / LP_NT), (unsigned)n);
    if (Cin == 4) hipLaunchKernelGGL((k_conv3x3_relu<4>), grid, dim3(256), 0, stream, H, W, Cin, Cout, tiles_x, in, wk, bias, out);
    else hipLaunchKernelGGL((k_conv3x3_relu<16>), grid, dim3(256), 0, stream, H, W, Cin, Cout, tiles_x, in, wk, bias, out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t egs_lpips_workspace_bytes(int height, int width) {
    if (!lpips_size_ok(height, width) || height > 8192 || width > 8192) return 0;
    return lpips_layout(height, width).total;
}

int egs_lpips_tap_offsets(int height, int width, int64_t* offsets /*[5]*/) {
    if (!offsets || !lpips_size_ok(height, width)) return EGS_ERR_ARG;
    if (height > 8192 || width > 8192) return EGS_ERR_RANGE;
    const LpipsLayout L = lpips_layout(height, width);
    for (int k = 0; k < 5; k++) offsets[k] = (int64_t)L.tap[k];
    return 0;
}

int egs_conv3x3_relu_nhwc(int n, int height, int width, int cin, int cout, const float* in, const float* packed_w, const float* bias, float* out,
                          void* stream) {
    if (n < 1 || height < 1 || width < 1 || !in || !packed_w || !bias || !out || in == out) return EGS_ERR_ARG;
    if ((cin != 4 && (cin < 16 || cin % 16)) || cout < LP_NT || cout % LP_NT) return EGS_ERR_ARG;
    if (((uintptr_t)in | (uintptr_t)packed_w | (uintptr_t)out) & 15) return EGS_ERR_ARG;                // 16-byte loads
    if (height > 32767 || width > 32767 || cin > 4096 || cout > 4096 || n > 65535) return EGS_ERR_RANGE;
    if (((size_t)(width + LP_TW - 1) / LP_TW) * ((size_t)(height + LP_TH - 1) / LP_TH) >= ((size_t)1 << 31)) return EGS_ERR_RANGE;
    return launch_conv(n, height, width, cin, cout, in, packed_w, bias, out, (hipStream_t)stream);
}

int egs_lpips_forward(int height, int width, const uint8_t* q_x, const uint8_t* q_y, const float* keep, const egs_lpips_weights* weights,
                      void* workspace, void* rows, int capacity, int32_t* cursor, void* stream) {
    if (!lpips_size_ok(height, width) || !q_x || !q_y || !weights || !workspace || !rows || !cursor || capacity < 0) return EGS_ERR_ARG;
    if ((uintptr_t)workspace & 255) return EGS_ERR_ARG;
    for (int i = 0; i < 13; i++) if (!weights->conv_w[i] || ((uintptr_t)weights->conv_w[i] & 15) || !weights->conv_b[i]) return EGS_ERR_ARG;
    for (int k = 0; k < 5; k++) if (!weights->lin[k]) return EGS_ERR_ARG;
    if (height > 8192 || width > 8192) return EGS_ERR_RANGE;
    const hipStream_t st = (hipStream_t)stream;
    const LpipsLayout L = lpips_layout(height, width);
    char* ws = (char*)workspace;
    float* input = (float*)(ws + L.input); float* A = (float*)(ws + L.a); float* B = (float*)(ws + L.b);
    double* partial = (double*)(ws + L.partial);
    const size_t hw = (size_t)height * (size_t)width;
    hipLaunchKernelGGL(k_lpips_input, dim3((unsigned)((hw + 255) / 256), 2), dim3(256), 0, st, height, width, q_x, q_y, keep, input);
    LpipsFinish fin;
    const float* src = input;                                   // what the block's first convolution reads
    int layer = 0;
    for (int k = 0; k < 5; k++) {
        const int h = L.h[k], w = L.w[k];
        float* tap = (float*)(ws + L.tap[k]);
        // the block's chain: src -> A [-> B] -> tap   (src is B itself from the second block on: B is free again once A is written)
        float* const dst2[2] = {A, tap}; float* const dst3[3] = {A, B, tap};
        const float* cur = src;
        for (int j = 0; j < kBlockConvs[k]; j++, layer++) {
            float* dst = kBlockConvs[k] == 2 ? dst2[j] : dst3[j];
            const int rc = launch_conv(2, h, w, kConvCin[layer], kConvCout[layer], cur, weights->conv_w[layer], weights->conv_b[layer], dst, st);
            if (rc) return rc;
            cur = dst;
        }
        hipLaunchKernelGGL(k_lpips_tap, dim3(L.part_count[k]), dim3(256), 0, st, h, w, kTapC[k], (const float*)tap, weights->lin[k],
                           k < 4 ? B : (float*)nullptr, partial + L.part_begin[k]);
        fin.begin[k] = L.part_begin[k]; fin.count[k] = L.part_count[k]; fin.pixels[k] = (double)h * (double)w;
        src = B;
    }
    hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(64), 0, st, fin, (const double*)partial, (double*)rows, capacity, cursor);
    return (int)hipGetLastError();
}

}  // extern "C"
