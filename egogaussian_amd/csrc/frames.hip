// frames.hip -- the 8-bit frame store's decode (include/egs_raster.h egs_frame_decode, egs_frame_store_layout): S packed float32 frames
// (graph.pack_frame / pack_label_frame, every float of every row, the gaps between segments as 0.0) written in ONE launch from a
// device-resident dataset kept in its native precision, the frames chosen on the device through a ring of indices.  Every decoded value has
// one right answer; egogaussian_amd/frames.py FrameStore.frame is the torch statement of it.
//
// The store's arrays (F frames of one size and one layout; egs_frame_store_layout gives the strides):
//   img    uint8  [F][image_stride]        the 3 H W image bytes in the CHW order of `gt`, then zero bytes up to image_stride =
//                                          3 H W rounded up to 16 BYTES: every 16-byte load of a frame's image is aligned and inside it
//                                          (absent for the label layout; pre-multiplied by the object mask for the object-loss layout)
//   bits   uint32 [F][n_planes][plane_words]   one bit per pixel, pixel p is bit p % 32 of word p / 32, gate first, then obj_mask;
//                                          plane_words = ceil(H W / 32) rounded up to 4 WORDS (16 bytes); unused bits are 0
//   small  float  [F][small_floats]        the frame's floats from the start of `cam` to the end of the last of cam / accum_R / accum_T / pose_rows,
//                                          as they lie in the packed frame (36, 48, 60 or -- with the pose_rows word -- 64 floats: a multiple of 4, so 16-byte rows)
//   table  float  [256]                    byte -> float, filled by the host with uint8 / 255.0 (true division): byte * (1 / 255.f) is NOT
//                                          that quotient at 126 of the 256 codes, so no reciprocal appears here.  Staged in LDS.
// A packed frame is a sequence of segments, each starting on a 16-byte boundary and padded with zeros to the next one:
//   [image] small [gate] [obj_mask]     (label layout: small [gate] obj_mask)
//
// Mapping.  grid (x, S): row k of `out` takes frame ring[(ctl[0] + k) % ctl[1]].
//   VEC (out, img and small 16-byte aligned): a lane owns one RUN of 16 consecutive floats of one segment, counted from the segment's start --
//   16 image bytes in one 16-byte load, or one half-word of a bit plane, or four float4 of the small block -- and writes it with up to four
//   float4 stores (a segment's padded length is a multiple of 4 floats, so its last run is 1 .. 4 whole float4).  The image segment is
//   treated as FLAT 3 H W elements: channel c starts at float c H W, which is not 16-byte aligned when H W % 4 != 0, and a lane's run may
//   straddle a channel boundary -- neither matters to a flat run, so there is no fall-back on H W.  A workgroup of 256 lanes owns 256 runs.
//   Scalar (any 4-byte aligned out): lane t takes floats t, t + 256, t + 512, t + 768 of the workgroup's 1024, finds each one's segment,
//   loads one byte / one word / one float and stores 4 bytes (consecutive lanes, consecutive addresses).  Same values either way.
//   Bytes at 540x960 with gate and obj_mask: 1.68 MB read, 10.4 MB written per frame.
//
// Safety.  The frame index is clamped into [0, F) and ctl into [0, length) x [1, ring_capacity] before anything is addressed with them;
// workgroup (0, k) counts each clamped row (and a clamped ctl, once) into the sticky status[0].  Nothing outside row k's frame_floats is written.
//
// k_frame_advance (one lane, a second launch): ctl[0] = (ctl[0] + S) % ctl[1].  It is a launch of its own because no workgroup of the
// decode may change the cursor while another may still read it.
#include "egs_common.h"

#define FRAME_WG 256
#define FRAME_RUN 16                 // floats per lane of the vector path
#define FRAME_SCALAR_PER_WG 1024     // floats per workgroup of the scalar path

namespace {

enum { SEG_IMAGE = 0, SEG_SMALL = 1, SEG_PLANE = 2 };

struct FrameSeg {
    int kind;                        // SEG_*
    int plane;                       // SEG_PLANE: which bit plane
    unsigned long long begin;        // first float of the segment in the packed frame
    unsigned long long padded;       // floats up to the next segment (a multiple of 4)
    unsigned run0;                   // first run of the segment (vector path)
};

struct FrameArgs {
    FrameSeg seg[4];
    int n_seg;
    unsigned total_runs;
    unsigned long long frame_floats, image_stride, plane_words, small_floats;
    int n_planes, n_frames, ring_capacity;
};

// the sanitised control words: 1 <= len <= ring_capacity, 0 <= cursor < len
__device__ __forceinline__ void frame_ctl(const int32_t* __restrict__ ctl, int ring_capacity, int& cursor, int& len, bool& bad) {
    const int c = ctl[0], l = ctl[1];
    len = min(max(l, 1), ring_capacity);
    cursor = c % len; if (cursor < 0) cursor += len;
    bad = l != len || c != cursor;
}

// the frame of row k, clamped; workgroup x == 0 keeps the count
__device__ __forceinline__ unsigned frame_of_row(const FrameArgs& a, const int32_t* __restrict__ ring, const int32_t* __restrict__ ctl,
                                                 int32_t* __restrict__ status) {
    int cursor, len; bool bad_ctl;
    frame_ctl(ctl, a.ring_capacity, cursor, len, bad_ctl);
    const int k = (int)blockIdx.y;
    const int idx = ring[(cursor + k) % len];
    const int f = min(max(idx, 0), a.n_frames - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int n = (f != idx ? 1 : 0) + ((bad_ctl && k == 0) ? 1 : 0);
        if (n) atomicAdd(status, n);
    }
    return (unsigned)f;
}

__device__ __forceinline__ float4 bits4(unsigned h) {
    return make_float4((h & 1u) ? 1.f : 0.f, (h & 2u) ? 1.f : 0.f, (h & 4u) ? 1.f : 0.f, (h & 8u) ? 1.f : 0.f);
}

__device__ __forceinline__ float4 bytes4(const float* lut, unsigned w) {
    return make_float4(lut[w & 255u], lut[(w >> 8) & 255u], lut[(w >> 16) & 255u], lut[w >> 24]);
}

// grid: (ceil(total_runs / 256), S)
__global__ __launch_bounds__(FRAME_WG) void k_frame_decode_vec(FrameArgs a, const uint8_t* __restrict__ img, const uint32_t* __restrict__ bits,
                                                               const float* __restrict__ small, const float* __restrict__ table,
                                                               const int32_t* __restrict__ ring, const int32_t* __restrict__ ctl,
                                                               int32_t* __restrict__ status, float* __restrict__ out) {
    __shared__ float lut[256];
    const unsigned t = threadIdx.x;
    lut[t] = table ? table[t] : 0.f;
    const unsigned f = frame_of_row(a, ring, ctl, status);
    __syncthreads();
    const unsigned g = blockIdx.x * FRAME_WG + t;
    if (g >= a.total_runs) return;
    FrameSeg sg = a.seg[0];                                                             // (selects, not an indexed read of the arguments)
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (j < a.n_seg && g >= a.seg[j].run0) sg = a.seg[j];
    const unsigned long long r = g - sg.run0, d0 = r * FRAME_RUN;                       // the run's first float within its segment
    const unsigned long long left = (sg.padded - d0) >> 2;                              // whole float4 left in the segment: >= 1
    const int nq = left < 4ull ? (int)left : 4;
    float4 v[4];
    if (sg.kind == SEG_IMAGE) {
        const uint4 b = *reinterpret_cast<const uint4*>(img + (size_t)f * a.image_stride + d0);      // 16 r + 15 < image_stride
        v[0] = bytes4(lut, b.x); v[1] = bytes4(lut, b.y); v[2] = bytes4(lut, b.z); v[3] = bytes4(lut, b.w);
    } else if (sg.kind == SEG_PLANE) {
        const uint32_t w = bits[((size_t)f * (size_t)a.n_planes + (size_t)sg.plane) * a.plane_words + (r >> 1)];      // r / 2 < plane_words
        const unsigned h = (w >> (16u * (unsigned)(r & 1ull))) & 0xffffu;
        v[0] = bits4(h); v[1] = bits4(h >> 4); v[2] = bits4(h >> 8); v[3] = bits4(h >> 12);
    } else {
        const float4* __restrict__ src = reinterpret_cast<const float4*>(small + (size_t)f * a.small_floats + d0);
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = src[q < nq ? q : 0];                           // (never past the frame's block)
    }
    float4* __restrict__ dst = reinterpret_cast<float4*>(out + (size_t)blockIdx.y * a.frame_floats + sg.begin + d0);
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (q < nq) dst[q] = v[q];
}

// grid: (ceil(frame_floats / 1024), S)
__global__ __launch_bounds__(FRAME_WG) void k_frame_decode_scalar(FrameArgs a, const uint8_t* __restrict__ img, const uint32_t* __restrict__ bits,
                                                                  const float* __restrict__ small, const float* __restrict__ table,
                                                                  const int32_t* __restrict__ ring, const int32_t* __restrict__ ctl,
                                                                  int32_t* __restrict__ status, float* __restrict__ out) {
    __shared__ float lut[256];
    const unsigned t = threadIdx.x;
    lut[t] = table ? table[t] : 0.f;
    const unsigned f = frame_of_row(a, ring, ctl, status);
    __syncthreads();
    float* __restrict__ row = out + (size_t)blockIdx.y * a.frame_floats;
#pragma unroll
    for (int j = 0; j < FRAME_SCALAR_PER_WG / FRAME_WG; j++) {
        const unsigned long long e = (unsigned long long)blockIdx.x * FRAME_SCALAR_PER_WG + (unsigned)j * FRAME_WG + t;
        if (e >= a.frame_floats) break;
        FrameSeg sg = a.seg[0];
#pragma unroll
        for (int i = 1; i < 4; i++)
            if (i < a.n_seg && e >= a.seg[i].begin) sg = a.seg[i];
        const unsigned long long d = e - sg.begin;                                      // < sg.padded
        float v;
        if (sg.kind == SEG_IMAGE) v = lut[img[(size_t)f * a.image_stride + d]];         // d < 3 H W rounded up to 4 <= image_stride; the pad bytes are 0
        else if (sg.kind == SEG_PLANE)
            v = ((bits[((size_t)f * (size_t)a.n_planes + (size_t)sg.plane) * a.plane_words + (d >> 5)] >> (unsigned)(d & 31ull)) & 1u) ? 1.f : 0.f;
        else v = small[(size_t)f * a.small_floats + d];
        row[e] = v;
    }
}

__global__ __launch_bounds__(64) void k_frame_advance(int S, int ring_capacity, int32_t* __restrict__ ctl) {
    if (threadIdx.x == 0) {
        int cursor, len; bool bad;
        frame_ctl(ctl, ring_capacity, cursor, len, bad);
        ctl[0] = (cursor + S % len) % len;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline unsigned long long up4(unsigned long long x) { return (x + 3ull) & ~3ull; }

// the layout of graph.frame_layout for `flags`, and the store's strides
int frame_layout_of(int height, int width, int flags, egs_frame_layout* L) {
    if (height < 1 || width < 1 || !L || (flags & ~63)) return EGS_ERR_ARG;
    if ((size_t)height * (size_t)width >= ((size_t)1 << 31)) return EGS_ERR_RANGE;
    const bool dynamic = flags & EGS_FRAME_DYNAMIC, motion = flags & EGS_FRAME_MOTION, gated = flags & EGS_FRAME_GATED;
    const bool object_loss = flags & EGS_FRAME_OBJECT_LOSS, label = flags & EGS_FRAME_LABEL_PHASE, pose_rows = flags & EGS_FRAME_POSE_ROWS;
    if (label && (dynamic || motion || object_loss)) return EGS_ERR_MODE;
    if (pose_rows && !motion) return EGS_ERR_MODE;                           // the frame word of a pose sequence goes with a pose
    const unsigned long long n_pix = (unsigned long long)height * (unsigned long long)width;
    unsigned long long end = 0;
    L->image_floats = label ? 0 : 3 * n_pix;
    end = up4((unsigned long long)L->image_floats);
    L->small_begin = (int64_t)end;
    end = up4(end + 35);
    if (dynamic) end = up4(end + 9);
    if (motion) end = up4(end + 12);
    if (pose_rows) end = up4(end + 4);
    L->small_floats = (int64_t)end - L->small_begin;
    L->gate_begin = -1; L->obj_mask_begin = -1;
    if (gated) { L->gate_begin = (int64_t)end; end = up4(end + n_pix); }
    if (object_loss || label) { L->obj_mask_begin = (int64_t)end; end = up4(end + n_pix); }
    L->frame_floats = (int64_t)end;
    L->n_planes = (gated ? 1 : 0) + ((object_loss || label) ? 1 : 0);
    L->image_stride = label ? 0 : (int64_t)((3 * n_pix + 15ull) & ~15ull);
    L->plane_words = (int64_t)((((n_pix + 31ull) >> 5) + 3ull) & ~3ull);
    return 0;
}

}  // namespace

extern "C" {

int egs_frame_store_layout(int height, int width, int flags, egs_frame_layout* layout) {
    return frame_layout_of(height, width, flags, layout);
}

int egs_frame_decode(int height, int width, int flags, int n_frames, int n_rows, const uint8_t* img, const uint32_t* bits, const float* small,
                     const float* table, const int32_t* ring, int ring_capacity, int32_t* ctl, int32_t* status, float* out, void* stream) {
    if (height < 1 || width < 1 || n_frames < 1 || n_rows < 1 || ring_capacity < 1) return EGS_ERR_ARG;
    egs_frame_layout L;
    const int rc = frame_layout_of(height, width, flags, &L);
    if (rc) return rc;
    if (!small || !ring || !ctl || !status || !out) return EGS_ERR_ARG;
    if (L.image_floats && (!img || !table)) return EGS_ERR_ARG;
    if (L.n_planes && !bits) return EGS_ERR_ARG;
    if (n_rows > 65535) return EGS_ERR_RANGE;                                // rows are the grid's y
    FrameArgs a = {};
    a.frame_floats = (unsigned long long)L.frame_floats; a.image_stride = (unsigned long long)L.image_stride;
    a.plane_words = (unsigned long long)L.plane_words; a.small_floats = (unsigned long long)L.small_floats;
    a.n_planes = (int)L.n_planes; a.n_frames = n_frames; a.ring_capacity = ring_capacity;
    int n = 0, plane = 0;
    unsigned long long runs = 0;
    auto add = [&](int kind, int pl, unsigned long long begin, unsigned long long padded) {
        a.seg[n].kind = kind; a.seg[n].plane = pl; a.seg[n].begin = begin; a.seg[n].padded = padded; a.seg[n].run0 = (unsigned)runs;
        runs += (padded + FRAME_RUN - 1) / FRAME_RUN;
        n++;
    };
    const unsigned long long plane_pad = up4((unsigned long long)height * (unsigned long long)width);
    if (L.image_floats) add(SEG_IMAGE, 0, 0, up4((unsigned long long)L.image_floats));
    add(SEG_SMALL, 0, (unsigned long long)L.small_begin, (unsigned long long)L.small_floats);
    if (L.gate_begin >= 0) add(SEG_PLANE, plane++, (unsigned long long)L.gate_begin, plane_pad);
    if (L.obj_mask_begin >= 0) add(SEG_PLANE, plane++, (unsigned long long)L.obj_mask_begin, plane_pad);
    a.n_seg = n; a.total_runs = (unsigned)runs;                                // < 5 * 2^31 / 16
    const bool vec = aligned16(out) && aligned16(img) && aligned16(small);
    if (vec) {
        const unsigned wgs = (a.total_runs + FRAME_WG - 1) / FRAME_WG;
        hipLaunchKernelGGL(k_frame_decode_vec, dim3(wgs, (unsigned)n_rows), dim3(FRAME_WG), 0, (hipStream_t)stream, a, img, bits, small, table, ring, ctl,
                           status, out);
    } else {
        const unsigned wgs = (unsigned)((a.frame_floats + FRAME_SCALAR_PER_WG - 1) / FRAME_SCALAR_PER_WG);
        hipLaunchKernelGGL(k_frame_decode_scalar, dim3(wgs, (unsigned)n_rows), dim3(FRAME_WG), 0, (hipStream_t)stream, a, img, bits, small, table, ring,
                           ctl, status, out);
    }
    hipLaunchKernelGGL(k_frame_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, n_rows, ring_capacity, ctl);
    return (int)hipGetLastError();
}

}  // extern "C"
