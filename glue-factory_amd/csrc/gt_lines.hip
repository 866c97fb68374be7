// Close-point counts of the line ground truth, fused (no B x A x C x P intermediates).
//
// Replaces the point-to-segment test of gluefactory/geometry/gt_generation.py:173-206 and the `.sum(-1)` over the
// sampled points of :296-300 / :470-480: count[b,a,c] = how many of the P points sampled on line c of the other view
// lie within dist_th of segment a and project onto it.  Same skeleton as gt_nn.hip / gt_epi.hip: one thread per own
// segment (end point, direction, length in registers), the other view's points through LDS in tiles, every lane reading
// the same LDS address (a broadcast).
//
// The arithmetic is the one torch runs on a CUDA tensor, every operation rounded to fp16 by itself:
//   rel   = half(p - end)                                   fp32 subtract, one rounding
//   along = half(half(rel.x * dir.x) + half(rel.y * dir.y))
//   perp  = half(half(rel.y * dir.x) - half(rel.x * dir.y))
//   count += along <= 0 && |along| <= len && |perp| < th
// Native fp16 multiply / add / subtract round correctly, which is what torch's compute-in-fp32-then-round gives (the fp32
// result of two fp16 operands is exact for a product and within double rounding's safe width for a sum: 24 >= 2 * 11 + 2).
// No contraction: a fused multiply-add skips the rounding of the product and changes counts, so this translation unit is
// built with -ffp-contract=off (csrc/Makefile) and carries the pragma below.  fp16 subnormals are kept (the default mode of
// a kernel); NaN / inf operands fall out of the comparisons as they do in torch: the point does not count.
//
// dist_th: torch compares the fp16 tensor |perp| with a Python scalar by casting the scalar to the tensor's type first, so
// the entry rounds dist_th to fp16 (round to nearest even) and the kernel compares with that value: with dist_th = 4.298
// (-> 4.296875) a point at |perp| == 4.296875 does NOT count (the constructed case of tests/test_gpu_gt_lines.py,
// test_threshold_rounding, compares exactly this against the torch form on the device).
#include <hip/hip_fp16.h>

#include "gf_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int LC_SEGS = 256;     // own segments of one workgroup, one per thread
constexpr int LC_LINES = 32;     // lines of the other view per workgroup: a stored row of `count` is 32 ints = 128 B
constexpr int LC_PTS = 64;       // points of one line staged at a time; longer lines go through in chunks

__device__ __forceinline__ int lc_passes(float px, float py, float ex, float ey, __half2 d, float len, float th) {
    const __half2 r = __floats2half2_rn(px - ex, py - ey);
    const __half2 m = __hmul2(r, d);                              // (rel.x * dir.x, rel.y * dir.y)
    const __half2 x = __hmul2(__lowhigh2highlow(r), d);           // (rel.y * dir.x, rel.x * dir.y)
    const float along = __half2float(__hadd(__low2half(m), __high2half(m)));
    const float perp = __half2float(__hsub(__low2half(x), __high2half(x)));
    return (along <= 0.f) & (fabsf(along) <= len) & (fabsf(perp) < th);
}

__global__ __launch_bounds__(LC_SEGS) void line_close_counts_kernel(
    const float* __restrict__ end, const __half* __restrict__ dir, const __half* __restrict__ len,
    const float* __restrict__ pts, const uint8_t* __restrict__ keep, int32_t* __restrict__ count, int A, int C, int P,
    float th, int transposed) {
    __shared__ float2 sp[LC_LINES * LC_PTS];         // staged points; x = NaN where keep is not set (never counts)
    __shared__ int sc[LC_LINES][LC_SEGS + 1];        // counts; +1: the [B,A,C] read-out below walks a column
    const int tid = threadIdx.x;
    const size_t b = blockIdx.z;
    const int c0 = blockIdx.y * LC_LINES, a0 = blockIdx.x * LC_SEGS;
    const int nc = min(LC_LINES, C - c0);
    const int a = a0 + tid;
    const size_t s = b * A + min(a, A - 1);
    const float ex = end[s * 2], ey = end[s * 2 + 1];
    const __half2 d = __halves2half2(dir[s * 2], dir[s * 2 + 1]);
    const float ln = __half2float(len[s]);
    for (int c = 0; c < nc; ++c) sc[c][tid] = 0;
    for (int p0 = 0; p0 < P; p0 += LC_PTS) {
        const int np = min(LC_PTS, P - p0);
        __syncthreads();
        for (int i = tid; i < nc * np; i += LC_SEGS) {
            const int c = i / np, p = i - c * np;
            const size_t g = (b * C + c0 + c) * P + p0 + p;
            const bool k = keep == nullptr || keep[g] != 0;
            sp[c * LC_PTS + p] = make_float2(k ? pts[g * 2] : NAN, pts[g * 2 + 1]);
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const float2* row = sp + c * LC_PTS;
            int n = 0;
#pragma unroll 8
            for (int p = 0; p < np; ++p) n += lc_passes(row[p].x, row[p].y, ex, ey, d, ln, th);
            sc[c][tid] += n;                         // a thread only ever touches its own column until the read-out
        }
    }
    if (transposed) {                                // count [B,C,A]: the lanes' stores are consecutive in a
        if (a < A)
            for (int c = 0; c < nc; ++c) count[(b * C + c0 + c) * A + a] = sc[c][tid];
    } else {                                         // count [B,A,C]: 32 lanes store one row segment of 32 consecutive ints
        __syncthreads();
        const int cc = tid % LC_LINES;
        const int na = min(LC_SEGS, A - a0);
        if (cc < nc)
            for (int r = tid / LC_LINES; r < na; r += LC_SEGS / LC_LINES)
                count[(b * A + a0 + r) * C + c0 + cc] = sc[cc][r];
    }
}

}  // namespace

extern "C" int gf_line_close_counts(const float* end, const uint16_t* dir, const uint16_t* len, const float* pts,
                                    const uint8_t* keep, int32_t* count, int B, int A, int C, int P, float dist_th,
                                    int transposed, void* stream) {
    if (B <= 0 || A <= 0 || C <= 0 || P <= 0) return GF_ERR_UNSUPPORTED;
    const int ct = (C + LC_LINES - 1) / LC_LINES;
    if (B > 65535 || ct > 65535) return GF_ERR_UNSUPPORTED;      // grid limits of the y / z dimensions
    const float th = __half2float(__float2half_rn(dist_th));     // torch's rule: the scalar takes the tensor's type
    line_close_counts_kernel<<<dim3((A + LC_SEGS - 1) / LC_SEGS, ct, B), LC_SEGS, 0, gf_stream(stream)>>>(
        end, reinterpret_cast<const __half*>(dir), reinterpret_cast<const __half*>(len), pts, keep, count, A, C, P, th,
        transposed);
    return gf_launched();
}
