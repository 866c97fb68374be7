// Homography view synthesis: V output views from S source images, in two launches (one when no view is blurred).
//
// Stands where gluefactory/datasets/homographies.py:37-44 + :217-233 run cv2.warpPerspective, an albumentations chain and
// the grayscale reduction on DataLoader workers, one view at a time.  Here the sources sit in HBM as one padded NHWC buffer
// (uint8 or fp32), every view is described by a row of small device tables, and
//   gf_hv_warp    gathers the view (bilinear, constant-0 border on the source's OWN size), applies the PRE stage (gamma, value
//                 shift) and, when `finish` is set, the POST stage (a v + b clamped, gray reduction);
//   gf_hv_filter  correlates every view with its own sparse tap table (box blur, motion blur, or the single identity tap),
//                 reflect-101 border, then the POST stage.
// No host read, nothing allocated, kernel nodes only: both calls can be captured; a replay sees whatever the tables hold then.
//
// ---- gf_hv_warp, per output pixel (x, y) of view v, all in fp32, in exactly this order ---------------------------------------
//   h = Hinv[v] (row major, patch pixel -> source pixel; pixel centres at integer coordinates as in cv2.warpPerspective)
//   d  = fmaf(h20, x, fmaf(h21, y, h22))
//   sx = fmaf(h00, x, fmaf(h01, y, h02)) / d          sy = fmaf(h10, x, fmaf(h11, y, h12)) / d
//   s = clamp(view_src[v], 0, S-1); (w, h) = src_sizes[s] clamped to [0, Wmax] x [0, Hmax]
//   sampled value 0 (for every channel, no integer conversion) when d is not finite, |d| < GF_HV_EPS_D, or not
//   (-1 <= sx <= w and -1 <= sy <= h); otherwise x0 = floorf(sx), fx = sx - x0 (y alike) and, with t(i, j) the source value at
//   (x0 + i, y0 + j) or 0 when that lies outside [0, w) x [0, h) (such a tap is not loaded: the padding is never read),
//   top = fmaf(fx, t10 - t00, t00), bot = fmaf(fx, t11 - t01, t01), val = fmaf(fy, bot - top, top).
//   uint8 sources interpolate the raw 0..255 values and divide ONCE: val = val / 255.0f (an identity Hinv gives u / 255.0f).
//   PRE:  g = params[v][0]: val = powf(val, g) when g != 1 (val >= 0 for uint8; fp32 sources are expected in [0, 1]);
//         s = params[v][1]: C = 1: val = clamp(val + s, 0, 1) when s != 0;
//                           C = 3: m = max(r, g, b); when s != 0 and m > 0 every channel is multiplied by clamp(m + s, 0, 1) / m.
//   POST (only with finish): a = params[v][2], b = params[v][3]: val = min(max(fmaf(a, val, b), 0), 1) per channel; then with
//         gray and C = 3 the single output channel fmaf(0.114, B, fmaf(0.587, G, 0.299 * R)).
//   Pixels whose sampled value is 0 run through the same stages (the reference augments its black border too).
//
// ---- gf_hv_filter, per output pixel -------------------------------------------------------------------------------------
//   n = clamp(ntaps[v], 1, GF_HV_MAXTAPS); acc = 0; for t = 0 .. n-1 in order: acc = fmaf(tap_w[v][t], in(r(x + dx_t), r(y + dy_t)), acc)
//   with dx, dy clamped to [-GF_HV_RADIUS, GF_HV_RADIUS] and r the reflect-101 index map (-i for i < 0, 2 (n-1) - i for i >= n;
//   one reflection suffices because every extent exceeds GF_HV_RADIUS).  Then POST exactly as above.  Correlation, not
//   convolution: tap (dx, dy) reads the pixel to the right / below for positive offsets.
//
// Layout: a workgroup of 256 lanes owns a 64 x 16 output tile of one view (a compact source footprint under any rotation, so the
// four taps of neighbouring pixels meet in L1/L2).  In the warp a lane owns 4 consecutive x and stores 16 bytes per channel when
// pw % 4 == 0 and `out` is 16-byte aligned; in the filter a wave owns whole 64-pixel rows (256-byte stores, conflict-free LDS
// reads: 64 consecutive dwords) and the tile + the halo the view's taps really reach go through LDS.  Tap count, offsets and
// weights are indexed by blockIdx and the loop counter only, so they stay wave-uniform (scalar loads).
#include "gf_launch.h"

namespace {

constexpr int TW = 64, TH = 16;                        // output tile
constexpr int R = GF_HV_RADIUS;
constexpr int LW = TW + 2 * R, LH = TH + 2 * R;        // LDS tile with the full halo: 88 x 40 floats = 14080 bytes

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float post(float v, float a, float b) { return clamp01(fmaf(a, v, b)); }
__device__ __forceinline__ float gray3(float r, float g, float b) { return fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r)); }

__device__ __forceinline__ float ld_src(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float ld_src(const float* p) { return *p; }

template <typename T, int C>
__global__ __launch_bounds__(256) void hv_warp_kernel(const T* __restrict__ src, const int32_t* __restrict__ src_sizes,
                                                      const int32_t* __restrict__ view_src, const float* __restrict__ Hinv,
                                                      const float* __restrict__ params, float* __restrict__ out, int S, int Hmax,
                                                      int Wmax, int ph, int pw, int finish, int gray, int vec) {
    const int v = blockIdx.z;
    const int xb = blockIdx.x * TW + (threadIdx.x & 15) * 4;
    const int y = blockIdx.y * TH + (threadIdx.x >> 4);
    if (y >= ph || xb >= pw) return;
    const int s = min(max(view_src[v], 0), S - 1);
    const int w = min(max(src_sizes[2 * s], 0), Wmax), h = min(max(src_sizes[2 * s + 1], 0), Hmax);
    const float* hm = Hinv + (size_t)v * 9;
    const float h00 = hm[0], h01 = hm[1], h02 = hm[2], h10 = hm[3], h11 = hm[4], h12 = hm[5], h20 = hm[6], h21 = hm[7], h22 = hm[8];
    const float* pr = params + (size_t)v * GF_HV_NPARAM;
    const float gam = pr[0], shift = pr[1], pa = pr[2], pb = pr[3];
    const T* base = src + (size_t)s * Hmax * Wmax * C;
    const float fy_ = (float)y;
    const int cout = (finish && gray) ? 1 : C;
    float res[C][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float fx_ = (float)(xb + j);
        const float d = fmaf(h20, fx_, fmaf(h21, fy_, h22));
        const float sx = fmaf(h00, fx_, fmaf(h01, fy_, h02)) / d;
        const float sy = fmaf(h10, fx_, fmaf(h11, fy_, h12)) / d;
        float val[C];
#pragma unroll
        for (int c = 0; c < C; ++c) val[c] = 0.f;
        const bool ok = isfinite(d) && fabsf(d) >= GF_HV_EPS_D && sx >= -1.f && sx <= (float)w && sy >= -1.f && sy <= (float)h;
        if (ok) {
            const float xf = floorf(sx), yf = floorf(sy);
            const float fx = sx - xf, fy = sy - yf;
            const int x0 = (int)xf, y0 = (int)yf;              // in [-1, w] x [-1, h]: the conversion cannot overflow
            const bool cx0 = x0 >= 0 && x0 < w, cx1 = x0 + 1 >= 0 && x0 + 1 < w;
            const bool cy0 = y0 >= 0 && y0 < h, cy1 = y0 + 1 >= 0 && y0 + 1 < h;
            const T* r0 = base + ((size_t)max(y0, 0) * Wmax) * C;
            const T* r1 = base + ((size_t)max(y0 + 1, 0) * Wmax) * C;
            const size_t o0 = (size_t)max(x0, 0) * C, o1 = (size_t)max(x0 + 1, 0) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t00 = (cx0 && cy0) ? ld_src(r0 + o0 + c) : 0.f;
                const float t10 = (cx1 && cy0) ? ld_src(r0 + o1 + c) : 0.f;
                const float t01 = (cx0 && cy1) ? ld_src(r1 + o0 + c) : 0.f;
                const float t11 = (cx1 && cy1) ? ld_src(r1 + o1 + c) : 0.f;
                const float top = fmaf(fx, t10 - t00, t00), bot = fmaf(fx, t11 - t01, t01);
                float r = fmaf(fy, bot - top, top);
                if (sizeof(T) == 1) r = r / 255.0f;
                val[c] = r;
            }
        }
        if (gam != 1.f) {
#pragma unroll
            for (int c = 0; c < C; ++c) val[c] = powf(val[c], gam);
        }
        if (shift != 0.f) {
            if (C == 1) {
                val[0] = clamp01(val[0] + shift);
            } else {
                const float m = fmaxf(val[0], fmaxf(val[1], val[C - 1]));
                if (m > 0.f) {
                    const float k = clamp01(m + shift) / m;
#pragma unroll
                    for (int c = 0; c < C; ++c) val[c] *= k;
                }
            }
        }
        if (finish) {
#pragma unroll
            for (int c = 0; c < C; ++c) val[c] = post(val[c], pa, pb);
            if (gray && C == 3) val[0] = gray3(val[0], val[1], val[C - 1]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) res[c][j] = val[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c >= cout) break;
        float* o = out + (((size_t)v * cout + c) * ph + y) * pw + xb;
        if (vec) {                                             // pw % 4 == 0: the group of 4 is whole and 16-byte aligned
            st4(o, res[c][0], res[c][1], res[c][2], res[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (xb + j < pw) o[j] = res[c][j];
        }
    }
}

__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);                              // only positions no stored pixel reads get clamped
}

template <int C>
__global__ __launch_bounds__(256) void hv_filter_kernel(const float* __restrict__ in, const int32_t* __restrict__ tap_off,
                                                        const float* __restrict__ tap_w, const int32_t* __restrict__ ntaps,
                                                        const float* __restrict__ params, float* __restrict__ out, int ph, int pw,
                                                        int gray) {
    __shared__ float tile[LH * LW];
    const int v = blockIdx.z;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int n = min(max(ntaps[v], 1), GF_HV_MAXTAPS);
    const int32_t* off = tap_off + (size_t)v * GF_HV_MAXTAPS * 2;
    const float* wt = tap_w + (size_t)v * GF_HV_MAXTAPS;
    int rx = 0, ry = 0;                                        // the halo this view's taps reach (wave-uniform)
    for (int t = 0; t < n; ++t) {
        rx = max(rx, abs(min(max(off[2 * t], -R), R)));
        ry = max(ry, abs(min(max(off[2 * t + 1], -R), R)));
    }
    const float pa = params[(size_t)v * GF_HV_NPARAM + 2], pb = params[(size_t)v * GF_HV_NPARAM + 3];
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;    // a wave owns rows ly, ly + 4, ly + 8, ly + 12 of the tile
    const int cout = gray ? 1 : C;
    const int lw = TW + 2 * rx, lh = TH + 2 * ry;              // the part of the LDS tile in use: rows [R-ry, ..), columns [R-rx, ..)
    float res[C][4];
    for (int c = 0; c < C; ++c) {
        const float* plane = in + ((size_t)v * C + c) * ph * pw;
        if (c) __syncthreads();
        for (int i = threadIdx.x; i < lw * lh; i += 256) {
            const int r = i / lw, q = i - r * lw;
            const int gy = reflect101(y0 - ry + r, ph), gx = reflect101(x0 - rx + q, pw);
            tile[(R - ry + r) * LW + (R - rx + q)] = plane[(size_t)gy * pw + gx];
        }
        __syncthreads();
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < n; ++t) {
            const int dx = min(max(off[2 * t], -R), R), dy = min(max(off[2 * t + 1], -R), R);
            const float wgt = wt[t];
            const float* p = tile + (R + dy + ly) * LW + (R + dx + lx);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wgt, p[4 * j * LW], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) res[c][j] = post(acc[j], pa, pb);
    }
    const int x = x0 + lx;
    if (x >= pw) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + ly + 4 * j;
        if (y >= ph) continue;
        if (gray && C == 3) {
            out[((size_t)v * ph + y) * pw + x] = gray3(res[0][j], res[1][j], res[C - 1][j]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) out[(((size_t)v * cout + c) * ph + y) * pw + x] = res[c][j];
        }
    }
}

}  // namespace

extern "C" int gf_hv_warp(const void* src, int src_dtype, const int32_t* src_sizes, const int32_t* view_src, const float* Hinv,
                          const float* params, float* out, int S, int Hmax, int Wmax, int C, int V, int Cout, int ph, int pw,
                          int finish, int gray, void* stream) {
    if (!src || !src_sizes || !view_src || !Hinv || !params || !out) return GF_ERR_SHAPE;
    if (S <= 0 || Hmax <= 0 || Wmax <= 0 || V <= 0 || ph <= 0 || pw <= 0) return GF_ERR_SHAPE;
    if (C != 1 && C != 3) return GF_ERR_SHAPE;
    if (Cout != ((finish && gray) ? 1 : C)) return GF_ERR_SHAPE;
    if (V > 65535 || (ph + TH - 1) / TH > 65535) return GF_ERR_SHAPE;
    if (src_dtype != GF_DTYPE_F32 && src_dtype != GF_DTYPE_U8) return GF_ERR_DTYPE;
    const dim3 grid((pw + TW - 1) / TW, (ph + TH - 1) / TH, V);
    const int vec = (pw % 4 == 0) && gf_aligned16(out);
    hipStream_t st = gf_stream(stream);
#define GF_HV_LAUNCH(T, CC) \
    hv_warp_kernel<T, CC><<<grid, 256, 0, st>>>((const T*)src, src_sizes, view_src, Hinv, params, out, S, Hmax, Wmax, ph, pw, \
                                                 finish != 0, gray != 0, vec)
    if (src_dtype == GF_DTYPE_U8) {
        if (C == 1) GF_HV_LAUNCH(uint8_t, 1); else GF_HV_LAUNCH(uint8_t, 3);
    } else {
        if (C == 1) GF_HV_LAUNCH(float, 1); else GF_HV_LAUNCH(float, 3);
    }
#undef GF_HV_LAUNCH
    return gf_launched();
}

extern "C" int gf_hv_filter(const float* in, const int32_t* tap_off, const float* tap_w, const int32_t* ntaps, const float* params,
                            float* out, int V, int C, int Cout, int ph, int pw, int gray, void* stream) {
    if (!in || !tap_off || !tap_w || !ntaps || !params || !out || in == out) return GF_ERR_SHAPE;
    if (V <= 0 || ph <= GF_HV_RADIUS || pw <= GF_HV_RADIUS) return GF_ERR_SHAPE;
    if (C != 1 && C != 3) return GF_ERR_SHAPE;
    if (Cout != (gray ? 1 : C)) return GF_ERR_SHAPE;
    if (V > 65535 || (ph + TH - 1) / TH > 65535) return GF_ERR_SHAPE;
    const dim3 grid((pw + TW - 1) / TW, (ph + TH - 1) / TH, V);
    hipStream_t st = gf_stream(stream);
    if (C == 1) hv_filter_kernel<1><<<grid, 256, 0, st>>>(in, tap_off, tap_w, ntaps, params, out, ph, pw, gray != 0);
    else hv_filter_kernel<3><<<grid, 256, 0, st>>>(in, tap_off, tap_w, ntaps, params, out, ph, pw, gray != 0);
    return gf_launched();
}
