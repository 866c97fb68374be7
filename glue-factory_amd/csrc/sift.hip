// SIFT extractor kernels (glue_factory_amd/extractors/sift.py states the semantics; contracts in include/gf_amd.h).
// All fp32, no gradient.  Built with -ffp-contract=off: the threshold tests round operation by operation, as the stock
// path's torch ops do; the accumulation loops fuse explicitly (fmaf).
//
//   gf_sift_blur      one Gaussian level per launch: the source tile with its halo (read through the 2x bilinear
//                     upsampling or the every-second-pixel rule of an octave base) -> LDS, row pass LDS -> LDS, column
//                     pass out of LDS; writes the level and the DoG level (level - source).  Tile 64 x 32, halo <= 16:
//                     24.3 + 16 KiB of LDS per workgroup, so 3 workgroups share a CU's 160 KiB.
//   gf_sift_extrema   count / scan / write: every thread tests one DoG cell (26 neighbours, refinement, thresholds); a
//                     workgroup owns 256 consecutive cells, the scan turns the per-workgroup counts into list offsets,
//                     so the list is in cell order without an atomic and equal bit for bit across calls.
//   gf_sift_orient    one wave per keypoint: 64 window pixels per step; lane k < 36 owns bin k and adds the step's pixels
//                     in pixel order (values pass through v_readlane), so the sum order is fixed.
//   gf_sift_describe  one wave per keypoint, lane l owns bins 2l, 2l + 1 (cell l / 4); same fixed-order rule; both
//                     normalisations, the clip and RootSIFT on the registers.
//   gf_sift_dedupe    filter_dog_point's first two steps: atomicMax of (score bits, ~|angle| bits) per pixel.
#include <math.h>

#include "gf_launch.h"

namespace {

constexpr int SB_TW = 64, SB_TH = 32, SB_RMAX = 16;
constexpr int SIFT_LEVELS = 6, SIFT_LAYERS = 3, SIFT_MAX_OCT = 8;
constexpr float SIFT_2PI = 6.283185307179586f;

struct SiftTaps { float w[SB_RMAX + 1]; };
struct SiftGeom { const float* base[SIFT_MAX_OCT]; int h[SIFT_MAX_OCT]; int w[SIFT_MAX_OCT]; };

__device__ __forceinline__ int reflect101(int i, int n) {
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// value of the blur's source at (y, x) of the OUTPUT grid
template <int MODE> __device__ __forceinline__ float sift_src(const float* __restrict__ src, int Hs, int Ws, int y, int x) {
    if (MODE == 0) return src[(int64_t)y * Ws + x];
    if (MODE == 2) return src[(int64_t)(2 * y) * Ws + 2 * x];
    // 2x bilinear, align_corners=False: source coordinate 0.5 (u + 0.5) - 0.5, clamped at 0
    const float fy = fmaxf(0.5f * ((float)y + 0.5f) - 0.5f, 0.f), fx = fmaxf(0.5f * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = min(y0 + 1, Hs - 1), x1 = min(x0 + 1, Ws - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float* r0 = src + (int64_t)y0 * Ws;
    const float* r1 = src + (int64_t)y1 * Ws;
    return (1.f - ly) * ((1.f - lx) * r0[x0] + lx * r0[x1]) + ly * ((1.f - lx) * r1[x0] + lx * r1[x1]);
}

template <int MODE>
__global__ __launch_bounds__(256) void sift_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ dog,
                                                        float* __restrict__ src_copy, int Hs, int Ws, int H, int W, int64_t sbs,
                                                        int64_t obs, int64_t gbs, int R, SiftTaps taps) {
    __shared__ float in[SB_TH + 2 * SB_RMAX][SB_TW + 2 * SB_RMAX + 1];
    __shared__ float mid[SB_TH + 2 * SB_RMAX][SB_TW];
    const int tid = threadIdx.x, x0 = blockIdx.x * SB_TW, y0 = blockIdx.y * SB_TH, b = blockIdx.z;
    src += (int64_t)b * sbs;
    const int rows = SB_TH + 2 * R, cols = SB_TW + 2 * R;
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        in[r][c] = sift_src<MODE>(src, Hs, Ws, reflect101(y0 - R + r, H), reflect101(x0 - R + c, W));
    }
    __syncthreads();
    for (int i = tid; i < rows * SB_TW; i += 256) {
        const int r = i >> 6, c = (i & 63) + R;
        float acc = taps.w[0] * in[r][c];
        for (int k = 1; k <= R; ++k) acc = fmaf(taps.w[k], in[r][c - k] + in[r][c + k], acc);
        mid[r][i & 63] = acc;
    }
    __syncthreads();
    for (int i = tid; i < SB_TH * SB_TW; i += 256) {
        const int r = (i >> 6) + R, c = i & 63;
        const int y = y0 + (i >> 6), x = x0 + c;
        if (y >= H || x >= W) continue;
        float acc = taps.w[0] * mid[r][c];
        for (int k = 1; k <= R; ++k) acc = fmaf(taps.w[k], mid[r - k][c] + mid[r + k][c], acc);
        const int64_t o = (int64_t)y * W + x;
        const float centre = in[r][c + R];
        dst[(int64_t)b * obs + o] = acc;
        if (dog) dog[(int64_t)b * gbs + o] = acc - centre;
        if (src_copy) src_copy[(int64_t)b * obs + o] = centre;
    }
}

// ------------------------------------------------------------------------------------------------ extrema
struct SiftThr { float thr08, thr, er, er2; };

// D: one image's [5, h, w] DoG stack; (s, y, x) the cell, 1 <= s <= 3, 1 <= y <= h - 2, 1 <= x <= w - 2.
__device__ bool sift_candidate(const float* __restrict__ D, int h, int w, int& s, int& y, int& x, const SiftThr t, float* out) {
    const int64_t hw = (int64_t)h * w;
    const float* p = D + s * hw + (int64_t)y * w + x;
    float v = *p;
    if (!(fabsf(v) > t.thr08)) return false;
    float nmax = -INFINITY, nmin = INFINITY;
    for (int ds = -1; ds <= 1; ++ds)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (ds == 0 && dy == 0 && dx == 0) continue;
                const float n = p[ds * hw + dy * w + dx];
                nmax = fmaxf(nmax, n);
                nmin = fminf(nmin, n);
            }
    if (!(v > nmax || v < nmin)) return false;
    for (int it = 0; it < 5; ++it) {
        p = D + s * hw + (int64_t)y * w + x;
        v = *p;
        const float xm = p[-1], xp = p[1], ym = p[-w], yp = p[w], sm = p[-hw], sp = p[hw];
        const float gx = 0.5f * (xp - xm), gy = 0.5f * (yp - ym), gs = 0.5f * (sp - sm);
        const float a = xp + xm - 2.f * v, e = yp + ym - 2.f * v, i9 = sp + sm - 2.f * v;
        const float bq = 0.25f * (p[w + 1] - p[w - 1] - p[-w + 1] + p[-w - 1]);
        const float c = 0.25f * (p[hw + 1] - p[hw - 1] - p[-hw + 1] + p[-hw - 1]);
        const float f = 0.25f * (p[hw + w] - p[hw - w] - p[-hw + w] + p[-hw - w]);
        const float c00 = e * i9 - f * f, c01 = c * f - bq * i9, c02 = bq * f - c * e;
        const float c11 = a * i9 - c * c, c12 = bq * c - a * f, c22 = a * e - bq * bq;
        const float det = a * c00 + bq * c01 + c * c02;
        if (!(det != 0.f)) return false;
        const float inv = 1.0f / det;
        const float ox = -(c00 * gx + c01 * gy + c02 * gs) * inv, oy = -(c01 * gx + c11 * gy + c12 * gs) * inv,
                    os = -(c02 * gx + c12 * gy + c22 * gs) * inv;
        const int mx = (ox > 0.5f) - (ox < -0.5f), my = (oy > 0.5f) - (oy < -0.5f), ms = (os > 0.5f) - (os < -0.5f);
        if (mx == 0 && my == 0 && ms == 0) {
            const float dhat = v + 0.5f * (gx * ox + gy * oy + gs * os);
            const float tr = a + e, d2 = a * e - bq * bq;
            if (!(fabsf(dhat) >= t.thr) || !(d2 > 0.f) || !(tr * tr * t.er < t.er2 * d2)) return false;
            out[0] = ox; out[1] = oy; out[2] = os; out[3] = dhat;
            return true;
        }
        x += mx; y += my; s += ms;
        if (s < 1 || s > SIFT_LAYERS || y < 1 || y > h - 2 || x < 1 || x > w - 2) return false;
    }
    return false;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ dog, int h, int w, int octave, SiftThr t, int nblk,
                                                           int* __restrict__ ws, int* __restrict__ meta, float* __restrict__ vals, int cap) {
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int64_t cell = (int64_t)blockIdx.x * 256 + tid;
    const int iw = w - 2, ih = h - 2;
    bool keep = false;
    int s = 0, y = 0, x = 0;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    if (cell < (int64_t)SIFT_LAYERS * ih * iw) {
        s = (int)(cell / ((int64_t)ih * iw)) + 1;
        const int rem = (int)(cell % ((int64_t)ih * iw));
        y = rem / iw + 1;
        x = rem % iw + 1;
        keep = sift_candidate(dog + (int64_t)b * 5 * h * w, h, w, s, y, x, t, out);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) ws[(int64_t)b * nblk + blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        return;
    }
    if (!keep) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) rank += wcnt[k];
    const int64_t slot = (int64_t)ws[(int64_t)b * nblk + blockIdx.x] + rank;
    if (slot >= cap) return;
    int* mp = meta + ((int64_t)b * cap + slot) * 4;
    float* vp = vals + ((int64_t)b * cap + slot) * 4;
    mp[0] = octave; mp[1] = s; mp[2] = y; mp[3] = x;
    vp[0] = out[0]; vp[1] = out[1]; vp[2] = out[2]; vp[3] = out[3];
}

// per image: ws[blk] (counts) -> list offsets count[b] + exclusive prefix; count[b] += total (keeps counting past cap)
__global__ __launch_bounds__(256) void sift_extrema_scan_kernel(int* __restrict__ ws, int* __restrict__ count, int nblk) {
    __shared__ int sh[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    int* p = ws + (int64_t)b * nblk;
    int carry = count[b];
    for (int base = 0; base < nblk; base += 256) {
        const int v = base + tid < nblk ? p[base + tid] : 0;
        sh[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (base + tid < nblk) p[base + tid] = carry + sh[tid] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (tid == 0) count[b] = carry;
}

// ------------------------------------------------------------------------------------------------ per-keypoint kernels
__device__ __forceinline__ float lane_value(float v, int q) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), q));
}

// gradient of level L at (yy, xx), central differences; false when the pixel is less than 1 px inside
__device__ __forceinline__ bool sift_gradient(const float* __restrict__ L, int h, int w, int yy, int xx, float& gx, float& gy) {
    if (yy < 1 || yy > h - 2 || xx < 1 || xx > w - 2) return false;
    const float* p = L + (int64_t)yy * w + xx;
    gx = p[1] - p[-1];
    gy = p[w] - p[-w];
    return true;
}

struct SiftKp { const float* L; int h, w; bool ok; };

__device__ __forceinline__ SiftKp sift_level(const SiftGeom& g, int noct, int N, int64_t kp, const int* oct, const int* lvl, float sigma) {
    SiftKp r{nullptr, 0, 0, false};
    const int o = oct[kp];
    if (o < 0 || o >= noct || !(sigma > 0.f && sigma <= 16.f)) return r;
    const int l = min(max(lvl[kp], 0), SIFT_LEVELS - 1);
    r.h = g.h[o]; r.w = g.w[o];
    r.L = g.base[o] + ((kp / N) * SIFT_LEVELS + l) * (int64_t)r.h * r.w;
    r.ok = true;
    return r;
}

__global__ __launch_bounds__(256) void sift_orient_kernel(SiftGeom g, int noct, const int* __restrict__ oct, const int* __restrict__ lvl,
                                                          const int* __restrict__ xi, const int* __restrict__ yi,
                                                          const float* __restrict__ sigma, float* __restrict__ ori, int* __restrict__ valid,
                                                          int64_t total, int N) {
    const int lane = threadIdx.x & 63;
    const int64_t kp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (kp >= total) return;
    const float sg = sigma[kp];
    const SiftKp K = sift_level(g, noct, N, kp, oct, lvl, sg);
    const int cx = xi[kp], cy = yi[kp];
    if (!K.ok || cx < 0 || cx >= K.w || cy < 0 || cy >= K.h) {
        if (lane < 2) { ori[kp * 2 + lane] = 0.f; valid[kp * 2 + lane] = 0; }
        return;
    }
    const float sw = 1.5f * sg;
    const int rad = (int)rintf(3.0f * sw), side = 2 * rad + 1, P = side * side;
    const float den = 2.0f * sw * sw;
    float hist = 0.f;
    for (int base = 0; base < P; base += 64) {
        const int p = base + lane;
        float fb = 0.f, wv = 0.f, gx, gy;
        if (p < P) {
            const int j = p / side - rad, i = p % side - rad;
            if (sift_gradient(K.L, K.h, K.w, cy + j, cx + i, gx, gy)) {
                wv = expf(-(float)(i * i + j * j) / den) * sqrtf(gx * gx + gy * gy);
                fb = atan2f(gy, gx) * (float)(36.0 / (2.0 * M_PI));
                if (fb < 0.f) fb += 36.f;
            }
        }
        const int nq = min(64, P - base);
        for (int q = 0; q < nq; ++q) {
            const float wq = lane_value(wv, q);
            if (wq == 0.f) continue;
            float d = fabsf(lane_value(fb, q) - (float)lane);
            d = fminf(d, 36.f - d);
            hist = fmaf(wq, fmaxf(0.f, 1.f - d), hist);
        }
    }
    const int ll = lane < 36 ? (lane + 35) % 36 : lane, lr = lane < 36 ? (lane + 1) % 36 : lane;
    for (int it = 0; it < 6; ++it) hist = (__shfl(hist, ll) + hist + __shfl(hist, lr)) / 3.0f;
    const float left = __shfl(hist, ll), right = __shfl(hist, lr);
    const float mx = wave_allmax(lane < 36 ? hist : -INFINITY);
    float val = (lane < 36 && hist > left && hist > right && hist >= 0.8f * mx) ? hist : -1.0f;
    for (int k = 0; k < 2; ++k) {
        const float top = wave_allmax(val);
        const unsigned long long m = __ballot(val == top && lane < 36);
        const int first = m ? __ffsll((long long)m) - 1 : 0;
        const bool ok = top > 0.f;
        if (lane == first) {
            float th = 0.f;
            if (ok) {
                const float dd = 0.5f * (left - right) / (left - 2.f * hist + right);
                th = ((float)lane + dd) * (float)(2.0 * M_PI / 36.0);
                if (th < 0.f) th += SIFT_2PI;
                if (th >= SIFT_2PI) th -= SIFT_2PI;
            }
            ori[kp * 2 + k] = th;
            valid[kp * 2 + k] = ok ? 1 : 0;
            val = -1.0f;
        }
    }
}

__global__ __launch_bounds__(256) void sift_describe_kernel(SiftGeom g, int noct, const int* __restrict__ oct, const int* __restrict__ lvl,
                                                            const float* __restrict__ xo, const float* __restrict__ yo,
                                                            const float* __restrict__ sigma, const float* __restrict__ ori,
                                                            float* __restrict__ desc, int64_t total, int N, int rootsift) {
    const int lane = threadIdx.x & 63;
    const int64_t kp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (kp >= total) return;
    const float sg = sigma[kp];
    const SiftKp K = sift_level(g, noct, N, kp, oct, lvl, sg);
    const float px = xo[kp], py = yo[kp], th0 = ori[kp];
    f32x2* outp = reinterpret_cast<f32x2*>(desc + kp * 128) + lane;
    if (!K.ok || !(px >= 0.f && px < (float)K.w && py >= 0.f && py < (float)K.h)) {
        *outp = f32x2{0.f, 0.f};
        return;
    }
    const float hw = 3.0f * sg;
    const int rad = (int)rintf(hw * (float)(M_SQRT2 * 2.5)), side = 2 * rad + 1, P = side * side;
    const int cx = (int)rintf(px), cy = (int)rintf(py);
    const float cs = cosf(th0), sn = sinf(th0);
    const float myr = (float)(lane >> 4), myc = (float)((lane >> 2) & 3), myo = (float)((lane & 3) * 2);
    float b0 = 0.f, b1 = 0.f;
    for (int base = 0; base < P; base += 64) {
        const int p = base + lane;
        float rb = 0.f, cb = 0.f, ob = 0.f, wv = 0.f, gx, gy;
        if (p < P) {
            const int j = p / side - rad, i = p % side - rad;
            if (sift_gradient(K.L, K.h, K.w, cy + j, cx + i, gx, gy)) {
                const float dxp = (float)(cx + i) - px, dyp = (float)(cy + j) - py;
                const float rx = (cs * dxp + sn * dyp) / hw, ry = (-sn * dxp + cs * dyp) / hw;
                cb = rx + 1.5f;
                rb = ry + 1.5f;
                if (rb > -1.f && rb < 4.f && cb > -1.f && cb < 4.f) {
                    wv = expf(-(rx * rx + ry * ry) / 8.0f) * sqrtf(gx * gx + gy * gy);
                    ob = (atan2f(gy, gx) - th0) * (float)(8.0 / (2.0 * M_PI));
                    ob = ob - floorf(ob / 8.0f) * 8.0f;
                }
            }
        }
        const int nq = min(64, P - base);
        for (int q = 0; q < nq; ++q) {
            const float wq = lane_value(wv, q);
            if (wq == 0.f) continue;
            const float wr = fmaxf(0.f, 1.f - fabsf(lane_value(rb, q) - myr));
            const float wc = fmaxf(0.f, 1.f - fabsf(lane_value(cb, q) - myc));
            const float t = wq * wr * wc;
            const float o = lane_value(ob, q);
            float d0 = fabsf(o - myo), d1 = fabsf(o - (myo + 1.f));
            d0 = fminf(d0, 8.f - d0);
            d1 = fminf(d1, 8.f - d1);
            b0 = fmaf(t, fmaxf(0.f, 1.f - d0), b0);
            b1 = fmaf(t, fmaxf(0.f, 1.f - d1), b1);
        }
    }
    float nrm = fmaxf(sqrtf(wave_allsum(b0 * b0 + b1 * b1)), 1e-12f);
    b0 = fminf(b0 / nrm, 0.2f);
    b1 = fminf(b1 / nrm, 0.2f);
    nrm = fmaxf(sqrtf(wave_allsum(b0 * b0 + b1 * b1)), 1e-12f);
    b0 /= nrm;
    b1 /= nrm;
    if (rootsift) {
        const float l1 = fmaxf(wave_allsum(fabsf(b0) + fabsf(b1)), 1e-6f);
        b0 = sqrtf(fmaxf(b0 / l1, 1e-6f));
        b1 = sqrtf(fmaxf(b1 / l1, 1e-6f));
        nrm = fmaxf(sqrtf(wave_allsum(b0 * b0 + b1 * b1)), 1e-6f);
        b0 /= nrm;
        b1 /= nrm;
    }
    *outp = f32x2{b0, b1};
}

// ------------------------------------------------------------------------------------------------ dedupe
__device__ __forceinline__ unsigned long long sift_key(float score, float angle) {
    return ((unsigned long long)__float_as_uint(score + 0.f) << 32) | (unsigned long long)(0xFFFFFFFFu - __float_as_uint(fabsf(angle)));
}
__global__ void sift_dedupe_clear_kernel(unsigned long long* __restrict__ buf, float* __restrict__ sbuf, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { buf[i] = 0ull; sbuf[i] = 0.f; }
}
template <bool MARK>
__global__ void sift_dedupe_kernel(const int* __restrict__ ix, const int* __restrict__ iy, const float* __restrict__ score,
                                   const float* __restrict__ angle, const int* __restrict__ valid, unsigned long long* __restrict__ buf,
                                   float* __restrict__ sbuf, int* __restrict__ keep, int64_t total, int N, int H, int W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = ix[i], y = iy[i];
    const float s = score[i];
    const bool ok = valid[i] != 0 && x >= 0 && x < W && y >= 0 && y < H && s >= 0.f;
    if (!ok) {
        if (MARK) keep[i] = 0;
        return;
    }
    const int64_t pix = ((i / N) * H + y) * (int64_t)W + x;
    const unsigned long long key = sift_key(s, angle[i]);
    if (!MARK) {
        atomicMax(buf + pix, key);
    } else {
        const bool k = buf[pix] == key;
        keep[i] = k ? 1 : 0;
        if (k) sbuf[pix] = s + 0.f;
    }
}

}  // namespace

extern "C" int gf_sift_blur(const float* src, float* dst, float* dog, float* src_copy, int B, int Hs, int Ws, int H, int W,
                            int64_t src_bstride, int64_t out_bstride, int64_t dog_bstride, int mode, double sigma, void* stream) {
    if (!src || !dst || B <= 0 || Hs < 2 || Ws < 2 || H < 2 || W < 2 || !(sigma > 0.0)) return GF_ERR_SHAPE;
    if (B > 65535 || (H + SB_TH - 1) / SB_TH > 65535) return GF_ERR_SHAPE;
    if (mode == 0 ? (H != Hs || W != Ws) : mode == 1 ? (H != 2 * Hs || W != 2 * Ws || dog) : mode == 2 ? (H != (Hs + 1) / 2 || W != (Ws + 1) / 2) : true)
        return GF_ERR_SHAPE;
    if (src_bstride < (int64_t)Hs * Ws || out_bstride < (int64_t)H * W || (dog && dog_bstride < (int64_t)H * W)) return GF_ERR_SHAPE;
    const int R = (int)ceil(4.0 * sigma);
    if (R > SB_RMAX) return GF_ERR_UNSUPPORTED;
    double k[SB_RMAX + 1], sum = 0.0;
    for (int i = 0; i <= R; ++i) {
        k[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma));
        sum += i ? 2.0 * k[i] : k[i];
    }
    SiftTaps taps{};
    for (int i = 0; i <= R; ++i) taps.w[i] = (float)(k[i] / sum);
    const dim3 grid((unsigned)((W + SB_TW - 1) / SB_TW), (unsigned)((H + SB_TH - 1) / SB_TH), (unsigned)B);
    hipStream_t st = gf_stream(stream);
    if (mode == 0)
        sift_blur_kernel<0><<<grid, 256, 0, st>>>(src, dst, dog, src_copy, Hs, Ws, H, W, src_bstride, out_bstride, dog_bstride, R, taps);
    else if (mode == 1)
        sift_blur_kernel<1><<<grid, 256, 0, st>>>(src, dst, dog, src_copy, Hs, Ws, H, W, src_bstride, out_bstride, dog_bstride, R, taps);
    else
        sift_blur_kernel<2><<<grid, 256, 0, st>>>(src, dst, dog, src_copy, Hs, Ws, H, W, src_bstride, out_bstride, dog_bstride, R, taps);
    return gf_launched();
}

static inline int64_t sift_extrema_blocks(int H, int W) { return ((int64_t)SIFT_LAYERS * (H - 2) * (W - 2) + 255) / 256; }

extern "C" int64_t gf_sift_extrema_ws_ints(int B, int H, int W) {
    if (B <= 0 || H < 3 || W < 3) return 0;
    return (int64_t)B * sift_extrema_blocks(H, W);
}

extern "C" int gf_sift_extrema(const float* dog, int B, int H, int W, int octave, double thr, double edge_r, int* ws, int* count, int* meta,
                               float* vals, int cap, void* stream) {
    if (!dog || !ws || !count || B <= 0 || H < 3 || W < 3 || cap < 0 || octave < 0 || octave >= SIFT_MAX_OCT) return GF_ERR_SHAPE;
    if (cap > 0 && (!meta || !vals)) return GF_ERR_SHAPE;
    if (!(thr >= 0.0) || !(edge_r > 0.0) || B > 65535) return GF_ERR_SHAPE;
    const int64_t nblk = sift_extrema_blocks(H, W);
    if (nblk >= (1ll << 31) || (int64_t)5 * H * W >= (1ll << 31)) return GF_ERR_UNSUPPORTED;
    const SiftThr t{(float)(0.8 * thr), (float)thr, (float)edge_r, (float)((edge_r + 1.0) * (edge_r + 1.0))};
    hipStream_t st = gf_stream(stream);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    sift_extrema_kernel<false><<<grid, 256, 0, st>>>(dog, H, W, octave, t, (int)nblk, ws, meta, vals, cap);
    sift_extrema_scan_kernel<<<dim3((unsigned)B), 256, 0, st>>>(ws, count, (int)nblk);
    sift_extrema_kernel<true><<<grid, 256, 0, st>>>(dog, H, W, octave, t, (int)nblk, ws, meta, vals, cap);
    return gf_launched();
}

static int sift_geom(SiftGeom& g, const void* const* levels, const int* hw, int noct) {
    if (!levels || !hw || noct <= 0 || noct > SIFT_MAX_OCT) return GF_ERR_SHAPE;
    for (int o = 0; o < noct; ++o) {
        if (!levels[o] || hw[2 * o] < 3 || hw[2 * o + 1] < 3) return GF_ERR_SHAPE;
        g.base[o] = (const float*)levels[o];
        g.h[o] = hw[2 * o];
        g.w[o] = hw[2 * o + 1];
    }
    return 0;
}

extern "C" int gf_sift_orient(const void* const* levels, const int* hw, int noct, const int* oct, const int* lvl, const int* xi,
                              const int* yi, const float* sigma, float* ori, int* valid, int B, int N, void* stream) {
    SiftGeom g{};
    if (int e = sift_geom(g, levels, hw, noct)) return e;
    if (B <= 0 || N < 0) return GF_ERR_SHAPE;
    if (N == 0) return 0;
    if (!oct || !lvl || !xi || !yi || !sigma || !ori || !valid) return GF_ERR_SHAPE;
    const int64_t total = (int64_t)B * N;
    if ((total + 3) / 4 >= (1ll << 31)) return GF_ERR_SHAPE;
    sift_orient_kernel<<<dim3((unsigned)((total + 3) / 4)), 256, 0, gf_stream(stream)>>>(g, noct, oct, lvl, xi, yi, sigma, ori, valid, total, N);
    return gf_launched();
}

extern "C" int gf_sift_describe(const void* const* levels, const int* hw, int noct, const int* oct, const int* lvl, const float* xo,
                                const float* yo, const float* sigma, const float* ori, float* desc, int B, int N, int rootsift,
                                void* stream) {
    SiftGeom g{};
    if (int e = sift_geom(g, levels, hw, noct)) return e;
    if (B <= 0 || N < 0) return GF_ERR_SHAPE;
    if (N == 0) return 0;
    if (!oct || !lvl || !xo || !yo || !sigma || !ori || !desc) return GF_ERR_SHAPE;
    if (((uintptr_t)desc & 7) != 0) return GF_ERR_ALIGN;
    const int64_t total = (int64_t)B * N;
    if ((total + 3) / 4 >= (1ll << 31)) return GF_ERR_SHAPE;
    sift_describe_kernel<<<dim3((unsigned)((total + 3) / 4)), 256, 0, gf_stream(stream)>>>(g, noct, oct, lvl, xo, yo, sigma, ori, desc, total, N,
                                                                                          rootsift ? 1 : 0);
    return gf_launched();
}

extern "C" int gf_sift_dedupe(const int* ix, const int* iy, const float* score, const float* angle, const int* valid, void* buf, float* sbuf,
                              int* keep, int B, int N, int H, int W, void* stream) {
    if (B <= 0 || N < 0 || H <= 0 || W <= 0 || !buf || !sbuf) return GF_ERR_SHAPE;
    if (((uintptr_t)buf & 7) != 0) return GF_ERR_ALIGN;
    const int64_t pixels = (int64_t)B * H * W, total = (int64_t)B * N;
    if ((pixels + 255) / 256 >= (1ll << 31) || (total + 255) / 256 >= (1ll << 31)) return GF_ERR_SHAPE;
    hipStream_t st = gf_stream(stream);
    unsigned long long* b64 = (unsigned long long*)buf;
    sift_dedupe_clear_kernel<<<dim3((unsigned)((pixels + 255) / 256)), 256, 0, st>>>(b64, sbuf, pixels);
    if (N == 0) return gf_launched();
    if (!ix || !iy || !score || !angle || !valid || !keep) return GF_ERR_SHAPE;
    const dim3 grid((unsigned)((total + 255) / 256));
    sift_dedupe_kernel<false><<<grid, 256, 0, st>>>(ix, iy, score, angle, valid, b64, sbuf, keep, total, N, H, W);
    sift_dedupe_kernel<true><<<grid, 256, 0, st>>>(ix, iy, score, angle, valid, b64, sbuf, keep, total, N, H, W);
    return gf_launched();
}
