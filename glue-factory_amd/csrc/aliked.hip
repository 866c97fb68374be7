// ALIKED extractor kernels (gluefactory/models/extractors/aliked.py), fp32, inference only.
//
//   gf_ak_deform_cols  column matrix of the 3x3 deformable convolutions of blocks 3 and 4 (1/8 and 1/32 resolution: small
//                      maps, one thread per (image, tap, pixel) walking the channels; the product with regular_conv.weight
//                      is the caller's GEMM)
//   gf_ak_aggregate    one thread per padded pixel holds all `dim` aggregated channels in registers: selu(conv1 x1), the
//                      three align_corners=True bilinear reads of the gated lower levels, the L2 norm, and the score
//                      head's first 1x1 layer; writes the normalised map channels-last for the crop and the 8-channel map
//   gf_ak_dkd_refine   one lane per selected keypoint: (2r+1)^2 window of the score map in registers, soft-argmax,
//                      dispersity, bilinear score at the refined position
//   gf_ak_sddh         one 256-thread workgroup per 32 keypoints.  Offsets: the K x K patch (read channels-last straight
//                      from the map) times offset_conv.0 on exact-fp32 MFMA tiles, k split over the four waves; the
//                      2M -> 2M layer on the VALU.  Then per sample position m: the 32 x dim bilinear samples are staged
//                      in LDS, sf_conv (its rows live in registers for the whole tile) and the agg_weights[m]
//                      contraction run as two MFMA stages with the SELU between them; the [dim][32] descriptor
//                      accumulators stay in registers over all M.  Nothing per sample reaches HBM.
//
// Built with -ffp-contract=off: the position arithmetic (normalise to [-1, 1], un-normalise, floor) is rounded operation by
// operation as torch rounds it; the dot products fuse explicitly (fmaf).
#include "gf_launch.h"

namespace {

constexpr float AK_SELU_ALPHA = 1.6732632423543772848170429916717f;
constexpr float AK_SELU_SCALE = 1.0507009873554804934193349852946f;
__device__ __forceinline__ float ak_selu(float x) { return AK_SELU_SCALE * (x > 0.f ? x : AK_SELU_ALPHA * expm1f(x)); }

// ------------------------------------------------------------------------------------------------ deformable im2col
__global__ __launch_bounds__(256) void ak_deform_cols_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                             float* __restrict__ cols, int C, int H, int W, int pad, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int HW = H * W;
    const int pix = (int)(t % HW);
    const int k = (int)((t / HW) % 9);
    const int b = (int)(t / ((int64_t)HW * 9));
    const int y = pix / W, xq = pix % W;
    const float py = (float)(y - pad + k / 3) + off[((int64_t)b * 18 + 2 * k) * HW + pix];
    const float px = (float)(xq - pad + k % 3) + off[((int64_t)b * 18 + 2 * k + 1) * HW + pix];
    const bool inside = py > -1.f && py < (float)H && px > -1.f && px < (float)W;
    const float fy = floorf(py), fx = floorf(px);
    const int y0 = inside ? (int)fy : 0, x0 = inside ? (int)fx : 0;
    const float ly = py - fy, lx = px - fx, hy = 1.f - ly, hx = 1.f - lx;
    const bool t0 = inside && y0 >= 0, t1 = inside && y0 + 1 <= H - 1, l0 = x0 >= 0, l1 = x0 + 1 <= W - 1;
    const float w00 = hy * hx, w01 = hy * lx, w10 = ly * hx, w11 = ly * lx;
    const float* xb = x + (int64_t)b * C * HW;
    float* cb = cols + ((int64_t)b * C * 9 + k) * HW + pix;
    for (int c = 0; c < C; ++c) {
        const float* xc = xb + (int64_t)c * HW;
        const float v00 = (t0 && l0) ? xc[y0 * W + x0] : 0.f;
        const float v01 = (t0 && l1) ? xc[y0 * W + x0 + 1] : 0.f;
        const float v10 = (t1 && l0) ? xc[(y0 + 1) * W + x0] : 0.f;
        const float v11 = (t1 && l1) ? xc[(y0 + 1) * W + x0 + 1] : 0.f;
        cb[(int64_t)c * 9 * HW] = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
    }
}

// ------------------------------------------------------------------------------------------------ aggregation
// source index pair and weight of torch's align_corners=True bilinear upsampling: src = dst (in - 1) / (out - 1)
__device__ __forceinline__ void ak_up_axis(int dst, int in, int out, int& i0, int& i1, float& l1) {
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    const float src = scale * (float)dst;
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

template <int D4>
__device__ __forceinline__ void ak_up_level(const float* __restrict__ g, int b, int h, int w, int y, int x, int Hp, int Wp, float* v) {
    int y0, y1, x0, x1;
    float ly, lx;
    ak_up_axis(y, h, Hp, y0, y1, ly);
    ak_up_axis(x, w, Wp, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const int64_t plane = (int64_t)h * w;
    const float* gb = g + (int64_t)b * D4 * plane;
#pragma unroll
    for (int c = 0; c < D4; ++c) {
        const float* gc = gb + c * plane;
        v[c] = hy * (hx * gc[y0 * w + x0] + lx * gc[y0 * w + x1]) + ly * (hx * gc[y1 * w + x0] + lx * gc[y1 * w + x1]);
    }
}

template <int C1, int D4>
__global__ __launch_bounds__(256) void ak_aggregate_kernel(const float* __restrict__ x1, const float* __restrict__ g2,
                                                           const float* __restrict__ g3, const float* __restrict__ g4,
                                                           const float* __restrict__ w1, const float* __restrict__ w8,
                                                           float* __restrict__ feat, float* __restrict__ s8, int Hp, int Wp,
                                                           int top, int left, int H, int W) {
    constexpr int DIM = 4 * D4;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z;
    if (x >= Wp || y >= Hp) return;
    const int64_t plane = (int64_t)Hp * Wp;
    float v[DIM];
    {
        float a[C1];
#pragma unroll
        for (int c = 0; c < C1; ++c) a[c] = x1[((int64_t)b * C1 + c) * plane + (int64_t)y * Wp + x];
#pragma unroll
        for (int j = 0; j < D4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < C1; ++c) s = fmaf(w1[j * C1 + c], a[c], s);
            v[j] = ak_selu(s);
        }
    }
    ak_up_level<D4>(g2, b, Hp / 2, Wp / 2, y, x, Hp, Wp, v + D4);
    ak_up_level<D4>(g3, b, Hp / 8, Wp / 8, y, x, Hp, Wp, v + 2 * D4);
    ak_up_level<D4>(g4, b, Hp / 32, Wp / 32, y, x, Hp, Wp, v + 3 * D4);
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < DIM; ++c) ss = fmaf(v[c], v[c], ss);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < DIM; ++c) s = fmaf(w8[j * DIM + c], v[c], s);
        s8[((int64_t)b * 8 + j) * plane + (int64_t)y * Wp + x] = ak_selu(s);
    }
    const int yc = y - top, xc = x - left;
    if (yc < 0 || yc >= H || xc < 0 || xc >= W) return;
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    float* f = feat + (((int64_t)b * H + yc) * W + xc) * DIM;
#pragma unroll
    for (int c = 0; c < DIM; c += 4) st4(f + c, v[c] * inv, v[c + 1] * inv, v[c + 2] * inv, v[c + 3] * inv);
}

// ------------------------------------------------------------------------------------------------ DKD refinement
// bilinear read of a single-channel map at normalised (gx, gy): grid_sample(align_corners=True, zero padding)
__device__ __forceinline__ float ak_grid_sample1(const float* __restrict__ m, int H, int W, float gx, float gy) {
    const float ix = ((gx + 1.f) / 2.f) * (float)(W - 1), iy = ((gy + 1.f) / 2.f) * (float)(H - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    if (!(fx >= -1.f && fx <= (float)W && fy >= -1.f && fy <= (float)H)) return 0.f;
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wy1 = iy - fy, wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy;
    const bool a0 = y0 >= 0 && y0 < H, a1 = y0 + 1 >= 0 && y0 + 1 < H, c0 = x0 >= 0 && x0 < W, c1 = x0 + 1 >= 0 && x0 + 1 < W;
    float out = 0.f;
    if (a0 && c0) out += m[(int64_t)y0 * W + x0] * (wx0 * wy0);
    if (a0 && c1) out += m[(int64_t)y0 * W + x0 + 1] * (wx1 * wy0);
    if (a1 && c0) out += m[(int64_t)(y0 + 1) * W + x0] * (wx0 * wy1);
    if (a1 && c1) out += m[(int64_t)(y0 + 1) * W + x0 + 1] * (wx1 * wy1);
    return out;
}

template <int R>
__global__ __launch_bounds__(256) void ak_dkd_refine_kernel(const float* __restrict__ score, const int64_t* __restrict__ idx,
                                                            float* __restrict__ kxy, float* __restrict__ kscore,
                                                            float* __restrict__ disp, int64_t total, int N, int H, int W,
                                                            float temperature) {
    constexpr int KS = 2 * R + 1;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const float* m = score + (t / N) * (int64_t)H * W;
    int64_t flat = idx[t];
    flat = flat < 0 ? 0 : (flat >= (int64_t)H * W ? (int64_t)H * W - 1 : flat);
    const int x0 = (int)(flat % W), y0 = (int)(flat / W);
    float win[KS * KS];
    float mx = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
            const int yy = y0 + dy - R, xx = x0 + dx - R;
            const float s = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? m[(int64_t)yy * W + xx] : 0.f;      // nn.Unfold pads zeros
            win[dy * KS + dx] = s;
            mx = fmaxf(mx, s);
        }
    float sum = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
            const float e = expf((win[dy * KS + dx] - mx) / temperature);
            win[dy * KS + dx] = e;
            sum += e;
            sx = fmaf(e, (float)(dx - R), sx);
            sy = fmaf(e, (float)(dy - R), sy);
        }
    const float rx = sx / sum, ry = sy / sum;
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
            const float ax = ((float)(dx - R) - rx) / (float)R, ay = ((float)(dy - R) - ry) / (float)R;
            acc = fmaf(win[dy * KS + dx], ax * ax + ay * ay, acc);
        }
    const float gx = ((float)x0 + rx) / (float)(W - 1) * 2.f - 1.f;
    const float gy = ((float)y0 + ry) / (float)(H - 1) * 2.f - 1.f;
    kxy[2 * t] = gx;
    kxy[2 * t + 1] = gy;
    disp[t] = acc / sum;
    kscore[t] = ak_grid_sample1(m, H, W, gx, gy);
}

// ------------------------------------------------------------------------------------------------ SDDH
constexpr int AK_TK = 32;      // keypoints per workgroup: the column axis of every 32x32 MFMA tile

template <int DIM, int M, int K>
__global__ __launch_bounds__(256) void ak_sddh_kernel(const float* __restrict__ feat, const float* __restrict__ pos,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      const float* __restrict__ sf, const float* __restrict__ aggT,
                                                      float* __restrict__ out, int N, int H, int W, int tiles) {
    constexpr int O = 2 * M, LD = DIM + 4, KK = K * K * DIM, RT = O / 32, WV = DIM / 32, NQ = DIM / 32;
    constexpr int MAIN = (2 * AK_TK * LD > 4 * O * 32) ? 2 * AK_TK * LD : 4 * O * 32;
    __shared__ __attribute__((aligned(16))) float s_main[MAIN];      // X [kp][LD] | F [kp][LD]; first the layer-1 partial sums
    __shared__ float s_h[O * 33];
    __shared__ float s_off[O * 33];
    __shared__ float s_px[AK_TK], s_py[AK_TK];
    float* X = s_main;
    float* Fb = s_main + AK_TK * LD;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int b = blockIdx.x / tiles, kp0 = (blockIdx.x % tiles) * AK_TK;
    const float* fb = feat + (int64_t)b * H * W * DIM;
    if (tid < AK_TK) {
        const int kp = min(kp0 + tid, N - 1);       // a short last tile repeats its last keypoint; nothing of it is stored
        s_px[tid] = pos[((int64_t)b * N + kp) * 2];
        s_py[tid] = pos[((int64_t)b * N + kp) * 2 + 1];
    }
    __syncthreads();

    // ---- offsets, layer 1: [2M][K K dim] x patch [K K dim][32 keypoints]; wave w takes the 16-deep k-steps w, w + 4, ...
    {
        const int xi = min(max((int)s_px[j], 0), W - 1), yi = min(max((int)s_py[j], 0), H - 1);      // .long() truncates
        int cx = xi, cy = yi;
        if (K > 1) {       // corner = trunc(p_int - K / 2 + 1), clamped to [0, w - 1 - K] (the reference's upper limit)
            cx = min(max((int)((float)xi - 0.5f * K + 1.f), 0), W - 1 - K);
            cy = min(max((int)((float)yi - 0.5f * K + 1.f), 0), H - 1 - K);
        }
        f32x16 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
        for (int s = wave; s < KK / 16; s += 4) {
            const int k0 = s * 16, tap = k0 / DIM, c0 = k0 % DIM;
            const Frag<float> bf = ld_frag8(fb + ((int64_t)(cy + tap / K) * W + cx + tap % K) * DIM + c0 + 8 * hi);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) mma32(acc[rt], ld_frag8(w1 + (int64_t)(rt * 32 + j) * KK + k0 + 8 * hi), bf);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) s_main[(wave * O + rt * 32 + crow(r, hi)) * 32 + j] = acc[rt][r];
    }
    __syncthreads();
    for (int i = tid; i < O * 32; i += 256) {
        const int o = i >> 5, kp = i & 31;
        const float v = ((s_main[i] + s_main[O * 32 + i]) + (s_main[2 * O * 32 + i] + s_main[3 * O * 32 + i])) + b1[o];
        s_h[o * 33 + kp] = ak_selu(v);
    }
    __syncthreads();
    // ---- offsets, layer 2 (2M -> 2M) and the clamp
    {
        const float lim = (float)max(H, W) / 4.f;
        for (int i = tid; i < O * 32; i += 256) {
            const int o = i >> 5, kp = i & 31;
            float a = 0.f;
#pragma unroll 8
            for (int k = 0; k < O; ++k) a = fmaf(w2[o * O + k], s_h[k * 33 + kp], a);
            s_off[o * 33 + kp] = fminf(fmaxf(a + b2[o], -lim), lim);
        }
    }
    // sf_conv rows wave * 32 .. + 32 stay in registers for the whole tile
    Frag<float> asf[DIM / 16];
    if (wave < WV) {
#pragma unroll
        for (int ks = 0; ks < DIM / 16; ++ks) asf[ks] = ld_frag8(sf + (int64_t)(wave * 32 + j) * DIM + ks * 16 + 8 * hi);
    }
    f32x16 dacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) dacc[r] = 0.f;
    __syncthreads();

    const int skp = tid >> 3, sub = tid & 7;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    for (int m = 0; m < M; ++m) {
        {   // the 32 x dim samples of position m: grid_sample(align_corners=True, zero padding) after the reference's round trip
            const float gx = 2.f * (s_px[skp] + s_off[m * 33 + skp]) / wm1 - 1.f;
            const float gy = 2.f * (s_py[skp] + s_off[(M + m) * 33 + skp]) / hm1 - 1.f;
            const float ix = ((gx + 1.f) / 2.f) * wm1, iy = ((gy + 1.f) / 2.f) * hm1;
            const float fx = floorf(ix), fy = floorf(iy);
            const bool near = fx >= -1.f && fx <= (float)W && fy >= -1.f && fy <= (float)H;
            const int x0 = near ? (int)fx : -2, y0 = near ? (int)fy : -2;
            const float wx1 = ix - fx, wy1 = iy - fy, wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy;
            const bool a0 = y0 >= 0 && y0 < H, a1 = y0 + 1 >= 0 && y0 + 1 < H, c0 = x0 >= 0 && x0 < W, c1 = x0 + 1 >= 0 && x0 + 1 < W;
            const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
            const float* p00 = fb + ((int64_t)y0 * W + x0) * DIM;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = (q * 8 + sub) * 4;
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                if (a0 && c0) a += *reinterpret_cast<const f32x4*>(p00 + c) * w00;
                if (a0 && c1) a += *reinterpret_cast<const f32x4*>(p00 + DIM + c) * w01;
                if (a1 && c0) a += *reinterpret_cast<const f32x4*>(p00 + (int64_t)W * DIM + c) * w10;
                if (a1 && c1) a += *reinterpret_cast<const f32x4*>(p00 + (int64_t)W * DIM + DIM + c) * w11;
                *reinterpret_cast<f32x4*>(X + skp * LD + c) = a;
            }
        }
        __syncthreads();
        if (wave < WV) {      // F [c'][kp] = selu(sf_conv X)
            f32x16 f;
#pragma unroll
            for (int r = 0; r < 16; ++r) f[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < DIM / 16; ++ks) mma32(f, asf[ks], ld_frag8(X + j * LD + ks * 16 + 8 * hi));
#pragma unroll
            for (int r = 0; r < 16; ++r) Fb[j * LD + wave * 32 + crow(r, hi)] = ak_selu(f[r]);
        }
        __syncthreads();
        if (wave < WV) {      // descriptor [d][kp] += agg_weights[m][c'][d] F [c'][kp]
            const float* am = aggT + ((int64_t)m * DIM + wave * 32 + j) * DIM + 8 * hi;
#pragma unroll
            for (int ks = 0; ks < DIM / 16; ++ks) mma32(dacc, ld_frag8(am + ks * 16), ld_frag8(Fb + j * LD + ks * 16 + 8 * hi));
        }
    }
    // ---- L2 normalisation over d and the store (X was last read before the barrier in front of the final MFMA stage)
    if (wave < WV) {
#pragma unroll
        for (int r = 0; r < 16; ++r) X[j * LD + wave * 32 + crow(r, hi)] = dacc[r];
    }
    __syncthreads();
    float ss = 0.f;
    f32x4 d[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        d[q] = *reinterpret_cast<const f32x4*>(X + skp * LD + (q * 8 + sub) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(d[q][e], d[q][e], ss);
    }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    ss += __shfl_xor(ss, 4);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    if (kp0 + skp < N) {
        float* o = out + ((int64_t)b * N + kp0 + skp) * DIM;
#pragma unroll
        for (int q = 0; q < NQ; ++q) *reinterpret_cast<f32x4*>(o + (q * 8 + sub) * 4) = d[q] * inv;
    }
}

template <int DIM, int M, int K>
int ak_sddh_launch(const float* feat, const float* pos, const float* w1, const float* b1, const float* w2, const float* b2,
                   const float* sf, const float* aggT, float* out, int B, int N, int H, int W, hipStream_t st) {
    const int tiles = (N + AK_TK - 1) / AK_TK;
    ak_sddh_kernel<DIM, M, K><<<dim3((unsigned)(B * tiles)), 256, 0, st>>>(feat, pos, w1, b1, w2, b2, sf, aggT, out, N, H, W, tiles);
    return gf_launched();
}

}  // namespace

extern "C" int gf_ak_deform_cols(const float* x, const float* offset, float* cols, int B, int C, int H, int W, int pad, void* stream) {
    if (!x || !offset || !cols) return GF_ERR_SHAPE;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || pad < 0) return GF_ERR_SHAPE;
    if ((int64_t)H * W >= (1 << 24)) return GF_ERR_UNSUPPORTED;      // pixel coordinates are exact floats
    const int64_t total = (int64_t)B * 9 * H * W;
    ak_deform_cols_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, gf_stream(stream)>>>(x, offset, cols, C, H, W, pad, total);
    return gf_launched();
}

extern "C" int gf_ak_aggregate(const float* x1, const float* g2, const float* g3, const float* g4, const float* w1, const float* w8,
                               float* feat, float* s8, int B, int c1, int dim, int Hp, int Wp, int top, int left, int H, int W,
                               void* stream) {
    if (!x1 || !g2 || !g3 || !g4 || !w1 || !w8 || !feat || !s8) return GF_ERR_SHAPE;
    if (B <= 0 || Hp <= 0 || Wp <= 0 || H <= 0 || W <= 0 || Hp % 32 || Wp % 32) return GF_ERR_SHAPE;
    if (top < 0 || left < 0 || top + H > Hp || left + W > Wp || B > 65535 || Hp / 4 > 65535) return GF_ERR_SHAPE;
    if (!gf_aligned16(feat)) return GF_ERR_ALIGN;
    const dim3 grid((Wp + 63) / 64, Hp / 4, B);
    if (c1 == 8 && dim == 64)
        ak_aggregate_kernel<8, 16><<<grid, 256, 0, gf_stream(stream)>>>(x1, g2, g3, g4, w1, w8, feat, s8, Hp, Wp, top, left, H, W);
    else if (c1 == 16 && dim == 128)
        ak_aggregate_kernel<16, 32><<<grid, 256, 0, gf_stream(stream)>>>(x1, g2, g3, g4, w1, w8, feat, s8, Hp, Wp, top, left, H, W);
    else
        return GF_ERR_UNSUPPORTED;
    return gf_launched();
}

extern "C" int gf_ak_dkd_refine(const float* score, const int64_t* idx, float* kxy, float* kscore, float* disp, int B, int N, int H,
                                int W, int radius, float temperature, void* stream) {
    if (B <= 0 || N < 0 || H < 2 || W < 2 || !(temperature > 0.f)) return GF_ERR_SHAPE;
    if (radius < 1 || radius > 4) return GF_ERR_UNSUPPORTED;       // the window lives in registers: at most 9 x 9
    if (!score || (N > 0 && (!idx || !kxy || !kscore || !disp))) return GF_ERR_SHAPE;      // (empty tensors have no storage)
    if (N == 0) return 0;
    const int64_t total = (int64_t)B * N;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t st = gf_stream(stream);
    switch (radius) {
        case 1: ak_dkd_refine_kernel<1><<<grid, 256, 0, st>>>(score, idx, kxy, kscore, disp, total, N, H, W, temperature); break;
        case 2: ak_dkd_refine_kernel<2><<<grid, 256, 0, st>>>(score, idx, kxy, kscore, disp, total, N, H, W, temperature); break;
        case 3: ak_dkd_refine_kernel<3><<<grid, 256, 0, st>>>(score, idx, kxy, kscore, disp, total, N, H, W, temperature); break;
        default: ak_dkd_refine_kernel<4><<<grid, 256, 0, st>>>(score, idx, kxy, kscore, disp, total, N, H, W, temperature); break;
    }
    return gf_launched();
}

extern "C" int gf_ak_sddh(const float* feat, const float* pos, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* sf, const float* aggT, float* out, int B, int N, int H, int W, int dim, int M, int K,
                          void* stream) {
    if (!feat || !w1 || !b1 || !w2 || !b2 || !sf || !aggT || (N > 0 && (!pos || !out))) return GF_ERR_SHAPE;   // (empty tensors have no storage)
    if (B <= 0 || N < 0 || H <= 0 || W <= 0) return GF_ERR_SHAPE;
    if ((dim != 64 && dim != 128) || (M != 16 && M != 32) || (K != 1 && K != 3)) return GF_ERR_UNSUPPORTED;
    if (H < K + 1 || W < K + 1) return GF_ERR_SHAPE;                 // the patch corner is clamped to [0, w - 1 - K]
    if (!gf_aligned16(feat, w1, sf, aggT, out)) return GF_ERR_ALIGN;
    if (N == 0) return 0;
    if ((int64_t)B * ((N + AK_TK - 1) / AK_TK) >= (1ll << 31)) return GF_ERR_SHAPE;
    hipStream_t st = gf_stream(stream);
#define AK_SDDH_CASE(D_, M_, K_) \
    if (dim == D_ && M == M_ && K == K_) return ak_sddh_launch<D_, M_, K_>(feat, pos, w1, b1, w2, b2, sf, aggT, out, B, N, H, W, st);
    AK_SDDH_CASE(64, 16, 1) AK_SDDH_CASE(64, 16, 3) AK_SDDH_CASE(64, 32, 1) AK_SDDH_CASE(64, 32, 3)
    AK_SDDH_CASE(128, 16, 1) AK_SDDH_CASE(128, 16, 3) AK_SDDH_CASE(128, 32, 1) AK_SDDH_CASE(128, 32, 3)
#undef AK_SDDH_CASE
    return GF_ERR_UNSUPPORTED;
}
