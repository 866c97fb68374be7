// Skeleton shared by the kernels that stream S = a b^T through MFMA tiles (assignment.hip, nn_match.hip): one workgroup =
// 4 waves owns 128 rows of the "owner" matrix (fragments kept in registers: D/16 k-steps) and streams the other matrix
// through LDS in 64-row tiles; the tile is computed as C[tile_row][owner], so every reduction over the streamed axis is
// lane-local (see gf_common.h and the header of assignment.hip).
#pragma once
#include "gf_launch.h"

namespace {

template <typename T, int D> struct ALay {
    static constexpr int VEC = 16 / sizeof(T);
    static constexpr int CPR = D / VEC;
    static constexpr int LDR = D + VEC;
    static constexpr int TILE = 64 * LDR;  // elements
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Double-buffered stream of 64-row tiles [s_begin, s_end) of the streamed matrix through LDS: the global loads
// of tile t+1 are in flight (registers) while tile t is consumed, ONE barrier per tile.  Loads are
// unconditional (rows clamped to Ns-1) so the compiler keeps counted waits.  `bias(si, v0, v1)` supplies two
// per-row floats staged next to the tile (every thread evaluates it on a clamped row; 64 threads store).
// body(tile, vec0, vec1, s0) consumes one tile.
template <typename T, int D, typename Bias, typename Body>
__device__ __forceinline__ void stream_tiles(T* tiles, float* vecs, const T* othp, int s_begin, int s_end, int Ns,
                                             Bias&& bias, Body&& body) {
    using L = ALay<T, D>;
    constexpr int NCH = 64 * L::CPR / 256;      // 16-byte chunks per thread and tile
    if (s_begin >= s_end) return;
    u32x4 rg[NCH];
    float bv0 = 0.f, bv1 = 0.f;
    auto load = [&](int s0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = threadIdx.x + 256 * i;
            const int r = c / L::CPR, cc = c % L::CPR;
            rg[i] = *reinterpret_cast<const u32x4*>(othp + (int64_t)min(s0 + r, Ns - 1) * D + cc * L::VEC);
        }
        bias(s0 + (int)(threadIdx.x & 63), bv0, bv1);
    };
    auto store = [&](int buf) {
        T* t = tiles + buf * L::TILE;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = threadIdx.x + 256 * i;
            const int r = c / L::CPR, cc = c % L::CPR;
            *reinterpret_cast<u32x4*>(t + r * L::LDR + cc * L::VEC) = rg[i];
        }
        if (threadIdx.x < 64) {
            vecs[buf * 128 + threadIdx.x] = bv0;
            vecs[buf * 128 + 64 + threadIdx.x] = bv1;
        }
    };
    load(s_begin);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int s0 = s_begin; s0 < s_end; s0 += 64, buf ^= 1) {
        const bool more = s0 + 64 < s_end;
        if (more) load(s0 + 64);
        body(tiles + buf * L::TILE, vecs + buf * 128, vecs + buf * 128 + 64, s0);
        if (more) store(buf ^ 1);
        __syncthreads();
    }
}

template <typename T, int D>
__device__ __forceinline__ void load_owner(Frag<T> (&f)[D / 16], const T* rowptr, int hi) {
#pragma unroll
    for (int s = 0; s < D / 16; ++s) f[s] = ld_frag8(rowptr + 16 * s + 8 * hi);
}

template <typename T, int D>
__device__ __forceinline__ void mma_tile(f32x16& acc, const T* lds, int i0, const Frag<T> (&f)[D / 16],
                                         int l31, int hi) {
    using L = ALay<T, D>;
    const T* base = lds + (i0 + l31) * L::LDR + 8 * hi;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) mma32(acc, ld_frag8(base + 16 * s), f[s]);
}

struct HeadParams {
    const void* own;   // owner matrix  [B, No, D]
    const void* oth;   // streamed matrix [B, Ns, D]
    int B, No, Ns;
    const float* sbias;  // per streamed row  [B, Ns] or null
    const float* obias;  // per owner row     [B, No] or null
    float alpha;
    // outputs / extra inputs (kernel specific)
    float* f0; float* f1; int64_t* i0;
    const float* g0; const float* g1; const float* g2; const float* g3;
    const float* G; int64_t ldg; float galpha; float corner;
    void* out;
    int nsplit;          // workgroups per owner block along the streamed dimension (kernels with disjoint outputs)
};

#define GF_HEAD_PROLOGUE(T, D)                                                                   \
    using L = ALay<T, D>;                                                                         \
    extern __shared__ __attribute__((aligned(16))) char smem[];                                   \
    T* tiles = reinterpret_cast<T*>(smem);                                                        \
    float* vecs = reinterpret_cast<float*>(tiles + 2 * L::TILE);                                  \
    const int nob = (p.No + 127) / 128;                                                           \
    const int nsp = p.nsplit > 1 ? p.nsplit : 1;                                                  \
    const int lb_ = xcd_remap(blockIdx.x, nob * p.B * nsp);                                       \
    const int split = lb_ % nsp, lb = lb_ / nsp;                                                  \
    const int ob = lb % nob, b = lb / nob;                                                        \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                   \
    const int l31 = lane & 31, hi = lane >> 5;                                                    \
    const int orow = ob * 128 + wave * 32 + l31;                                                  \
    const int old_ = min(orow, p.No - 1);                                                         \
    const T* ownp = reinterpret_cast<const T*>(p.own) + (int64_t)b * p.No * D;                    \
    const T* othp = reinterpret_cast<const T*>(p.oth) + (int64_t)b * p.Ns * D;                    \
    Frag<T> of[D / 16];                                                                           \
    load_owner<T, D>(of, ownp + (int64_t)old_ * D, hi);                                           \
    (void)split;

// Running (max, argmax) of one lane.  A lane visits its streamed rows in ASCENDING index order (tiles ascend, and inside a
// tile the offset 32 kb + 8 g + e ascends with (kb, g, e); + 4 hi is fixed per lane), so a strict > keeps the lowest index
// of a tie: one compare + two selects per score, the offset an inline constant; the tile's winner meets the running one
// once per tile, and the full tie rule is only needed where the two half-wave partners meet.
struct TileArg {
    float v; int off;
    __device__ __forceinline__ void reset() { v = -INFINITY; off = 0; }
    __device__ __forceinline__ void see(float x, int off_const) {
        const bool gt = x > v;
        v = gt ? x : v;
        off = gt ? off_const : off;
    }
    __device__ __forceinline__ void merge(int s0, int hi, float& best, int& bidx) const {
        const bool gt = v > best;
        best = gt ? v : best;
        bidx = gt ? s0 + 4 * hi + off : bidx;
    }
};

template <typename T, int D> size_t head_lds() { return 2 * ALay<T, D>::TILE * sizeof(T) + 256 * sizeof(float); }

template <typename K> int set_lds(K kern, size_t bytes) {
    if (bytes > 48 * 1024) {
        if (int e = gf_allow_lds(kern, bytes)) return e;
    }
    return 0;
}

}  // namespace
