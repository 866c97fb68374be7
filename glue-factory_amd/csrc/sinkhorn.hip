// Log-domain Sinkhorn optimal transport with dustbins: the C entry points (include/gf_amd.h), the problem geometry and
// workspace carve, and the choice between the three implementations.  The maths is stated at the top of sinkhorn_common.h.
#include "sinkhorn_common.h"

namespace gfsk {

Geo make_geo(int B, int M, int N) {
    Geo g;
    g.B = B; g.M = M; g.N = N; g.R = M + 1; g.C = N + 1;
    g.Cp = (g.C + 3) & ~3;
    g.fast = (g.Cp >> 2) <= 64 * SKF_MAX_NS;
    if (g.fast) {
        g.RB = SKF_RPB;
    } else {
        // generic path: rows per block bounded by LDS (RB rows + 4 column vectors), at most 16
        size_t rb = (LDS_BUDGET - 4 * (size_t)g.C * 4 - 512) / ((size_t)g.C * 4);
        g.RB = (int)(rb > 16 ? 16 : rb);
    }
    g.nblk = g.RB > 0 ? (g.R + g.RB - 1) / g.RB : 0;
    g.norm = -logf((float)(M + N));
    g.lmu_last = logf((float)N) + g.norm;
    g.lnu_last = logf((float)M) + g.norm;
    return g;
}

// Pairs per chunk (balanced over the batch).  Measured on MI355X (tools/probe/time_sinkhorn.py, B=32, N=2048, T=100,
// forward ms): chunks of 1 / 2 / 4 / 8 / 16 / 32 pairs = 49.0 / 28.3 / 17.9 / 12.8 / 11.2 / 11.8 -- small chunks are
// launch/latency-bound and keeping a chunk under the Infinity Cache size (8 pairs = 134 MB) buys nothing: the row
// sweep streams at ~5 TB/s either way.  The chunk only bounds the padded copy / factor workspaces.
int batch_chunk(const Geo& g) {
    size_t per = g.fast ? (size_t)g.R * g.Cp * 4 + (size_t)g.nblk * g.Cp * 4
                        : (size_t)g.R * g.C * 4 + 2 * (size_t)g.nblk * g.C * 4;
    int ch = (int)((size_t)SK_CHUNK_MB * 1024 * 1024 / per);
    ch = ch < 1 ? 1 : (ch > g.B ? g.B : ch);
    const int nch = (g.B + ch - 1) / ch;
    return (g.B + nch - 1) / nch;
}

// workspace carve (layout: struct Ws); ws == nullptr only measures (w.total, w.part_rows)
Ws carve(void* ws, const Geo& g, int iters) {
    Ws w;
    float* p = reinterpret_cast<float*>(ws);
    const size_t wid = g.fast ? g.Cp : g.C;
    w.part_rows = 2 * (size_t)g.B * g.nblk;
    if (g.fast && w.part_rows < 4 * (size_t)SKR_PART_CUS) w.part_rows = 4 * (size_t)SKR_PART_CUS;   // resident path: one row per wave
    w.part = p;       p += w.part_rows * wid;
    w.ucur = p;       p += (size_t)g.B * g.R;
    w.vcur = p;       p += (size_t)g.B * wid;
    w.ubar_hist = p;  p += (size_t)(iters + 1) * g.B * g.R;
    w.vbar_hist = p;  p += (size_t)(iters + 1) * g.B * g.C;
    p += (4 - ((p - reinterpret_cast<float*>(ws)) & 3)) & 3;      // 16-byte aligned Zp
    w.zp = p;
    w.KP = (2 * iters + 15) & ~15;
    w.a2p = w.vbp = w.P = w.Q = nullptr;
    w.ctr = nullptr;
    if (g.fast) {
        const size_t ch = (size_t)batch_chunk(g);
        p += ch * g.R * g.Cp;
        w.a2p = p;  p += (size_t)g.B * g.Cp;
        w.vbp = p;  p += (size_t)g.B * g.Cp;
        w.P = p;    p += ch * g.R * w.KP;        // rank-2T factors of the final gradient (backward only)
        w.Q = p;    p += ch * g.C * w.KP;
        w.ctr = reinterpret_cast<unsigned*>(p);  p += 64;       // pair-barrier counters of the resident path
    }
    w.total = (size_t)(p - reinterpret_cast<float*>(ws)) * 4 + 1024;
    return w;
}

}  // namespace gfsk

using namespace gfsk;

namespace {

// Which implementation serves a call, and in chunks of how many pairs.  The ONLY place that decides it: the entry points
// below and gf_sinkhorn_plan all ask here.
//   generic  (sinkhorn_generic.hip)   N + 1 > 2304
//   stream   (sinkhorn_stream.hip)    the rest, unless
//   resident (sinkhorn_resident.hip)  the schedule allows it, there is at least one iteration, skr_plan finds a distribution
//                                     over `ncu` compute units (0: those of the current device) and the workspace holds a
//                                     partial row for every wave of a launch
enum class Tier { generic, stream, resident };
struct Choice {
    Tier tier;
    int ch;          // pairs per chunk
    SkrPlan plan;    // resident only
};
Choice select_tier(const Geo& g, int B, int iters, bool bwd, int schedule, int ncu, const Ws& w) {
    Choice c;
    c.tier = g.fast ? Tier::stream : Tier::generic;
    c.ch = batch_chunk(g);
    if (g.fast && iters > 0 && skr_plan(g, B, ncu > 0 ? ncu : skr_cus(), bwd, schedule & 3, c.plan) &&
        (size_t)c.plan.nw * c.plan.bc <= w.part_rows) {
        c.tier = Tier::resident;
        c.ch = c.plan.bc;
    }
    return c;
}

}  // namespace

// Host-only: the distribution the chip-resident path would use for this problem on a device of `ncu` compute units
// (out[8] = pairs per launch, workgroups per pair, waves per pair, rows per wave, waves with one more row, float4 columns per
// workgroup in the column phase, N / 256, LDS bytes).  Returns 1 and fills `out`, or 0 when the streaming kernels are used.
extern "C" int gf_sinkhorn_plan(int B, int M, int N, int ncu, int backward, int schedule, int64_t* out) {
    if (B <= 0 || M <= 0 || N <= 0 || ncu <= 0 || out == nullptr || (schedule & 3) == 3) return GF_ERR_SHAPE;
    const Geo g = make_geo(B, M, N);
    if (g.RB < 1) return 0;
    const Choice c = select_tier(g, B, 1, backward != 0, schedule, ncu, carve(nullptr, g, 1));
    if (c.tier != Tier::resident) return 0;
    const SkrPlan& d = c.plan;
    const int64_t v[8] = {d.bc, d.wpp, d.nw, d.base, d.extra, d.cs, d.nsm, (int64_t)d.lds};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 1;
}

extern "C" int64_t gf_sinkhorn_ws_bytes(int B, int M, int N, int iters) {
    if (B <= 0 || M <= 0 || N <= 0 || iters < 0) return GF_ERR_SHAPE;
    Geo g = make_geo(B, M, N);
    if (g.RB < 1) return GF_ERR_UNSUPPORTED;
    return (int64_t)carve(nullptr, g, iters).total;
}

extern "C" int gf_sinkhorn_fwd(const float* Z, float* out, float* u_hist, float* v_hist, void* ws,
                               int B, int M, int N, int iters, int schedule, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0 || iters < 0 || (schedule & 3) == 3) return GF_ERR_SHAPE;
    const Geo g = make_geo(B, M, N);
    if (g.RB < 1) return GF_ERR_UNSUPPORTED;
    if (!gf_aligned16(ws)) return GF_ERR_ALIGN;
    hipStream_t st = gf_stream(stream);
    const Ws w = carve(ws, g, iters);
    const Choice c = select_tier(g, B, iters, false, schedule, 0, w);
    SkrArgs ra{};
    if (c.tier == Tier::resident) ra = skr_shared_args(g, w, c.plan, iters, schedule);
    const size_t zs = (size_t)g.R * g.C;
    for (int b0 = 0; b0 < B; b0 += c.ch) {
        const int bc = (B - b0) < c.ch ? (B - b0) : c.ch;
        const float* Zc = Z + b0 * zs;
        float* uh = u_hist + (size_t)b0 * g.R;
        float* vh = v_hist + (size_t)b0 * g.C;
        int rc = 0;
        if (c.tier == Tier::resident) {
            // the chunk stays on the chip for all iterations; it is loaded from the couplings themselves and writes `out`
            // from its last iteration
            ra.Zraw = Zc; ra.out = out + b0 * zs;
            ra.u_hist = uh; ra.v_hist = vh;
            ra.d.bc = bc;
            rc = skr_fwd_launch(ra, st);
        } else if (c.tier == Tier::stream) {
            if (iters > 0) {
                skf_prescale_launch(Zc, w.zp, g, bc, st);
                rc = skf_fwd_launch(w.zp, w.vcur + (size_t)b0 * g.Cp, w.ucur + (size_t)b0 * g.R, uh, vh,
                                    w.part + (size_t)b0 * g.nblk * g.Cp, g, bc, iters, st);
            }
        } else {
            float* pm = w.part + (size_t)b0 * g.nblk * g.C;
            rc = sk_fwd_launch(Zc, w.ucur + (size_t)b0 * g.R, w.vcur + (size_t)b0 * g.C, uh, vh, pm,
                               pm + (size_t)B * g.nblk * g.C, g, bc, iters, st);
        }
        if (rc) return rc;
        // out = Z + u + v - norm with the final iterates (natural-log units = the last history entries); the resident kernel
        // has written it already
        if (c.tier != Tier::resident)
            sk_final_fwd_launch(Zc, iters ? uh + (size_t)(iters - 1) * B * g.R : nullptr,
                                iters ? vh + (size_t)(iters - 1) * B * g.C : nullptr, out + b0 * zs, g, bc, st);
    }
    return gf_launched();
}

extern "C" int gf_sinkhorn_bwd(const float* Z, const float* gout, const float* gsum_row, const float* gsum_col,
                               const float* u_hist, const float* v_hist, float* gZ, void* ws,
                               int B, int M, int N, int iters, int schedule, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0 || iters < 0 || (schedule & 3) == 3) return GF_ERR_SHAPE;
    const Geo g = make_geo(B, M, N);
    if (g.RB < 1) return GF_ERR_UNSUPPORTED;
    if (!gf_aligned16(ws)) return GF_ERR_ALIGN;
    hipStream_t st = gf_stream(stream);
    const Ws w = carve(ws, g, iters);             // ubar_hist [iters, B, R] (index k-1), vbar_hist [iters+1, B, C] (index k = 0..T)
    const size_t zs = (size_t)g.R * g.C;
    if (iters == 0) return (int)gf_copy_f32(gZ, gout, (size_t)B * zs, st);
    // vbar^T = colsum(G)
    hipError_t e = gf_copy_f32(w.vbar_hist + (size_t)iters * B * g.C, gsum_col, (size_t)B * g.C, st);
    if (e != hipSuccess) return (int)e;
    const Choice c = select_tier(g, B, iters, true, schedule, 0, w);
    SkrArgs ra{};
    if (c.tier == Tier::resident) ra = skr_shared_args(g, w, c.plan, iters, schedule);
    for (int b0 = 0; b0 < B; b0 += c.ch) {
        const int bc = (B - b0) < c.ch ? (B - b0) : c.ch;
        const float* Zc = Z + b0 * zs;
        const float* uh = u_hist + (size_t)b0 * g.R;
        const float* vh = v_hist + (size_t)b0 * g.C;
        float* ubh = w.ubar_hist + (size_t)b0 * g.R;
        float* vbh = w.vbar_hist + (size_t)b0 * g.C;
        if (c.tier == Tier::generic) {
            int rc = sk_bwd_launch(Zc, gout + b0 * zs, gsum_row + (size_t)b0 * g.R, uh, vh, ubh, vbh,
                                   w.part + (size_t)b0 * g.nblk * g.C, gZ + b0 * zs, g, bc, iters, st);
            if (rc) return rc;
            continue;
        }
        // both register tiers: padded copy, first column vectors, T reverse sweeps, then dZ as one rank-2T product.  The
        // streaming sweeps keep per-pair scratch for the whole batch; a resident chunk uses the front of it.
        const bool resident = c.tier == Tier::resident;
        float* a2p = w.a2p + (resident ? 0 : (size_t)b0 * g.Cp);
        float* vbp = w.vbp + (resident ? 0 : (size_t)b0 * g.Cp);
        skf_prescale_launch(Zc, w.zp, g, bc, st);
        skf_bwd_prep_launch(vh + (size_t)(iters - 1) * B * g.C, gsum_col + (size_t)b0 * g.C, a2p, vbp, g, bc, st);
        int rc;
        if (resident) {
            ra.u_hist = const_cast<float*>(uh); ra.v_hist = const_cast<float*>(vh);
            ra.base_row = gsum_row + (size_t)b0 * g.R;
            ra.ubar_hist = ubh; ra.vbar_hist = vbh;
            ra.d.bc = bc;
            rc = skr_bwd_launch(ra, st);
        } else {
            rc = skf_bwd_launch(w.zp, uh, vh, gsum_row + (size_t)b0 * g.R, ubh, vbh, w.part + (size_t)b0 * g.nblk * g.Cp,
                                a2p, vbp, g, bc, iters, st);
        }
        if (rc) return rc;
        skf_final_bwd_launch(Zc, gout + b0 * zs, uh, vh, ubh, vbh, w.P, w.Q, w.KP, gZ + b0 * zs, g, bc, iters, st);
    }
    return gf_launched();
}
