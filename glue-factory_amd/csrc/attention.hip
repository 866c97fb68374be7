// Flash-style multi-head attention over N keypoints, forward and backward, for gfx950: the C entry points, their argument
// checks and the choice of kernel family.  The kernels live in one translation unit per family (launch functions in
// attn_common.h).
//
// Replaces (reference) gluefactory/models/matchers/lightglue.py:97-128 (Attention / SDPA),
// :161 (self attention context) and :203-216 (cross attention, both directions as two calls
// with (q,k,v) = (qk0,qk1,v1) and (qk1,qk0,v0)), and gluefactory_nonfree/superglue.py:112-116.
//
// Layout: q,k,v,o are [B, N, H, hd] views with arbitrary element strides for (b, n, h) and
// hd contiguous (so the fused Wqkv output is consumed in place).  lse/delta are [B,H,N] fp32.
#include "gf_launch.h"
#include "attn_common.h"

using namespace gfattn;

namespace {

bool bad_stride(const int64_t* s, int align) { return s[0] % align || s[1] % align || s[2] % align; }

// The argument checks forward and backward share, and the AttnParams fields both fill.  `known`: the flag bits the entry
// point takes; `o_f32_if_split`: the backward's `o` under GF_ATTN_SPLIT is the forward's fp32 copy (strides in fp32 elements).
int attn_params(AttnParams& p, const void* q, const void* k, const void* v, const void* o, const float* lse,
                int B, int H, int Nq, int Nk, int D, const int64_t* qs, const int64_t* ks, const int64_t* vs, const int64_t* os,
                float scale, int dtype, int flags, int known, bool o_f32_if_split) {
    if (D != 64 && D != 32 && D != 128) return GF_ERR_UNSUPPORTED;
    if (flags & ~known) return GF_ERR_UNSUPPORTED;
    if (D != 64 && (flags & GF_ATTN_SPLIT) && dtype != GF_F32) return GF_ERR_UNSUPPORTED;   // split products: 64-wide heads only
    if (dtype == GF_F32) flags &= ~GF_ATTN_SPLIT;                    // fp32 operands: nothing to split
    // the split products exist in the LDS-DMA bf16 kernels only (rows addressed through 32-bit buffer offsets)
    if ((flags & GF_ATTN_SPLIT) && !(kvdma_ok(Nk, ks[1]) && kvdma_ok(Nk, vs[1]))) return GF_ERR_UNSUPPORTED;
    if (B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0) return GF_ERR_SHAPE;
    const int align = gf_vec_elems(dtype);
    if (bad_stride(qs, align) || bad_stride(ks, align) || bad_stride(vs, align) ||
        bad_stride(os, (o_f32_if_split && (flags & GF_ATTN_SPLIT)) ? 4 : align))
        return GF_ERR_ALIGN;
    p = {};
    p.q = q; p.k = k; p.v = v; p.o = const_cast<void*>(o); p.lse = const_cast<float*>(lse);
    p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.scale = scale;
    host_split_scale(scale, p.p2, p.rr);
    p.flags = flags;
    p.sqb = qs[0]; p.sqn = qs[1]; p.sqh = qs[2];
    p.skb = ks[0]; p.skn = ks[1]; p.skh = ks[2];
    p.svb = vs[0]; p.svn = vs[1]; p.svh = vs[2];
    p.sob = os[0]; p.son = os[1]; p.soh = os[2];
    return 0;
}

// Which kernels run:
//   bf16, D = 64, K / V rows within kvdma_ok   fwd3 | dq3 + dkv_bf16      (LDS-DMA kernels: the step's path)
//   bf16, D = 64, otherwise                    generic forward | generic dQ + dkv_bf16
//   fp32; bf16 at D = 32 / 128                 generic forward | generic dQ (ATTN_PLAIN_STATS) + generic dK/dV
bool lds_dma(const AttnParams& p, int dtype, int D) {
    return dtype == GF_BF16 && D == 64 && kvdma_ok(p.Nk, p.skn) && kvdma_ok(p.Nk, p.svn);
}
int launch_fwd(const AttnParams& p, hipStream_t st, int dtype, int D) {
    return lds_dma(p, dtype, D) ? launch_fwd3_bf16(p, st) : launch_fwd_generic(p, st, dtype, D);
}
int launch_bwd(const AttnParams& p, hipStream_t st, int dtype, int D) {
    if (dtype != GF_BF16 || D != 64) return launch_bwd_generic(p, st, dtype, D);
    if (int e = lds_dma(p, dtype, D) ? launch_dq3_bf16(p, st) : launch_dq_generic(p, st, dtype, D)) return e;
    return launch_dkv_bf16(p, st);
}

}  // namespace

extern "C" int gf_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                           int B, int H, int Nq, int Nk, int D,
                           const int64_t* q_strides, const int64_t* k_strides,
                           const int64_t* v_strides, const int64_t* o_strides,
                           float scale, int dtype, void* stream) {
    return gf_attn_fwd_ex(q, k, v, o, lse, B, H, Nq, Nk, D, q_strides, k_strides, v_strides, o_strides, scale, dtype, 0, nullptr, stream);
}
extern "C" int gf_attn_fwd_ex(const void* q, const void* k, const void* v, void* o, float* lse,
                              int B, int H, int Nq, int Nk, int D,
                              const int64_t* q_strides, const int64_t* k_strides,
                              const int64_t* v_strides, const int64_t* o_strides,
                              float scale, int dtype, int flags, float* o32, void* stream) {
    AttnParams p;
    if (int e = attn_params(p, q, k, v, o, lse, B, H, Nq, Nk, D, q_strides, k_strides, v_strides, o_strides, scale, dtype,
                            flags, GF_ATTN_SPLIT, false))
        return e;
    p.o32 = (p.flags & GF_ATTN_SPLIT) ? o32 : nullptr;
    return launch_fwd(p, gf_stream(stream), dtype, D);
}

extern "C" int gf_attn_bwd(const void* q, const void* k, const void* v, const void* o,
                           const void* dout, const float* lse, float* delta,
                           void* dq, void* dk, void* dv,
                           int B, int H, int Nq, int Nk, int D,
                           const int64_t* q_strides, const int64_t* k_strides,
                           const int64_t* v_strides, const int64_t* o_strides,
                           const int64_t* do_strides, const int64_t* dq_strides,
                           const int64_t* dk_strides, const int64_t* dv_strides,
                           float scale, int dtype, void* stream) {
    return gf_attn_bwd_acc(q, k, v, o, dout, lse, delta, dq, dk, dv, B, H, Nq, Nk, D, q_strides, k_strides, v_strides, o_strides,
                           do_strides, dq_strides, dk_strides, dv_strides, scale, dtype, 0, stream);
}

extern "C" int gf_attn_bwd_acc(const void* q, const void* k, const void* v, const void* o,
                               const void* dout, const float* lse, float* delta,
                               void* dq, void* dk, void* dv,
                               int B, int H, int Nq, int Nk, int D,
                               const int64_t* q_strides, const int64_t* k_strides,
                               const int64_t* v_strides, const int64_t* o_strides,
                               const int64_t* do_strides, const int64_t* dq_strides,
                               const int64_t* dk_strides, const int64_t* dv_strides,
                               float scale, int dtype, int flags, void* stream) {
    AttnParams p;
    if (int e = attn_params(p, q, k, v, o, lse, B, H, Nq, Nk, D, q_strides, k_strides, v_strides, o_strides, scale, dtype,
                            flags, GF_ATTN_ACC_DQ | GF_ATTN_ACC_DK | GF_ATTN_SPLIT, true))
        return e;
    const int align = gf_vec_elems(dtype);
    if (bad_stride(do_strides, align) || bad_stride(dq_strides, align) || bad_stride(dk_strides, align) || bad_stride(dv_strides, align))
        return GF_ERR_ALIGN;
    p.dout = dout; p.delta = delta; p.dq = dq; p.dk = dk; p.dv = dv;
    p.sdob = do_strides[0]; p.sdon = do_strides[1]; p.sdoh = do_strides[2];
    p.sdqb = dq_strides[0]; p.sdqn = dq_strides[1]; p.sdqh = dq_strides[2];
    p.sdkb = dk_strides[0]; p.sdkn = dk_strides[1]; p.sdkh = dk_strides[2];
    p.sdvb = dv_strides[0]; p.sdvn = dv_strides[1]; p.sdvh = dv_strides[2];
    return launch_bwd(p, gf_stream(stream), dtype, D);
}
