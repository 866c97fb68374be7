// Host-side launch helpers for the extern "C" entry points: no device code, no state, nothing that outlives the call.
#pragma once
#include <type_traits>

#include "gf_amd.h"
#include "gf_common.h"

static inline hipStream_t gf_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// f(float{}) or f(bf16_t{}) for the run-time dtype code; f returns the entry point's int.  The call site writes its launch
// once, with `using T = decltype(t)`.
template <typename F> inline int gf_by_dtype(int dtype, F&& f) {
    if (dtype == GF_F32) return f(float{});
    if (dtype == GF_BF16) return f(bf16_t{});
    return GF_ERR_DTYPE;
}
// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument, `decltype(b)::value`.
template <typename F> inline int gf_by_bool(bool flag, F&& f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

// elements of a 16-byte chunk for a dtype code (Vec16<T>::N where T is known)
static inline int gf_vec_elems(int dtype) { return dtype == GF_BF16 ? 8 : 4; }

// opt a kernel in to `bytes` of dynamic LDS; 0 or the hipError_t
template <typename K> inline int gf_allow_lds(K* kernel, size_t bytes) {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// every pointer 16-byte aligned (null counts as aligned)
template <typename... P> inline bool gf_aligned16(const P*... p) {
    return (((uintptr_t)p | ... | (uintptr_t)0) & 15) == 0;
}

static inline int gf_launched() { return (int)hipGetLastError(); }
