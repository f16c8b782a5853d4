// Activation accesses of the tile bodies that one source serves both the launch chain and the persistent decode step with
// (gpt.hip: gemm16_tile, sample_topk_row; attention_core.h: attention_decode_item).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------
// Agent-scope ("sc1") accesses for data that one workgroup hands to another INSIDE a launch (the persistent decode step of gpt.hip; the
// split-K slabs since round 2).  Per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores
// (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility"): the producer stores sc1 (write-through)
// and drains (s_waitcnt vmcnt(0)) before its workgroup signals; EVERY consumer load of those bytes is an sc1 load (it bypasses
// L1) issued after the consumer's poll has matched and its workgroup has passed a barrier.  COH = false: the plain access (a
// kernel boundary orders it), so that one body serves the launch chain and the persistent kernel with identical arithmetic.
// ---------------------------------------------------------------------------------------
template <bool COH>
__device__ __forceinline__ float ld_act(const float* p) {
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool COH>
__device__ __forceinline__ void st_act(float* p, float v) {
    if constexpr (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
// threadIdx.x, opaque to the optimiser when OPAQUE: inside the persistent step's phase loop every lane-derived constant of every
// phase body (LDS offsets, row / column maps, masks -- dozens of registers) is loop-invariant and gets hoisted in front of the loop,
// where it stays live across all the other phases (with a 64-register cap: 19 spills, all of them such values); behind an asm
// statement the optimiser cannot move, each body recomputes its handful of shifts and masks where it runs.
template <bool OPAQUE>
__device__ __forceinline__ int thread_id() {
    int t = threadIdx.x;
    if constexpr (OPAQUE) asm volatile("" : "+v"(t));
    return t;
}
// 16 bytes, sc1 (global_load_dwordx4 ... sc1 through a one-off buffer descriptor: aux bit 4)
__device__ __forceinline__ f32x4 ld_act4_sc1(const float* p) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, 16, 0x00020000);
    typedef unsigned int u32x4_ __attribute__((ext_vector_type(4)));
    const u32x4_ v = __builtin_amdgcn_raw_buffer_load_b128(r, 0, 0, 16);
    return __builtin_bit_cast(f32x4, v);
}
