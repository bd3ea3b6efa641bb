// Scene edits (include/iodine_hip.h: iodine_scene_edit): the rendering of final_out_kernel for E copies of a decoded scene that each differ
// from it in ONE slot - replaced by a freshly decoded slot-image, or removed.  The decoder treats slot-images independently; only this
// per-pixel step couples the slots of an image, so an edit costs one slot-image decode (a removal: none) plus one pass of this kernel.
//
// scene_edit_out_kernel<K>: grid (ceil(P / PIX_BLOCK), edits of the launch), one thread per pixel, no LDS, no atomics.  Edit e of the launch
// reads the K float4 (pre-sigmoid rgb + logit, [N][P][4]) of image b from the base decoder output - K * 16 B per pixel and edit, re-read by
// every edit of the image and meant to come from L2 - except slot s, which comes from row src of the edit decoder's output.  A removal
// (src < 0) keeps the base slot and sets its logit to -inf: expf(-inf) is an exact 0, so the maximum, the denominator and pred are those of
// the K - 1 other slots and the removed slot's mask is exactly 0 (the build uses no fast-math flag; the host refuses a removal at K = 1,
// where the denominator would be 0).  The arithmetic is final_out_kernel's, operation by operation: max over k, expf(w - mx), den summed
// in k order, one reciprocal, m[k] *= rden, sigmoidf_, pr[c] += m[k] * mu[c] in k order - a replace edit gives the bits of a full decode.
//
// The per-edit indices (image, slot, source row) are host values: they travel in the kernel arguments (SceneEditList, by value), so the
// entry point needs no index buffer, no host-to-device copy and no synchronise.  The host has range-checked every one of them.
#include "common.h"

#define PIX_BLOCK 256

template <int K>
__global__ __launch_bounds__(PIX_BLOCK)
void scene_edit_out_kernel(const float4* __restrict__ base, const float4* __restrict__ edit, const SceneEditList list,
                           float* __restrict__ pred, float* __restrict__ mask, float* __restrict__ mean, int P)
{
    const int e = blockIdx.y;
    const int p = blockIdx.x * PIX_BLOCK + threadIdx.x;
    if (p >= P) return;
    const int b = list.bs[e] >> 4, s = list.bs[e] & 15, src = list.src[e];       // block-uniform
    const float4* base_b = base + (size_t)b * K * P;
    float4 d[K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float4* q = (k == s && src >= 0) ? edit + (size_t)src * P : base_b + (size_t)k * P;
        d[k] = q[p];
        if (k == s && src < 0) d[k].w = -INFINITY;
        mx = fmaxf(mx, d[k].w);
    }
    float m[K], den = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { m[k] = expf(d[k].w - mx); den += m[k]; }
    const float rden = 1.f / den;
    float pr[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
        m[k] *= rden;
        const float mu[3] = {sigmoidf_(d[k].x), sigmoidf_(d[k].y), sigmoidf_(d[k].z)};
        if (mask) mask[((size_t)e * K + k) * P + p] = m[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (mean && k == s) mean[((size_t)e * 3 + c) * P + p] = mu[c];
            pr[c] += m[k] * mu[c];
        }
    }
    if (pred)
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[((size_t)e * 3 + c) * P + p] = pr[c];
}

#define FOR_EACH_K(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

// pred (n,3,P), mask (n,K,P), mean (n,3,P) of the list's n edits, each may be NULL; base [B K][P][4], edit [rows][P][4] (not read when every
// src is < 0).  The caller guarantees 1 <= list.n <= SCENE_EDIT_MAX, image < B, slot < K, src < rows.
hipError_t launch_scene_edit_out(hipStream_t st, const float* base, const float* edit, const SceneEditList& list, float* pred, float* mask,
                                 float* mean, int K, int P)
{
    if (list.n < 1 || list.n > SCENE_EDIT_MAX) return hipErrorInvalidValue;
    const dim3 grid((P + PIX_BLOCK - 1) / PIX_BLOCK, list.n);
    switch (K) {
#define CASE(KK) case KK: hipLaunchKernelGGL((scene_edit_out_kernel<KK>), grid, dim3(PIX_BLOCK), 0, st, \
        (const float4*)base, (const float4*)edit, list, pred, mask, mean, P); break;
        FOR_EACH_K(CASE)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
