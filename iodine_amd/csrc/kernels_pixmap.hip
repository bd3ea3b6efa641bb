// Per-pixel likelihood maps and the gradient of the log-likelihood wrt the image and the pixel weights.
//
// Reference (lib/modeling/iodine.py:210-220):
//   K_log_likelihood = gaussian_log_likelihood(x[:, None], mean, sigma)                          (B, K, 3, S, S)   = l_kc
//   log_likelihood   = logsumexp_k(log(mask + 1e-12) + K_log_likelihood)                         (B, 3, S, S)      = ll_c
//   LL               = log_likelihood.mean(0).sum()
// With the pixel weight w_p (iodine_set_pixel_weights, 1 without) the objective's LL is (1 / B) sum_b sum_p w_p sum_c ll_c(p), and
//   d LL / d x[b,c,p] = -(1 / B) sum_k g1_kc        g1_kc = w_p r_kc (x_c - mu_kc) / sigma^2   (r: responsibilities; pixel_terms.h)
//   d LL / d w[b,p]   =  (1 / B) sum_c ll_c(p)      (raw: not multiplied by w)
// The refinement input is detached (iodine.py:343) and the KL term does not see the image, so these direct terms are all of d ELBO / d x.
//
// Two kernels, both apart from pass 1 / pass 2 / pixel_sigma_grad, which stay the same code with the options off:
//   pixel_like_maps_kernel:  the two maps, raw (the weight in lane 3 of the packed image is not read).  Its arithmetic is written out here
//     from the primitives of pixel_terms.h (pt_sigmoid / pt_exp_bounded / pt_rcp; libm and IEEE division under STRICT) because
//     pixel_terms_core only keeps the sum over the channels: sum_c of the map agrees with the reported LL to rounding, not bitwise.
//   pixel_input_grad_kernel: through pixel_terms_core itself, so g1 and ll_sum are the bits pass 1 differentiated and summed.
//     out = coef * v (first) or out += coef * v: the evaluations of a call are added in evaluation order in fp32, one launch each on the
//     same stream - deterministic.  coef == 0 contributes an exact 0 whatever v is.
// One thread owns one pixel, lane i of a wave takes pixel p0 + i: the NHWC4 decoder output and the packed image are read as 16 B per lane at
// consecutive addresses, the NCHW planes are written 4 B per lane at consecutive addresses (256 B per wave and plane), the pattern of
// render_bwd_kernel.  HBM-bound: 16 K + 16 B in, 12 (K + 1) B (maps) or 12 .. 16 B (gradients; twice that when accumulating) out per pixel.
#include "common.h"

#include "pixel_terms.h"

#define PMAP_BLOCK 256

template <int K, bool STRICT, bool JOINT>
__global__ __launch_bounds__(PMAP_BLOCK)
void pixel_like_maps_kernel(const float4* __restrict__ x4, const float4* __restrict__ dec, float* __restrict__ ll, float* __restrict__ kll,
                            int P, float inv2s2, float lconst)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * PMAP_BLOCK + threadIdx.x;
    if (p >= P) return;
    const float4* dec_b = dec + (size_t)b * K * P;
    const float4 xv = x4[(size_t)b * P + p];
    const float xs[3] = {xv.x, xv.y, xv.z};
    float mu[K][3], lm[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float4 d = dec_b[(size_t)k * P + p];
        mu[k][0] = pt_sigmoid<STRICT>(d.x); mu[k][1] = pt_sigmoid<STRICT>(d.y); mu[k][2] = pt_sigmoid<STRICT>(d.z);
        lm[k] = d.w;
        mx = fmaxf(mx, d.w);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { lm[k] = pt_exp_bounded<STRICT>(lm[k] - mx); den += lm[k]; }
    const float rden = pt_rcp<STRICT>(den);
#pragma unroll
    for (int k = 0; k < K; ++k) lm[k] = logf(lm[k] * rden + 1e-12f);
    if constexpr (JOINT) {
        // option joint_likelihood: kll as below, ll (B,1,P) = logsumexp_k(log(m_k + 1e-12) + sum_c l_kc), s_k summed in channel order
        float sk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) sk[k] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float d = xs[c] - mu[k][c];
                const float l = -(d * d) * inv2s2 + lconst;
                if (kll) kll[(((size_t)b * K + k) * 3 + c) * P + p] = l;
                sk[k] += l;
            }
        float amax = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) { sk[k] += lm[k]; amax = fmaxf(amax, sk[k]); }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) s += pt_exp_bounded<STRICT>(sk[k] - amax);
        if (ll) ll[(size_t)b * P + p] = amax + logf(s);
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float a[K], amax = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float d = xs[c] - mu[k][c];
            const float l = -(d * d) * inv2s2 + lconst;
            if (kll) kll[(((size_t)b * K + k) * 3 + c) * P + p] = l;
            a[k] = lm[k] + l;
            amax = fmaxf(amax, a[k]);
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) s += pt_exp_bounded<STRICT>(a[k] - amax);
        if (ll) ll[((size_t)b * 3 + c) * P + p] = amax + logf(s);
    }
}

// gx + b * gx_bs: the (3, P) planes of image b; gw + b * gw_bs: its (P) plane.  The strides let one frame of a batch-first clip (B, F, 3, P)
// be written in place.
template <int K, bool STRICT, bool JOINT>
__global__ __launch_bounds__(PMAP_BLOCK)
void pixel_input_grad_kernel(const float4* __restrict__ x4, const float4* __restrict__ dec, float* __restrict__ gx, size_t gx_bs,
                             float* __restrict__ gw, size_t gw_bs, int P, float inv2s2, float invs2, float lconst, float coef, int first_x,
                             int first_w)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * PMAP_BLOCK + threadIdx.x;
    if (p >= P) return;
    PixelTerms<K> t;
    const float4 xv = x4[(size_t)b * P + p];
    pixel_terms<K, STRICT, JOINT>(xv, dec + (size_t)b * K * P, (size_t)P, (size_t)p, inv2s2, invs2, lconst, t);
    if (gx) {
        float* o = gx + (size_t)b * gx_bs + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) v += t.g1[k][c];
            const float q = coef == 0.f ? 0.f : coef * -v;
            o[(size_t)c * P] = first_x ? q : o[(size_t)c * P] + q;
        }
    }
    if (gw) {
        float* o = gw + (size_t)b * gw_bs + p;
        const float q = coef == 0.f ? 0.f : coef * t.ll_sum;
        *o = first_w ? q : *o + q;
    }
}

#define FOR_EACH_K(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

hipError_t launch_pixel_like_maps(hipStream_t st, const float* x4, const float* dec, float* ll, float* kll, int B, int K, int P, float sigma,
                                  int strict, int joint)
{
    if (!x4 || !dec || B < 1 || P < 1) return hipErrorInvalidValue;
    if (!ll && !kll) return hipSuccess;
    const dim3 grid((P + PMAP_BLOCK - 1) / PMAP_BLOCK, B);
    const float inv2s2 = 1.f / (2.f * sigma * sigma);
    const float lconst = (float)(-log((double)sigma) - 0.5 * log(2.0 * M_PI));
    switch (K) {
#define LM(KK, ST, JT) hipLaunchKernelGGL((pixel_like_maps_kernel<KK, ST, JT>), grid, dim3(PMAP_BLOCK), 0, st, (const float4*)x4, (const float4*)dec, ll, kll, P, inv2s2, lconst)
#define CASE(KK) case KK: \
        if (joint) { if (strict) LM(KK, true, true); else LM(KK, false, true); } \
        else { if (strict) LM(KK, true, false); else LM(KK, false, false); } \
        break;
        FOR_EACH_K(CASE)
#undef CASE
#undef LM
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_pixel_input_grad(hipStream_t st, const float* x4, const float* dec, float* gx, size_t gx_bs, float* gw, size_t gw_bs, int B,
                                   int K, int P, float sigma, int strict, float coef, int first_x, int first_w, int joint)
{
    if (!x4 || !dec || B < 1 || P < 1) return hipErrorInvalidValue;
    if (!gx && !gw) return hipSuccess;
    const dim3 grid((P + PMAP_BLOCK - 1) / PMAP_BLOCK, B);
    const float inv2s2 = 1.f / (2.f * sigma * sigma), invs2 = 1.f / (sigma * sigma);
    const float lconst = (float)(-log((double)sigma) - 0.5 * log(2.0 * M_PI));
    switch (K) {
#define IG(KK, ST, JT) hipLaunchKernelGGL((pixel_input_grad_kernel<KK, ST, JT>), grid, dim3(PMAP_BLOCK), 0, st, (const float4*)x4, (const float4*)dec, gx, gx_bs, gw, gw_bs, P, inv2s2, invs2, lconst, coef, first_x, first_w)
#define CASE(KK) case KK: \
        if (joint) { if (strict) IG(KK, true, true); else IG(KK, false, true); } \
        else { if (strict) IG(KK, true, false); else IG(KK, false, false); } \
        break;
        FOR_EACH_K(CASE)
#undef CASE
#undef IG
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
