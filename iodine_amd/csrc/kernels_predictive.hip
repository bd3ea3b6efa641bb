// Multi-sample evaluation (include/iodine_hip.h: iodine_predictive): S draws z_s = mu + exp(logvar / 2) eps_s from one posterior, decoded by
// the existing decoder kernels as S B K independent slot-images; everything that couples the samples sits in the per-pixel step below -
// running mean / M2 of the rendered image and of the masks, the count of samples in which each slot wins the pixel, and the per-image
// log-likelihood of every sample.  No sample's NCHW planes are ever written.
//
// predictive_accum_kernel<K, STRICT, HAS_X, JOINT>: grid (ceil(P / PIX_BLOCK), B), one thread owns one pixel of one image for ALL n_s samples of
// the launch (block-uniform, in the arguments), no atomics, no LDS except the block sum of the likelihood.  Per sample, in sample order:
//   * K float4 (pre-sigmoid rgb + logit, [n_s B K][P][4], sample-major) at 16 B per lane, consecutive lanes on consecutive pixels, rendered
//     with final_out_kernel's arithmetic operation for operation - max over k, expf(w - mx), den in k order, one reciprocal, m[k] *= rden,
//     sigmoidf_, pr[c] += m[k] * mu[c] in k order: the sample's pred / mask are the bits iodine_decode returns for z_s.  That last
//     statement is written as fmaf here: under the build's fp contraction final_out_kernel<K> compiles it to one fused chain
//     fma(m0, mu0, 0), fma(m1, mu1, .), .. for every K, while in this larger loop body the vectoriser pairs the products over k and leaves
//     some of them unfused (1 ulp apart) - the explicit form pins the chain the decode uses;
//   * Welford in fp32 with n = the GLOBAL 1-based sample index: mean += (v - mean) / n, M2 += (v - mean_old) (v - mean_new), for the 3
//     values of pred and the K of mask (IEEE division, no contraction: the update is the same code whatever the chunking);
//   * votes[b][k*][p] += 1 for the arg-max slot of the sample's mask, strict `>` from -inf upwards like slot_table_kernel: the lowest
//     index wins a tie, a NaN never wins;
//   * HAS_X: pixel_terms_core<K, STRICT, JOINT> (JOINT: option joint_likelihood, the form of ll_sum) on the packed image {r, g, b, w}; w_p ll_sum - what pass 1 sums - goes through a wave sum and a
//     block sum in fp64 to part[s][b][block]; predictive_ll_kernel adds the blocks in block order and writes ll (S, B) in fp32.
// The moment state lives in the OUTPUT buffers: a launch whose first sample is not sample 0 reads it, every launch writes it back, and the
// update is strictly sequential in the sample index, so the result does not depend on how the samples are cut into launches.  Up to
// K = PRED_REG_K the mask moments and the votes stay in registers for the launch (3 K values); above it they stay in global memory and are
// touched once per sample - the same thread re-reads what it wrote, L2-resident between samples - so that no instantiation spills.
// Traffic per pixel and sample: 16 K bytes in; once per launch 16 more for the image with HAS_X and the state, (2 K + 6) floats + K ints in
// and out (K <= PRED_REG_K), or 8 K + 8 bytes in and out per sample for the mask moments and the one vote touched (K > PRED_REG_K).
#include "common.h"

#define PIX_BLOCK 256
#define PRED_REG_K 8

#include "pixel_terms.h"

// one value of the running moments; n = the 1-based index of the sample as a float (exact: the host refuses more than 2^24 samples)
IOD_DEVINL void welford_step(float v, float n, float& mean, float& m2)
{
#pragma clang fp contract(off)
    const float d0 = v - mean;
    mean = mean + d0 / n;
    m2 = m2 + d0 * (v - mean);
}

template <int K, bool STRICT, bool HAS_X, bool JOINT>        // JOINT: option joint_likelihood (pixel_terms.h), with HAS_X only
__global__ __launch_bounds__(PIX_BLOCK)
void predictive_accum_kernel(const float4* __restrict__ dec, const float4* __restrict__ x4, int B, int P, int s0, int n_s,
                             float* pred_mean, float* pred_m2, float* mask_mean, float* mask_m2, int* votes,
                             double* __restrict__ part, float inv2s2, float invs2, float lconst)
{
    constexpr bool REG = K <= PRED_REG_K;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int pr_ = blockIdx.x * PIX_BLOCK + tid;
    const bool valid = pr_ < P;                     // (no early return with HAS_X: the block sum below has a barrier)
    if (!HAS_X && !valid) return;
    const int p = valid ? pr_ : P - 1;              // idle lanes of the last block recompute its last pixel and store nothing
    const size_t sP = (size_t)P;
    float* pm_ = pred_mean + (size_t)b * 3 * sP + p;
    float* p2_ = pred_m2 + (size_t)b * 3 * sP + p;
    float* mm_ = mask_mean + (size_t)b * K * sP + p;
    float* m2_ = mask_m2 + (size_t)b * K * sP + p;
    int* vt_ = votes + (size_t)b * K * sP + p;

    float pmean[3] = {0.f, 0.f, 0.f}, pm2[3] = {0.f, 0.f, 0.f};
    float mmean[REG ? K : 1], mm2[REG ? K : 1];
    int vt[REG ? K : 1];
    if (s0 > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { pmean[c] = pm_[c * sP]; pm2[c] = p2_[c * sP]; }
    }
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            mmean[k] = s0 > 0 ? mm_[k * sP] : 0.f;
            mm2[k] = s0 > 0 ? m2_[k * sP] : 0.f;
            vt[k] = s0 > 0 ? vt_[k * sP] : 0;
        }
    } else if (s0 == 0 && valid) {
#pragma unroll
        for (int k = 0; k < K; ++k) { mm_[k * sP] = 0.f; m2_[k * sP] = 0.f; vt_[k * sP] = 0; }
    }

    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (HAS_X) xv = x4[(size_t)b * sP + p];
    __shared__ double s_red[2][PIX_BLOCK / 64];     // two sets: one barrier per sample

    for (int s = 0; s < n_s; ++s) {
        const float4* dec_b = dec + ((size_t)s * B + b) * K * sP;
        float4 d[K];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) { d[k] = dec_b[(size_t)k * sP + p]; mx = fmaxf(mx, d[k].w); }
        float m[K], den = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { m[k] = expf(d[k].w - mx); den += m[k]; }
        const float rden = 1.f / den;
        float pr[3] = {0.f, 0.f, 0.f};
        float bv = -INFINITY;
        int best = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            m[k] *= rden;
            const float mu[3] = {sigmoidf_(d[k].x), sigmoidf_(d[k].y), sigmoidf_(d[k].z)};
#pragma unroll
            for (int c = 0; c < 3; ++c) pr[c] = fmaf(m[k], mu[c], pr[c]);       // (see the head of the file: final_out_kernel's chain is fused)
            if (m[k] > bv) { bv = m[k]; best = k; }
        }
        const float n = (float)(s0 + s + 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) welford_step(pr[c], n, pmean[c], pm2[c]);
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < K; ++k) { welford_step(m[k], n, mmean[k], mm2[k]); vt[k] += best == k ? 1 : 0; }
        } else if (valid) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float a = mm_[k * sP], q = m2_[k * sP];
                welford_step(m[k], n, a, q);
                mm_[k * sP] = a; m2_[k * sP] = q;
            }
            vt_[best * sP] += 1;
        }
        if constexpr (HAS_X) {
            PixelTerms<K> t;
            pixel_terms_core<K, STRICT, JOINT>(xv, d, inv2s2, invs2, lconst, t);
            double v = valid ? (double)(xv.w * t.ll_sum) : 0.0;
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((tid & 63) == 0) s_red[s & 1][tid >> 6] = v;
            __syncthreads();
            if (tid == 0) {
                double a = 0.0;
#pragma unroll
                for (int w = 0; w < PIX_BLOCK / 64; ++w) a += s_red[s & 1][w];
                part[((size_t)s * B + b) * gridDim.x + blockIdx.x] = a;
            }
        }
    }

    if (!valid) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) { pm_[c * sP] = pmean[c]; p2_[c * sP] = pm2[c]; }
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < K; ++k) { mm_[k * sP] = mmean[k]; m2_[k * sP] = mm2[k]; vt_[k * sP] = vt[k]; }
    }
}

// ll[i] = (float) sum_blk part[i][blk] in block order, i = (sample of the launch, image): one thread per value
__global__ __launch_bounds__(256)
void predictive_ll_kernel(const double* __restrict__ part, int nblk, int n, float* __restrict__ ll)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    for (int j = 0; j < nblk; ++j) v += part[(size_t)i * nblk + j];
    ll[i] = (float)v;
}

// z[s][n][l] = mean + exp(logvar / 2) * eps[s][n][l] for the n_s samples of a chunk: dec_v_kernel's expression (and this file is compiled
// with the same contraction setting), so z_s is what iodine_elbo leaves in buf.z for eps_s.  post_stride = L: a posterior (rows, L);
// 0: the initial posterior init_mean / init_logvar (L), the same for every row.
__global__ __launch_bounds__(256)
void predictive_sample_kernel(const float* __restrict__ pm, const float* __restrict__ plv, const float* __restrict__ eps,
                              float* __restrict__ z, size_t rows, int L, int post_stride, size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = (i / L) % rows;
        const int l = (int)(i % L);
        const size_t j = r * post_stride + l;
        z[i] = pm[j] + expf(0.5f * plv[j]) * eps[i];
    }
}

#define FOR_EACH_K(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

int predictive_blocks_per_image(int P) { return (P + PIX_BLOCK - 1) / PIX_BLOCK; }

hipError_t launch_predictive_sample(hipStream_t st, const float* pm, const float* plv, const float* eps, float* z, int n_s, int rows, int L,
                                    int post_stride)
{
    const size_t total = (size_t)n_s * rows * L;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(predictive_sample_kernel, dim3(blocks), dim3(256), 0, st, pm, plv, eps, z, (size_t)rows, L, post_stride, total);
    return hipGetLastError();
}

// dec [n_s B K][P][4] of samples s0 .. s0 + n_s - 1 (sample-major); the five state buffers (B,3,P) x 2, (B,K,P) x 2, int (B,K,P) are all
// required (read when s0 > 0, written always).  x4 (B,P,4) = NULL: no likelihood; else part = n_s B predictive_blocks_per_image(P) doubles
// of scratch and ll = n_s B floats, the chunk's rows of ll (S,B).
hipError_t launch_predictive_accum(hipStream_t st, const float* dec, const float* x4, int B, int K, int P, int s0, int n_s, float* pred_mean,
                                   float* pred_m2, float* mask_mean, float* mask_m2, int* votes, double* part, float* ll, float sigma,
                                   int strict, int joint)
{
    if (!pred_mean || !pred_m2 || !mask_mean || !mask_m2 || !votes || n_s < 1 || s0 < 0 || B < 1 || B > 65535) return hipErrorInvalidValue;
    if (x4 && (!part || !ll)) return hipErrorInvalidValue;
    const int nblk = predictive_blocks_per_image(P);
    const dim3 grid(nblk, B);
    const float inv2s2 = 1.f / (2.f * sigma * sigma), invs2 = 1.f / (sigma * sigma);
    const float lconst = (float)(-log((double)sigma) - 0.5 * log(2.0 * M_PI));
    switch (K) {
#define PA(KK, ST, HX, JT) hipLaunchKernelGGL((predictive_accum_kernel<KK, ST, HX, JT>), grid, dim3(PIX_BLOCK), 0, st, (const float4*)dec, \
        (const float4*)x4, B, P, s0, n_s, pred_mean, pred_m2, mask_mean, mask_m2, votes, part, inv2s2, invs2, lconst)
#define CASE(KK) case KK: \
        if (!x4) PA(KK, false, false, false); \
        else if (joint) { if (strict) PA(KK, true, true, true); else PA(KK, false, true, true); } \
        else { if (strict) PA(KK, true, true, false); else PA(KK, false, true, false); } \
        break;
        FOR_EACH_K(CASE)
#undef CASE
#undef PA
        default: return hipErrorInvalidValue;
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (x4) {
        const int n = n_s * B;
        hipLaunchKernelGGL(predictive_ll_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const double*)part, nblk, n, ll);
    }
    return hipGetLastError();
}
