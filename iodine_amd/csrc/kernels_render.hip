// Backward of the rendering step of IODINE.decode (lib/modeling/iodine.py:59-71) for arbitrary upstream gradients, and the product
// that turns the broadcast layer's class sums into d / dz - the two pieces in front of / behind decoder_backward_data when a single
// decode(z) or elbo(x) is differentiated (iodine_decode_backward / iodine_elbo_backward).
//
//   mean = sigmoid(rgb), mask = softmax_k(logit), pred = sum_k mask_k * mean_k          (iodine.py:64-70, 185)
//
// With G_pred, G_mask, G_mean the caller's gradients wrt (pred, mask, mean), mu = sigmoid(o), m = softmax_k(logit):
//   d mu_kc    = G_mean_kc + G_pred_c * m_k                   d o_kc     = d mu_kc * mu_kc * (1 - mu_kc)
//   d m_k      = G_mask_k + sum_c G_pred_c * mu_kc            d logit_k  = m_k * (d m_k - sum_j m_j * d m_j) + G_logit_k
// (G_logit: a gradient on the mask logits themselves, self.mask_logits of iodine.py:185 - the auxiliary cotangents of
// iodine_train_backward_aux; it adds behind the softmax backward, so a NULL G_logit leaves every bit as it was.)
// One thread owns one pixel and keeps all K slots of it in registers, like the other per-pixel kernels.  HBM-bound: 16 B of decoder
// output + up to 4 + 4 + 12 / K B of upstream planes in, 16 B out per slot-pixel.  Lane i of a wave handles pixel p0 + i: the NCHW
// planes of the caller are read 4 B per lane at consecutive addresses (256 B per wave and plane), the NHWC4 decoder output and the
// result as 16 B per lane at consecutive addresses (1 KiB per wave instruction).
#include "common.h"

#include "pixel_terms.h"

#define RND_BLOCK 256

template <int K, bool STRICT>
__global__ __launch_bounds__(RND_BLOCK)
void render_bwd_kernel(const float4* __restrict__ dec, const float* __restrict__ g_pred, const float* __restrict__ g_mask,
                       const float* __restrict__ g_mean, const float* __restrict__ g_logits, float4* __restrict__ g, int P)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * RND_BLOCK + threadIdx.x;
    if (p >= P) return;
    const float4* dec_b = dec + (size_t)b * K * P;
    float4* g_b = g + (size_t)b * K * P;
    // mu and m recomputed as the forward forms them: max-subtracted softmax like F.softmax.  Bit-identical to what decode returned only
    // with STRICT (conv_precision 0): final_out_kernel always uses libm expf + IEEE division, and so does STRICT here; the default path
    // uses v_exp_f32 / v_rcp_f32 on the bounded arguments as pixel_terms.h does (relative error <= |x| 2^-24 + 1 ulp, far inside the gates)
    float mu[K][3], m[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float4 d = dec_b[(size_t)k * P + p];
        mu[k][0] = pt_sigmoid<STRICT>(d.x); mu[k][1] = pt_sigmoid<STRICT>(d.y); mu[k][2] = pt_sigmoid<STRICT>(d.z);
        m[k] = d.w;
        mx = fmaxf(mx, d.w);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { m[k] = pt_exp_bounded<STRICT>(m[k] - mx); den += m[k]; }
    const float rden = pt_rcp<STRICT>(den);
    float gp[3] = {0.f, 0.f, 0.f};
    if (g_pred)
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[c] = g_pred[((size_t)b * 3 + c) * P + p];
    float dm[K], mdm = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        m[k] *= rden;
        dm[k] = (g_mask ? g_mask[((size_t)b * K + k) * P + p] : 0.f) + ((gp[0] * mu[k][0] + gp[1] * mu[k][1]) + gp[2] * mu[k][2]);
        mdm += m[k] * dm[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float dmu = (g_mean ? g_mean[(((size_t)b * K + k) * 3 + c) * P + p] : 0.f) + gp[c] * m[k];
            o[c] = dmu * mu[k][c] * (1.f - mu[k][c]);
        }
        // one slot: the softmax is the constant 1, its gradient exactly 0 (not the rounding residue of dm - 1 * dm)
        float dl = K == 1 ? 0.f : m[k] * (dm[k] - mdm);
        if (g_logits) dl += g_logits[((size_t)b * K + k) * P + p];
        g_b[(size_t)k * P + p] = make_float4(o[0], o[1], o[2], dl);
    }
}

#define FOR_EACH_K(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

hipError_t launch_render_bwd_logits(hipStream_t st, const float* dec, const float* g_pred, const float* g_mask, const float* g_mean,
                                    const float* g_logits, float* g, int B, int K, int P, int strict)
{
    if (!dec || !g || B < 1 || P < 1) return hipErrorInvalidValue;
    const dim3 grid((P + RND_BLOCK - 1) / RND_BLOCK, B);
    switch (K) {
#define CASE(KK) case KK: \
        if (strict) hipLaunchKernelGGL((render_bwd_kernel<KK, true>), grid, dim3(RND_BLOCK), 0, st, (const float4*)dec, g_pred, g_mask, g_mean, g_logits, (float4*)g, P); \
        else hipLaunchKernelGGL((render_bwd_kernel<KK, false>), grid, dim3(RND_BLOCK), 0, st, (const float4*)dec, g_pred, g_mask, g_mean, g_logits, (float4*)g, P); \
        break;
        FOR_EACH_K(CASE)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_render_bwd(hipStream_t st, const float* dec, const float* g_pred, const float* g_mask, const float* g_mean, float* g,
                             int B, int K, int P, int strict)
{
    return launch_render_bwd_logits(st, dec, g_pred, g_mask, g_mean, nullptr, g, B, K, P, strict);
}

// -----------------------------------------------------------------------------------------------
// dz[n][l] = sum_j Rc[n][j] * wclsT[j][l], j < 9 C: the class sums of d(pre-activation 0) through the broadcast layer's latent weights
// (what dz_latent_kernel computes in front of its KL / layer-norm terms, which a single differentiated pass does not want).
//   pm == NULL:  dz_out[n][l] = dz                                                                     (iodine_decode_backward)
//   otherwise:   g_pm  = scale * (dz - beta mu)                                                        (iodine_elbo_backward: scale = 1 / B,
//                g_plv = scale * (dz * 1/2 exp(logvar / 2) * eps - beta 1/2 (exp(logvar) - 1))          the batch mean of iodine.py:193,220;
//                                                                                                       beta: the objective's KL weight)
// One block per slot; blockDim = NS * Lp (Lp = L rounded up to 64): the contraction is cut into NS slices with four independent partial
// sums each, combined in fixed order.
// the contraction, shared by the two kernels below: s_rc = 9 * C class sums of slot n, then NS * Lp partial sums; the result is valid in
// the threads of slice 0 with l < L (the others must not use it)
IOD_DEVINL float dz_contract(const float* __restrict__ Rc, const float* __restrict__ wclsT, int L, int C, float* s_rc)
{
    const int n = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const int Lp = (L + 63) / 64 * 64, NS = nth / Lp, l = tid % Lp, slice = tid / Lp, J = 9 * C;
    float* s_dz = s_rc + J;
    for (int i = tid; i < J; i += nth) s_rc[i] = Rc[(size_t)n * J + i];
    __syncthreads();
    {
        const int per = (J + NS - 1) / NS, j0 = slice * per, j1 = min(J, j0 + per);
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (l < L) {
            const float* w = wclsT + l;
            int j = j0;
            for (; j + 3 < j1; j += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = fmaf(s_rc[j + q], w[(size_t)(j + q) * L], a[q]);
            }
            for (; j < j1; ++j) a[0] = fmaf(s_rc[j], w[(size_t)j * L], a[0]);
        }
        s_dz[slice * Lp + l] = (a[0] + a[1]) + (a[2] + a[3]);
    }
    __syncthreads();
    float dz = 0.f;
    if (slice == 0 && l < L)
        for (int q = 0; q < NS; ++q) dz += s_dz[q * Lp + l];
    return dz;
}

__global__ void dz_plain_kernel(const float* __restrict__ Rc, const float* __restrict__ wclsT, int L, int C, float* __restrict__ dz_out,
                                const float* __restrict__ pm, const float* __restrict__ plv, const float* __restrict__ eps, float scale,
                                float* __restrict__ g_pm, float* __restrict__ g_plv, float beta)
{
    extern __shared__ float s_rc[];                     // 9 * C, then NS * Lp partial sums
    const int n = blockIdx.x, Lp = (L + 63) / 64 * 64, l = threadIdx.x % Lp, slice = threadIdx.x / Lp;
    const float dz = dz_contract(Rc, wclsT, L, C, s_rc);
    if (slice != 0 || l >= L) return;
    const size_t i = (size_t)n * L + l;
    if (!pm) { dz_out[i] = dz; return; }
    const float mu = pm[i], lv = plv[i];
    if (beta == 1.f) {                                      // (uniform) the default keeps its expression as it was
        g_pm[i] = scale * (dz - mu);
        g_plv[i] = scale * (dz * 0.5f * expf(0.5f * lv) * eps[i] - 0.5f * (expf(lv) - 1.f));
    } else {
        g_pm[i] = scale * (dz - beta * mu);
        g_plv[i] = scale * (dz * 0.5f * expf(0.5f * lv) * eps[i] - beta * (0.5f * (expf(lv) - 1.f)));
    }
}

hipError_t launch_dz_plain(hipStream_t st, const float* Rc, const float* wclsT, int N, int L, int C, float* dz_out, const float* pm,
                           const float* plv, const float* eps, float scale, float* g_pm, float* g_plv, float beta)
{
    const int Lp = (L + 63) / 64 * 64;
    if (Lp > 512 || N < 1 || (pm ? (!plv || !eps || !g_pm || !g_plv) : !dz_out)) return hipErrorInvalidValue;
    const int nth = (512 / Lp) * Lp;
    hipLaunchKernelGGL(dz_plain_kernel, dim3(N), dim3(nth), (9 * C + nth) * sizeof(float), st, Rc, wclsT, L, C, dz_out, pm, plv, eps, scale,
                       g_pm, g_plv, beta);
    return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------
// Seeds of the head's back-propagation through time from cotangents on the FINAL evaluation of a training forward
// (iodine_train_backward_aux; iodine.py:171-187,642-651).  z_T = mu_T + exp(logvar_T / 2) eps_T and lambda_T = detach(lambda_{T-1}) + delta_{T-1}:
//   dz       = Rc . wclsT (the decoder pass of the cotangents on mean / mask / mask_logits; Rc == NULL: none) + c_z
//   seed_m   = dz + c_pm                                         = d / d delta_mean_{T-1}
//   seed_v   = dz * 1/2 exp(logvar_T / 2) eps_T + c_plv          = d / d delta_logvar_{T-1}
// No KL term: the final ELBO's KL is part of the loss.  The forward keeps z_T and mu_T, not the caller's noise:
// exp(logvar_T / 2) eps_T is read back as z_T - mu_T.  The subtraction is exact to the rounding of z_T, so seed_v carries an absolute error
// of at most 2^-25 |z_T| |dz| - negligible beside seed_m = dz - but RELATIVE to the term itself that is 2^-24 |z_T| / (sigma_T |eps_T|):
// the cancellation loses about log2(|mu_T| / sigma_T) bits (sigma = 0.01, |mu| = 3: ~2e-5 relative on the dz part of d logvar_T).
// Keeping the noise instead would cost the plain training forward a copy per step.
// One launch over N * L: the block layout of dz_plain_kernel.
// The same for any evaluation i of the forward (iodine_train_backward_frames), one launch per evaluation right behind its decoder pass:
// z = z_i, pm = mu_i with row stride ldpm (the forward keeps lambda_i as the first L of the 4 L entries of a row of its saved refinement
// input), seeds = d / d delta_{i-1}.  c_z2 / c_pm2 / c_plv2: a second, optional set of cotangents on the same evaluation, added behind the
// first (evaluation T named both as the final state and as an attached frame); all NULL and ldpm = L is the launch as it was.
__global__ void latent_seed_kernel(const float* __restrict__ Rc, const float* __restrict__ wclsT, int L, int C, const float* __restrict__ c_z,
                                   const float* __restrict__ c_pm, const float* __restrict__ c_plv, const float* __restrict__ z,
                                   const float* __restrict__ pm, float* __restrict__ seed_m, float* __restrict__ seed_v, int ldpm,
                                   const float* __restrict__ c_z2, const float* __restrict__ c_pm2, const float* __restrict__ c_plv2)
{
    extern __shared__ float s_rc[];
    const int n = blockIdx.x, Lp = (L + 63) / 64 * 64, l = threadIdx.x % Lp, slice = threadIdx.x / Lp;
    float dz = Rc ? dz_contract(Rc, wclsT, L, C, s_rc) : 0.f;          // (Rc is uniform over the grid: every thread meets the barriers)
    if (slice != 0 || l >= L) return;
    const size_t i = (size_t)n * L + l;
    if (c_z) dz += c_z[i];
    if (c_z2) dz += c_z2[i];
    float sm = dz + (c_pm ? c_pm[i] : 0.f);
    float sv = dz * 0.5f * (z[i] - pm[(size_t)n * ldpm + l]) + (c_plv ? c_plv[i] : 0.f);
    if (c_pm2) sm += c_pm2[i];
    if (c_plv2) sv += c_plv2[i];
    seed_m[i] = sm;
    seed_v[i] = sv;
}

hipError_t launch_latent_seed(hipStream_t st, const float* Rc, const float* wclsT, int N, int L, int C, const float* c_z, const float* c_pm,
                              const float* c_plv, const float* z, const float* pm, float* seed_m, float* seed_v, int ldpm, const float* c_z2,
                              const float* c_pm2, const float* c_plv2)
{
    const int Lp = (L + 63) / 64 * 64;
    if (ldpm <= 0) ldpm = L;
    if (Lp > 512 || N < 1 || !z || !pm || !seed_m || !seed_v || (Rc && !wclsT) || ldpm < L) return hipErrorInvalidValue;
    const int nth = (512 / Lp) * Lp;
    hipLaunchKernelGGL(latent_seed_kernel, dim3(N), dim3(nth), (9 * C + nth) * sizeof(float), st, Rc, wclsT, L, C, c_z, c_pm, c_plv, z, pm,
                       seed_m, seed_v, ldpm, c_z2, c_pm2, c_plv2);
    return hipGetLastError();
}
