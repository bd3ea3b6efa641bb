// Matching slots to ground-truth masks (include/iodine_hip.h: iodine_mask_overlap, iodine_assign, iodine_mask_match,
// iodine_mask_match_backward).  Stateless like kernels_objects.hip: no handle, no workspace, NCHW fp32 masks and uint8 0/1 ground truth in.
// A training step runs three launches: one per-pixel pass (statistics), one tiny pass (costs, assignment, loss, backward coefficients),
// one per-pixel pass (gradient).
//
// mask_overlap_kernel: one block per (image b, slot k), so every mask plane is read from HBM once; its 1024 threads stride the plane in
// 16-byte vectors and read the G ground-truth planes of their pixels (K - 1 of the K reads of a gt plane are meant to come from L2: the
// block-id remap of slot_table_kernel puts the blocks of one image on one XCD, speed only).  Every term - m, gt * m, -gt * logf(m + eps) -
// is an exact fp32 number converted to fp64 and added in fp64: per thread in loop order, per wave in a fixed xor butterfly, across the 16
// waves in index order.  No atomics, no scratch buffer: the same input gives the same bits.  logf is the accurate one (1 ulp).
//
// mask_match_kernel / assign_kernel: one wave per image.  The lanes fill the (G x K) cost in LDS, lane 0 runs iod_assign_solve (assign.h:
// loops bounded by G and K, non-finite costs refused before the search) and derives the loss and the per-row coefficients.
//
// mask_match_bwd_kernel: elementwise over (b, k, p); a slot that is no row's match gets zeros.  `assign` is only ever compared, never used
// as an index.
#include "common.h"
#include "assign.h"

static constexpr int MT_THREADS = 1024;
static constexpr int MT_WAVES = MT_THREADS / 64;
static constexpr int MT_MAX = IOD_ASSIGN_MAX;               // slots and gt rows per image
static constexpr int MT_BWD_THREADS = 256;

// W = 4: P % 4 == 0, mask 16-byte and gt 4-byte aligned (launch_mask_overlap decides); W = 1: anything.
template <int W>
__global__ __launch_bounds__(MT_THREADS)
void mask_overlap_kernel(const float* __restrict__ mask, const unsigned char* __restrict__ gt, int K, int G, int P, float eps,
                         float* __restrict__ inter, float* __restrict__ nll, float* __restrict__ mask_area, int* __restrict__ gt_area)
{
    __shared__ double s_d[MT_WAVES][2 * MT_MAX + 1];
    __shared__ unsigned s_n[MT_WAVES][MT_MAX];

    // blocks id, id + 8, ... share an XCD: a contiguous run of (b, k) per group (slot_table_kernel's bijection; placement changes speed only)
    const int n = gridDim.x, id = blockIdx.x;
    const int xg = id & 7, q = n >> 3, r = n & 7;
    const int w = (xg < r ? xg * (q + 1) : r * (q + 1) + (xg - r) * q) + (id >> 3);
    const int b = w / K, k = w - b * K;
    const int tid = threadIdx.x;

    const float* mk = mask + ((size_t)b * K + k) * P;
    const unsigned char* gb = gt + (size_t)b * G * P;
    const bool want_nll = nll != nullptr;

    double a_area = 0.0, a_i[MT_MAX], a_n[MT_MAX];
    unsigned cnt[MT_MAX];
#pragma unroll
    for (int g = 0; g < MT_MAX; ++g) { a_i[g] = 0.0; a_n[g] = 0.0; cnt[g] = 0; }

    const int nvec = P / W;                                   // W == 4 only where P % 4 == 0
    for (int v = tid; v < nvec; v += MT_THREADS) {
        const int p0 = v * W;
        float m[W], l[W];
        if constexpr (W == 4) {
            const float4 t = *reinterpret_cast<const float4*>(mk + p0);
            m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
        } else {
            m[0] = mk[p0];
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            l[j] = want_nll ? -logf(m[j] + eps) : 0.f;
            a_area += (double)m[j];
        }
#pragma unroll
        for (int g = 0; g < MT_MAX; ++g) {
            if (g < G) {                                      // (uniform)
                unsigned bits;
                if constexpr (W == 4) bits = *reinterpret_cast<const unsigned*>(gb + (size_t)g * P + p0);
                else bits = gb[(size_t)g * P + p0];
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const bool on = ((bits >> (8 * j)) & 255u) != 0u;
                    a_i[g] += on ? (double)m[j] : 0.0;
                    a_n[g] += on ? (double)l[j] : 0.0;
                    cnt[g] += on ? 1u : 0u;
                }
            }
        }
    }

    // wave step: fixed butterflies; block step: one thread per column, waves in index order
    const int wv = tid >> 6;
    a_area = wave_sum(a_area);
#pragma unroll
    for (int g = 0; g < MT_MAX; ++g) {
        if (g < G) {
            a_i[g] = wave_sum(a_i[g]);
            a_n[g] = wave_sum(a_n[g]);
            cnt[g] = wave_sum(cnt[g]);
            if ((tid & 63) == 0) { s_d[wv][g] = a_i[g]; s_d[wv][MT_MAX + g] = a_n[g]; s_n[wv][g] = cnt[g]; }
        }
    }
    if ((tid & 63) == 0) s_d[wv][2 * MT_MAX] = a_area;
    __syncthreads();
    if (tid <= 2 * MT_MAX) {
        const int g = tid & (MT_MAX - 1);
        const bool is_area = tid == 2 * MT_MAX;
        if (is_area || g < G) {
            double d = 0.0;
#pragma unroll 1
            for (int i = 0; i < MT_WAVES; ++i) d += s_d[i][tid];
            if (is_area) mask_area[(size_t)b * K + k] = (float)d;
            else if (tid < MT_MAX) inter[((size_t)b * G + g) * K + k] = (float)d;
            else if (want_nll) nll[((size_t)b * G + g) * K + k] = (float)d;
        }
    } else if (k == 0 && tid >= 64 && tid < 64 + G) {
        const int g = tid - 64;
        unsigned c = 0;
#pragma unroll 1
        for (int i = 0; i < MT_WAVES; ++i) c += s_n[i][g];
        gt_area[(size_t)b * G + g] = (int)c;
    }
}

hipError_t launch_mask_overlap(hipStream_t st, const float* mask, const unsigned char* gt, int B, int K, int G, int S, float eps,
                               float* inter, float* nll, float* mask_area, int* gt_area)
{
    if (K < 1 || K > MT_MAX || G < 1 || G > MT_MAX) return hipErrorInvalidValue;       // the register and LDS tables are 16 wide
    const int P = S * S;
    const bool vec = P % 4 == 0 && ((uintptr_t)mask & 15) == 0 && ((uintptr_t)gt & 3) == 0;
    const unsigned grid = (unsigned)B * (unsigned)K;
    if (vec)
        hipLaunchKernelGGL(mask_overlap_kernel<4>, dim3(grid), dim3(MT_THREADS), 0, st, mask, gt, K, G, P, eps, inter, nll, mask_area, gt_area);
    else
        hipLaunchKernelGGL(mask_overlap_kernel<1>, dim3(grid), dim3(MT_THREADS), 0, st, mask, gt, K, G, P, eps, inter, nll, mask_area, gt_area);
    return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------
// Assignment of any (B, G, K) cost: one wave per image, the matrix staged in LDS, lane 0 solves.
// -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64)
void assign_kernel(const float* __restrict__ cost, const unsigned char* __restrict__ row_valid, int G, int K,
                   int* __restrict__ assign, float* __restrict__ total)
{
    __shared__ float s_cost[MT_MAX * MT_MAX];
    __shared__ unsigned char s_valid[MT_MAX];
    __shared__ int s_assign[MT_MAX];
    __shared__ IodAssignWork s_work;
    const int b = blockIdx.x, t = threadIdx.x;
    const int cells = G * K;                                  // <= 256
    for (int c = t; c < cells; c += 64) s_cost[c] = cost[(size_t)b * cells + c];
    if (t < G) s_valid[t] = row_valid ? (unsigned char)(row_valid[(size_t)b * G + t] != 0) : (unsigned char)1;
    __syncthreads();
    if (t == 0) {
        float tot;
        iod_assign_solve(s_cost, s_valid, G, K, s_assign, &tot, &s_work);
        total[b] = tot;
    }
    __syncthreads();
    if (t < G) assign[(size_t)b * G + t] = s_assign[t];
}

hipError_t launch_assign(hipStream_t st, const float* cost, const unsigned char* row_valid, int B, int G, int K, int* assign,
                         float* total)
{
    if (K < 1 || K > MT_MAX || G < 1 || G > MT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assign_kernel, dim3((unsigned)B), dim3(64), 0, st, cost, row_valid, G, K, assign, total);
    return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------
// Costs, assignment, per-image loss and backward coefficients from the statistics.  Every quantity is formed in fp64 from the fp32
// statistics and rounded to fp32 once.  kind 0 = 'iou': 1 - I / U, U = n + a - I; kind 1 = 'ce': N / n.  A padding row (n = 0) reads cost 0,
// iou 0, assign -1, coefficients 0.  coef [b][g] = {on, off}: d loss_b / d m_kp for k = assign[g] is on (x 1 / (m + eps) for 'ce') where
// gt = 1 and off where gt = 0.
// -----------------------------------------------------------------------------------------------
IOD_DEVINL double mt_pair(int kind, double I, double Nl, double a, double n)
{
    return kind == 0 ? 1.0 - I / (n + a - I) : Nl / n;
}

__global__ __launch_bounds__(64)
void mask_match_kernel(const float* __restrict__ inter, const float* __restrict__ nll, const float* __restrict__ mask_area,
                       const int* __restrict__ gt_area, int K, int G, int match_kind, int loss_kind, int* __restrict__ assign,
                       float* __restrict__ loss, float* __restrict__ coef, float* __restrict__ cost_out, float* __restrict__ iou_out)
{
    __shared__ float s_cost[MT_MAX * MT_MAX];
    __shared__ unsigned char s_valid[MT_MAX];
    __shared__ int s_assign[MT_MAX];
    __shared__ IodAssignWork s_work;
    const int b = blockIdx.x, t = threadIdx.x;
    const int cells = G * K;
    const float* ib = inter + (size_t)b * cells;
    const float* nb = nll ? nll + (size_t)b * cells : nullptr;
    const float* ab = mask_area + (size_t)b * K;
    const int* gb = gt_area + (size_t)b * G;
    for (int c = t; c < cells; c += 64) {
        const int g = c / K, k = c - g * K;
        const int n = gb[g];
        const double I = (double)ib[c], Nl = nb ? (double)nb[c] : 0.0, a = (double)ab[k];
        const float cv = n > 0 ? (float)mt_pair(match_kind, I, Nl, a, (double)n) : 0.f;
        s_cost[c] = cv;
        if (cost_out) cost_out[(size_t)b * cells + c] = cv;
        if (iou_out) iou_out[(size_t)b * cells + c] = n > 0 ? (float)(I / ((double)n + a - I)) : 0.f;
    }
    if (t < G) s_valid[t] = (unsigned char)(gb[t] > 0);
    __syncthreads();
    if (t == 0) {
        float tot;
        const int M = iod_assign_solve(s_cost, s_valid, G, K, s_assign, &tot, &s_work);
        double sum = 0.0;
        for (int g = 0; g < G; ++g) {
            const int k = s_assign[g];
            float on = 0.f, off = 0.f;
            if (k >= 0 && k < K) {
                const int c = g * K + k;
                const double n = (double)gb[g], I = (double)ib[c], Nl = nb ? (double)nb[c] : 0.0, a = (double)ab[k];
                sum += mt_pair(loss_kind, I, Nl, a, n);
                if (loss_kind == 0) {
                    const double U = n + a - I;
                    on = (float)(-1.0 / ((double)M * U));
                    off = (float)(I / ((double)M * U * U));
                } else {
                    on = (float)(-1.0 / ((double)M * n));
                }
            }
            coef[((size_t)b * G + g) * 2] = on;
            coef[((size_t)b * G + g) * 2 + 1] = off;
        }
        loss[b] = M < 0 ? NAN : (M == 0 ? 0.f : (float)(sum / (double)M));
    }
    __syncthreads();
    if (t < G) assign[(size_t)b * G + t] = s_assign[t];
}

hipError_t launch_mask_match(hipStream_t st, const float* inter, const float* nll, const float* mask_area, const int* gt_area, int B,
                             int K, int G, int match_kind, int loss_kind, int* assign, float* loss, float* coef, float* cost_out,
                             float* iou_out)
{
    if (K < 1 || K > MT_MAX || G < 1 || G > MT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_match_kernel, dim3((unsigned)B), dim3(64), 0, st, inter, nll, mask_area, gt_area, K, G, match_kind,
                       loss_kind, assign, loss, coef, cost_out, iou_out);
    return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------
// Backward: grad_mask[b][k][p] = grad_loss[b] * (gt ? on (/ (m + eps) for 'ce') : off) of the row matched to slot k, 0 for a slot without
// one.  bx blocks per plane; every element of grad_mask is written.
// -----------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(MT_BWD_THREADS)
void mask_match_bwd_kernel(const float* __restrict__ mask, const unsigned char* __restrict__ gt, const int* __restrict__ assign,
                           const float* __restrict__ coef, const float* __restrict__ grad_loss, int K, int G, int P, int bx,
                           int loss_kind, float eps, float* __restrict__ grad)
{
    const int plane = blockIdx.x / bx, blk = blockIdx.x - plane * bx, tid = threadIdx.x;
    const int b = plane / K, k = plane - b * K;
    int g = -1;
    for (int i = G - 1; i >= 0; --i)
        if (assign[(size_t)b * G + i] == k) g = i;            // (uniform; the lowest such row, an injective map has one at the most)
    float on = 0.f, off = 0.f;
    if (g >= 0) {
        const float gl = grad_loss[b];
        on = gl * coef[((size_t)b * G + g) * 2];
        off = loss_kind == 0 ? gl * coef[((size_t)b * G + g) * 2 + 1] : 0.f;
    }
    const float* mk = mask + (size_t)plane * P;
    const unsigned char* gp = gt + ((size_t)b * G + (g >= 0 ? g : 0)) * P;
    float* out = grad + (size_t)plane * P;
    const int nvec = P / W;
    for (int v = blk * MT_BWD_THREADS + tid; v < nvec; v += bx * MT_BWD_THREADS) {
        const int p0 = v * W;
        float r[W];
        if (g < 0) {
#pragma unroll
            for (int j = 0; j < W; ++j) r[j] = 0.f;
        } else {
            float m[W];
            unsigned bits;
            if constexpr (W == 4) {
                const float4 t = *reinterpret_cast<const float4*>(mk + p0);
                m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
                bits = *reinterpret_cast<const unsigned*>(gp + p0);
            } else {
                m[0] = mk[p0];
                bits = gp[p0];
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const bool hit = ((bits >> (8 * j)) & 255u) != 0u;
                r[j] = hit ? (loss_kind == 0 ? on : on / (m[j] + eps)) : off;
            }
        }
        if constexpr (W == 4) *reinterpret_cast<float4*>(out + p0) = make_float4(r[0], r[1], r[2], r[3]);
        else out[p0] = r[0];
    }
}

hipError_t launch_mask_match_bwd(hipStream_t st, const float* mask, const unsigned char* gt, const int* assign, const float* coef,
                                 const float* grad_loss, int B, int K, int G, int S, int loss_kind, float eps, float* grad)
{
    if (K < 1 || K > MT_MAX || G < 1 || G > MT_MAX) return hipErrorInvalidValue;
    const int P = S * S;
    const bool vec = P % 4 == 0 && ((uintptr_t)mask & 15) == 0 && ((uintptr_t)grad & 15) == 0 && ((uintptr_t)gt & 3) == 0;
    const int per = MT_BWD_THREADS * (vec ? 4 : 1) * 4;       // about four vectors per thread
    const int bx = std::max(1, std::min((P + per - 1) / per, 64));
    const unsigned grid = (unsigned)B * (unsigned)K * (unsigned)bx;
    if (vec)
        hipLaunchKernelGGL(mask_match_bwd_kernel<4>, dim3(grid), dim3(MT_BWD_THREADS), 0, st, mask, gt, assign, coef, grad_loss, K, G, P,
                           bx, loss_kind, eps, grad);
    else
        hipLaunchKernelGGL(mask_match_bwd_kernel<1>, dim3(grid), dim3(MT_BWD_THREADS), 0, st, mask, gt, assign, coef, grad_loss, K, G, P,
                           bx, loss_kind, eps, grad);
    return hipGetLastError();
}
