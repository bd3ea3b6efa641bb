// Training-only kernels: column sums (bias gradients, partial-row reductions) and the two SGEMMs - the small dense
// algebra of the refinement head's backward and of the broadcast layer's latent-channel weight gradient.
#include "common.h"

// dst[c] += alpha * sum_r src[r][c]   (bias gradients, init_mean / init_logvar gradients, partial-bias reduction)
__global__ void colsum_kernel(const float* __restrict__ src, int rows, int cols, int ld, float alpha, float* __restrict__ dst)
{
    __shared__ float s_red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int r = tid; r < rows; r += 256) s += src[(size_t)r * ld + c];
    s_red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) dst[c] += alpha * s_red[0];
}

hipError_t launch_colsum(hipStream_t st, const float* src, int rows, int cols, int ld, float alpha, float* dst)
{
    IOD_XSKIP(1);
    hipLaunchKernelGGL(colsum_kernel, dim3(cols), dim3(256), 0, st, src, rows, cols, ld, alpha, dst);
    return hipGetLastError();
}

// column sums of a tall matrix (rows ~ 1e6, cols <= 256, cols % 4 == 0, contiguous): coalesced float4 streaming,
// one partial row per block, then the small column-sum kernel over the partials (fixed order -> deterministic).
__global__ __launch_bounds__(256)
void colsum_tall_partial_kernel(const float4* __restrict__ src, int rows, int c4, int rows_per_block,
                                float4* __restrict__ partial)
{
    __shared__ float4 s_red[256];
    const int tid = threadIdx.x;
    const int rl = 256 / c4;                               // row lanes
    const int c = tid % c4, r0 = tid / c4;
    const int rbeg = blockIdx.x * rows_per_block, rend = min(rows, rbeg + rows_per_block);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 < rl)
        for (int r = rbeg + r0; r < rend; r += rl) {
            const float4 v = src[(size_t)r * c4 + c];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    s_red[tid] = s;
    __syncthreads();
    if (tid < c4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < rl; ++j) { const float4 v = s_red[j * c4 + tid]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        partial[(size_t)blockIdx.x * c4 + tid] = t;
    }
}

hipError_t launch_colsum_tall(hipStream_t st, const float* src, int rows, int cols, float alpha, float* dst, float* tmp,
                              size_t tmp_elems)
{
    if (cols % 4 != 0 || cols > 256 || 256 % (cols / 4) != 0 || rows < 8192) return launch_colsum(st, src, rows, cols, cols, alpha, dst);
    int nblk = (int)std::min<size_t>(448, tmp_elems / cols);
    if (nblk < 1) return hipErrorInvalidValue;
    const int rpb = (rows + nblk - 1) / nblk;
    nblk = (rows + rpb - 1) / rpb;
    hipLaunchKernelGGL(colsum_tall_partial_kernel, dim3(nblk), dim3(256), 0, st, (const float4*)src, rows, cols / 4, rpb,
                       (float4*)tmp);
    return launch_colsum(st, tmp, nblk, cols, cols, alpha, dst);
}

// =========================================================================================
// generic small SGEMM (row-major): C[M][N] = alpha * op(A)[M][K] * op(B)[K][N] + beta * C, 16x16 LDS tiles.
// Used for the head backward (N = B*K rows; at most a few hundred MFLOP per call).
// =========================================================================================
template <int BK>
__global__ __launch_bounds__(256)
void sgemm_kernel(int ta, int tb, int M, int N, int K, float alpha, const float* __restrict__ A, int lda,
                  const float* __restrict__ B, int ldb, float beta, float* __restrict__ Cm, int ldc)
{
    // These GEMMs are latency-bound (operands are L2-resident, a few hundred blocks): K advances BK = 64 at a time so that every
    // thread has 8 independent loads in flight per barrier pair instead of 2, and 256 at a time (32 loads, four float4 per
    // operand) for the long reductions (K >= 512: 16 -> 4 exposed round trips at K = 1024); the k order of the fma chain is
    // unchanged, so every BK gives the same bits.
    __shared__ float sA[16][BK + 1], sB[BK][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int row = blockIdx.y * 16 + ty, col = blockIdx.x * 16 + tx;
    float acc = 0.f;
    // operand tiles are fetched as float4 along their contiguous dimension when the leading dimensions allow it (16-byte
    // loads: a quarter of the instructions, full rate of the texture path); scalar loads otherwise / at the edges
    const int t = threadIdx.x;
    const bool vec_ok = !tb && (lda & 3) == 0 && (ldb & 3) == 0 && (K & 3) == 0 && (M & 3) == 0 && (N & 3) == 0 &&
                        (((size_t)A | (size_t)B) & 15) == 0;
    for (int k0 = 0; k0 < K; k0 += BK) {
        if (vec_ok) {
            constexpr int NV = BK / 64;                      // float4 loads per thread and operand
            float4 va[NV], vb4[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                va[q] = vb4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!ta) {                                   // A [M][K]: 16 rows x 64 k per pass, float4 along k
                    const int r = t >> 4, kq = q * 64 + (t & 15) * 4, gr = blockIdx.y * 16 + r;
                    if (gr < M && k0 + kq < K) va[q] = *reinterpret_cast<const float4*>(A + (size_t)gr * lda + k0 + kq);
                } else {                                     // A [K][M]: 64 k x 16 rows per pass, float4 along m
                    const int kk = q * 64 + (t >> 2), gm = blockIdx.y * 16 + (t & 3) * 4;
                    if (k0 + kk < K && gm < M) va[q] = *reinterpret_cast<const float4*>(A + (size_t)(k0 + kk) * lda + gm);
                }
                {                                            // B [K][N]: 64 k x 16 columns per pass, float4 along n
                    const int kk = q * 64 + (t >> 2), gn = blockIdx.x * 16 + (t & 3) * 4;
                    if (k0 + kk < K && gn < N) vb4[q] = *reinterpret_cast<const float4*>(B + (size_t)(k0 + kk) * ldb + gn);
                }
            }
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                if (!ta) {
                    const int r = t >> 4, kq = q * 64 + (t & 15) * 4;
                    sA[r][kq] = va[q].x; sA[r][kq + 1] = va[q].y; sA[r][kq + 2] = va[q].z; sA[r][kq + 3] = va[q].w;
                } else {
                    const int kk = q * 64 + (t >> 2), mq = (t & 3) * 4;
                    sA[mq][kk] = va[q].x; sA[mq + 1][kk] = va[q].y; sA[mq + 2][kk] = va[q].z; sA[mq + 3][kk] = va[q].w;
                }
                const int kk = q * 64 + (t >> 2), nq = (t & 3) * 4;
                sB[kk][nq] = vb4[q].x; sB[kk][nq + 1] = vb4[q].y; sB[kk][nq + 2] = vb4[q].z; sB[kk][nq + 3] = vb4[q].w;
            }
        } else {
            float ra[BK / 16], rb[BK / 16];
#pragma unroll
            for (int q = 0; q < BK / 16; ++q) {
                const int ka = k0 + q * 16 + tx, kb = k0 + q * 16 + ty;
                ra[q] = (row < M && ka < K) ? (ta ? A[(size_t)ka * lda + row] : A[(size_t)row * lda + ka]) : 0.f;
                rb[q] = (kb < K && col < N) ? (tb ? B[(size_t)col * ldb + kb] : B[(size_t)kb * ldb + col]) : 0.f;
            }
#pragma unroll
            for (int q = 0; q < BK / 16; ++q) { sA[ty][q * 16 + tx] = ra[q]; sB[q * 16 + ty][tx] = rb[q]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BK; ++k) acc = fmaf(sA[ty][k], sB[k][tx], acc);
        __syncthreads();
    }
    if (row < M && col < N) {
        float* c = Cm + (size_t)row * ldc + col;
        *c = alpha * acc + (beta != 0.f ? beta * *c : 0.f);
    }
}

// ---- C[M][N] = alpha * A^T . B + beta * C for A [K][M], B [K][N] (the "sum of outer products over rows" shape of every weight gradient of the
// refinement head and of the broadcast layer's latent channels) on v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate.  Both
// operands are K-major, so a lane's operand element of MFMA step k is A[k + lane / 32][m0 + lane % 32]: 128 contiguous bytes per half wave,
// straight from global memory (L2-resident) into the operand register - no LDS, no transposes.  A wave owns a 32 x 32 tile of C;
//   * SPLITK = false: four tiles per block (the 1024 x 512 x 1120 LSTM gradient: 512 tiles; 16 x 16 scalar LDS tiles took 100 us);
//   * SPLITK = true: ONE tile per block, its four waves take a quarter of K each and are added in wave order through LDS (deterministic) -
//     for products with few tiles (64 x 256, K = 1120: 16 tiles).
// MODE 1 writes through the broadcast layer's index map: row = latent channel ci, column = tap * C + co -> gw[co][ci][tap] (ldc = L + 2).
// AROW: A is row-major [M][K] (lda = row stride) instead of K-major - lane i of a half wave reads row m0 + i: 32 cache lines per load
// instruction, 16 MFMA steps per line; for the LSTM gate pre-activations (A = the 224 x 768 head inputs, L1-resident).
template <bool SPLITK, int MODE, bool AROW>
__global__ __launch_bounds__(256)
void sgemm_tn_mfma_kernel(int M, int N, int K, float alpha, const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                          float beta, float* __restrict__ Cm, int ldc, int mode_c)
{
    __shared__ float s_red[SPLITK ? 3 * 1024 : 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tiles_n = N / 32, ntiles = (M / 32) * tiles_n;
    const int tile = SPLITK ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv;
    if (tile >= ntiles) return;                              // (wave-uniform; no barrier below unless SPLITK, where it is block-uniform)
    const int m0 = (tile / tiles_n) * 32, n0 = (tile % tiles_n) * 32;
    int k0 = 0, k1 = K;
    if (SPLITK) {
        const int per = ((K + 3) / 4 + 1) & ~1;              // even: a wave's range starts on an MFMA step
        k0 = min(K, wv * per); k1 = min(K, k0 + per);
    }
    const float* pa = AROW ? A + (size_t)(m0 + (lane & 31)) * lda : A + m0 + (lane & 31);
    const float* pb = B + n0 + (lane & 31);
    const int kh = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    constexpr int U = 32;                                    // MFMA steps per group: 2 U loads in flight under the previous group's MFMAs (U = 16:
                                                             // 1024 matrix cycles per group did not cover an L2 round trip under load - 61 us for the LSTM gradient)
    float a[U], b[U];
    auto fetch = [&](int k) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = k + 2 * u + kh;
            const int kc = min(kk, K - 1);                   // unconditional loads at a clamped row; rows past the range count as zero
            const float av = AROW ? pa[kc] : pa[(size_t)kc * lda], bv = pb[(size_t)kc * ldb];
            a[u] = kk < k1 ? av : 0.f; b[u] = bv;
        }
    };
    if (k0 < k1) fetch(k0);
    for (int k = k0; k < k1; k += 2 * U) {
        float ca[U], cb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { ca[u] = a[u]; cb[u] = b[u]; }
        if (k + 2 * U < k1) fetch(k + 2 * U);
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[u], cb[u], acc, 0, 0, 0);
    }
    if (SPLITK) {
        // waves 1 - 3 hand their partial tiles to wave 0: [wave - 1][reg][lane], added in wave order
        if (wv > 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s_red[(wv - 1) * 1024 + i * 64 + lane] = acc[i];
        }
        __syncthreads();
        if (wv > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += s_red[w * 1024 + i * 64 + lane];
    }
    const int col = n0 + (lane & 31);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * kh;
        float* c;
        if (MODE == 1) { const int tap = col / mode_c, co = col % mode_c; c = Cm + ((size_t)co * ldc + row) * 9 + tap; }
        else c = Cm + (size_t)row * ldc + col;
        *c = alpha * acc[i] + (beta != 0.f ? beta * *c : 0.f);
    }
}

bool sgemm_tn_mfma_ok(int M, int N, int K) { return M % 32 == 0 && N % 32 == 0 && K >= 1; }

// mode 0: C row-major [M][ldc]; mode 1: the broadcast-layer map (see above), mode_c = C channels, ldc = L + 2
hipError_t launch_sgemm_tn_mfma(hipStream_t st, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                                float beta, float* C, int ldc, int mode, int mode_c, int a_rowmajor)
{
    IOD_XSKIP(2);
    if (!sgemm_tn_mfma_ok(M, N, K) || (mode == 1 && (mode_c < 1 || N != 9 * mode_c))) return hipErrorInvalidValue;
    const int ntiles = (M / 32) * (N / 32);
    // (two waves per SIMD at 512 tiles: one computes while the other waits.  Row-major A = per-slot rows of the refinement head: the summation
    //  order must not depend on how many slots share the launch - a slot's result is the same bits in every batch - so always split)
    const bool splitk = (a_rowmajor || ntiles <= 512) && K >= 64;
#define TN_LAUNCH(SK, MD, AR, GRID) hipLaunchKernelGGL((sgemm_tn_mfma_kernel<SK, MD, AR>), dim3(GRID), dim3(256), 0, st, M, N, K, alpha, A, lda, B, \
                                                       ldb, beta, C, ldc, mode_c)
    if (a_rowmajor) {
        if (mode != 0) return hipErrorInvalidValue;
        if (splitk) TN_LAUNCH(true, 0, true, ntiles); else TN_LAUNCH(false, 0, true, (ntiles + 3) / 4);
    } else if (splitk) { if (mode == 1) TN_LAUNCH(true, 1, false, ntiles); else TN_LAUNCH(true, 0, false, ntiles); }
    else { if (mode == 1) TN_LAUNCH(false, 1, false, (ntiles + 3) / 4); else TN_LAUNCH(false, 0, false, (ntiles + 3) / 4); }
#undef TN_LAUNCH
    return hipGetLastError();
}

hipError_t launch_sgemm(hipStream_t st, int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda,
                        const float* B, int ldb, float beta, float* C, int ldc)
{
    IOD_XSKIP(2);
    if (ta && !tb && sgemm_tn_mfma_ok(M, N, K)) return launch_sgemm_tn_mfma(st, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, 0, 0);
    // (the long-K form only where the grid leaves the chip mostly empty: with >= 1024 blocks its 34 KB of LDS costs occupancy -
    // 99 -> 111 us for the 1024 x 512 x 1120 weight gradient)
    if (K >= 512 && ((N + 15) / 16) * ((M + 15) / 16) <= 512)
        hipLaunchKernelGGL(sgemm_kernel<256>, dim3((N + 15) / 16, (M + 15) / 16), dim3(256), 0, st, ta, tb, M, N, K, alpha, A, lda,
                           B, ldb, beta, C, ldc);
    else
        hipLaunchKernelGGL(sgemm_kernel<64>, dim3((N + 15) / 16, (M + 15) / 16), dim3(256), 0, st, ta, tb, M, N, K, alpha, A, lda,
                           B, ldb, beta, C, ldc);
    return hipGetLastError();
}
