// Training-only kernels: weight gradients of the 3x3 conv stacks on fp32 MFMA (reduction over pixels) - the LDS-tiled
// stride-1 kernel, the gathering stride-2 kernel - and the fixed-order reductions of their partial tiles.
//
// They replace what autograd does for the outer ``loss.backward()`` (lib/engine/train.py:63) on the
// graph built by IODINE.forward (lib/modeling/iodine.py:115-158).  Because every ELBO_i reaches the
// decoder parameters only through decoder pass i, and the inner backward of iteration i already
// produced d(B*ELBO_i)/d(pre-activations) for every decoder layer, the decoder weight gradients are
// accumulated during the forward loop with the factor -w_i/B (w_i = (i+1)/(T+1), iodine.py:151-153).
#include "common.h"

// =========================================================================================
// stride-1 3x3 weight gradient, LDS-tiled:  dW[tap][ci][co] = sum_{n,p} a[n, p+tap, ci] * d[n, p, co]
//   GEMM view per tap: M = ci, N = co, K = pixels.  Block = 4 waves, persistent over 8x16-pixel tiles;
//   wave -> (ci half, co half, pixel split); each wave keeps the 9 taps' 32x32 accumulators (144 regs).
//   Partial sums go to part[(block*KS + ks)][tap][ci][co_pad]; a second kernel reduces them in fixed order.
// =========================================================================================
template <int CI, int NCO>
__global__ __launch_bounds__(256, 2)
void conv3x3_wgrad_tile_kernel(const float* __restrict__ a, const float* __restrict__ d, float* __restrict__ part,
                               float* __restrict__ part_b, int S, int ntiles, int tiles_x, int tiles_y)
{
    constexpr int MT = CI / 32;
    constexpr int NTT = (NCO + 31) / 32;
    constexpr int KS = 4 / (MT * NTT);
    constexpr int NCOP = NTT * 32;
    constexpr int TH = 8, TW = 16, HH = TH + 2, HW = TW + 2;
    constexpr int A4 = CI / 4, D4 = NCO / 4;
    constexpr int PXW = (TH * TW) / KS;                 // pixels per wave per tile

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_a = smem;                                   // HH*HW*CI
    float* s_d = smem + HH * HW * CI;                    // TH*TW*NCO

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, half = lane >> 5, li = lane & 31;
    const int mi = wv % MT, ni = (wv / MT) % NTT, ks = wv / (MT * NTT);

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int t = tile;
        const int tx = t % tiles_x; t /= tiles_x;
        const int ty = t % tiles_y;
        const int n = t / tiles_y;
        const int y0 = ty * TH - 1, x0 = tx * TW - 1;
        const float* a_n = a + (size_t)n * S * S * CI;
        const float* d_n = d + (size_t)n * S * S * NCO;
        __syncthreads();
        for (int idx = tid; idx < HH * HW * A4; idx += 256) {
            const int px = idx / A4, c4 = idx % A4;
            const int gy = y0 + px / HW, gx = x0 + px % HW;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < S && gx >= 0 && gx < S)
                v = *reinterpret_cast<const float4*>(a_n + ((size_t)gy * S + gx) * CI + c4 * 4);
            *reinterpret_cast<float4*>(s_a + px * CI + c4 * 4) = v;
        }
        for (int idx = tid; idx < TH * TW * D4; idx += 256) {
            const int px = idx / D4, c4 = idx % D4;
            const int gy = ty * TH + px / TW, gx = tx * TW + px % TW;
            const float4 v = *reinterpret_cast<const float4*>(d_n + ((size_t)gy * S + gx) * NCO + c4 * 4);
            *reinterpret_cast<float4*>(s_d + px * NCO + c4 * 4) = v;
            bsum.x += v.x; bsum.y += v.y; bsum.z += v.z; bsum.w += v.w;
        }
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < PXW / 2; ++s) {
            const int px = ks * PXW + 2 * s + half;
            const int r = px / TW, c = px % TW;
            float bval = 0.f;
            if (NCO >= 32 || li < NCO) bval = s_d[px * NCO + ni * 32 + li];
            const float* ap = s_a + (r * HW + c) * CI + mi * 32 + li;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float aval = ap[((tap / 3) * HW + (tap % 3)) * CI];
                acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(aval, bval, acc[tap], 0, 0, 0);
            }
        }
    }

    // partial dW: rows = ci (accumulator rows), cols = co (lane & 31)
    float* pw = part + ((size_t)(blockIdx.x * KS + ks) * 9) * CI * NCOP;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            pw[((size_t)tap * CI + ci) * NCOP + ni * 32 + li] = acc[tap][r];
        }
    // partial bias gradient: thread's channel group is fixed (256 % D4 == 0)
    __syncthreads();
    float4* s_red = reinterpret_cast<float4*>(smem);
    s_red[tid] = bsum;
    __syncthreads();
    if (tid < D4) {
        float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = tid; j < 256; j += D4) { const float4 v = s_red[j]; t4.x += v.x; t4.y += v.y; t4.z += v.z; t4.w += v.w; }
        *reinterpret_cast<float4*>(part_b + (size_t)blockIdx.x * NCO + tid * 4) = t4;
    }
}

int wgrad_tile_blocks(int N, int S) { const int nt = N * (S / 8) * (S / 16); return nt < 512 ? nt : 512; }

template <int CI, int NCO>
static hipError_t launch_wgrad_tile_inst(hipStream_t st, const float* a, const float* d, float* part, float* part_b,
                                         int N, int S, int* nparts, int* ncop)
{
    constexpr int MT = CI / 32, NTT = (NCO + 31) / 32, KS = 4 / (MT * NTT);
    constexpr size_t lds = (size_t)(10 * 18 * CI + 8 * 16 * NCO) * 4;
    const int tiles_x = S / 16, tiles_y = S / 8, ntiles = N * tiles_x * tiles_y;
    const int blocks = wgrad_tile_blocks(N, S);
    *nparts = blocks * KS;
    *ncop = NTT * 32;
    return iod_launch<conv3x3_wgrad_tile_kernel<CI, NCO>>(st, dim3(blocks), dim3(256), lds, (int)lds, a, d, part, part_b, S, ntiles, tiles_x, tiles_y);
}

hipError_t launch_conv3x3_wgrad_tile(hipStream_t st, const float* a, const float* d, float* part, float* part_b, int N,
                                     int S, int ci, int nco, int* nparts, int* ncop, int* nbias_parts)
{
    if (S % 16 != 0) return hipErrorInvalidValue;
    *nbias_parts = wgrad_tile_blocks(N, S);
    if (ci == 64 && nco == 64) return launch_wgrad_tile_inst<64, 64>(st, a, d, part, part_b, N, S, nparts, ncop);
    if (ci == 32 && nco == 32) return launch_wgrad_tile_inst<32, 32>(st, a, d, part, part_b, N, S, nparts, ncop);
    if (ci == 64 && nco == 4) return launch_wgrad_tile_inst<64, 4>(st, a, d, part, part_b, N, S, nparts, ncop);
    if (ci == 32 && nco == 4) return launch_wgrad_tile_inst<32, 4>(st, a, d, part, part_b, N, S, nparts, ncop);
    return hipErrorInvalidValue;
}

// =========================================================================================
// strided 3x3 weight gradient, operands gathered from global memory (refinement stack):
//   dW[tap][ci][co] = sum_m in[n(m), STRIDE*o(m) + tap - 1, ci] * d[m, co],  m over all output pixels.
// =========================================================================================
template <int CIP, int CO, int STRIDE>
__global__ __launch_bounds__(256, 2)
void conv3x3_wgrad_gather_kernel(const float* __restrict__ in, const float* __restrict__ d, float* __restrict__ part,
                                 int M, int IH, int IW, int OH, int OW, int nchunks)
{
    constexpr int MT = (CIP + 31) / 32;
    constexpr int NTT = CO / 32;
    constexpr int KS = 4 / (MT * NTT);
    constexpr int PXW = 128 / KS;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, half = lane >> 5, li = lane & 31;
    const int mi = wv % MT, ni = (wv / MT) % NTT, ks = wv / (MT * NTT);
    const int ci = mi * 32 + li;
    const bool ci_ok = ci < CIP;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    constexpr int UNR = 4;                                   // k-steps whose 10 gathers each are issued before any MFMA
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        for (int s0 = 0; s0 < PXW / 2; s0 += UNR) {
            float bval[UNR], aval[UNR][9];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int m = chunk * 128 + ks * PXW + 2 * (s0 + u) + half;
                const bool valid = m < M;
                int t = valid ? m : 0;
                const int ox = t % OW; t /= OW;
                const int oy = t % OH;
                const int n = t / OH;
                bval[u] = valid ? d[(size_t)m * CO + ni * 32 + li] : 0.f;
                const float* in_n = in + (size_t)n * IH * IW * CIP + ci;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int iy = oy * STRIDE + tap / 3 - 1, ix = ox * STRIDE + tap % 3 - 1;
                    float v = 0.f;
                    if (valid && ci_ok && iy >= 0 && iy < IH && ix >= 0 && ix < IW) v = in_n[((size_t)iy * IW + ix) * CIP];
                    aval[u][tap] = v;
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(aval[u][tap], bval[u], acc[tap], 0, 0, 0);
        }
    }
    constexpr int CIPAD = MT * 32;
    float* pw = part + ((size_t)(blockIdx.x * KS + ks) * 9) * CIPAD * CO;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cr = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            pw[((size_t)tap * CIPAD + cr) * CO + ni * 32 + li] = acc[tap][r];
        }
}

template <int CIP, int CO, int STRIDE>
static hipError_t launch_wgrad_gather_inst(hipStream_t st, const float* in, const float* d, float* part, int N, int IH,
                                           int IW, int* nparts, int* cipad)
{
    constexpr int MT = (CIP + 31) / 32, NTT = CO / 32, KS = 4 / (MT * NTT);
    const int OH = (IH - 1) / STRIDE + 1, OW = (IW - 1) / STRIDE + 1;
    const int M = N * OH * OW, nchunks = (M + 127) / 128;
    const int blocks = nchunks < 512 ? nchunks : 512;
    hipLaunchKernelGGL((conv3x3_wgrad_gather_kernel<CIP, CO, STRIDE>), dim3(blocks), dim3(256), 0, st, in, d, part, M, IH,
                       IW, OH, OW, nchunks);
    *nparts = blocks * KS;
    *cipad = MT * 32;
    return hipGetLastError();
}

hipError_t launch_conv3x3_wgrad_gather(hipStream_t st, const float* in, const float* d, float* part, int N, int IH,
                                       int IW, int cip, int co, int stride, int* nparts, int* cipad)
{
    if (stride != 2) return hipErrorInvalidValue;
    if (cip == 20 && co == 64) return launch_wgrad_gather_inst<20, 64, 2>(st, in, d, part, N, IH, IW, nparts, cipad);
    if (cip == 64 && co == 64) return launch_wgrad_gather_inst<64, 64, 2>(st, in, d, part, N, IH, IW, nparts, cipad);
    if (cip == 20 && co == 32) return launch_wgrad_gather_inst<20, 32, 2>(st, in, d, part, N, IH, IW, nparts, cipad);
    if (cip == 32 && co == 32) return launch_wgrad_gather_inst<32, 32, 2>(st, in, d, part, N, IH, IW, nparts, cipad);
    return hipErrorInvalidValue;
}

// fixed-order reduction of the partial tiles into an OIHW gradient:
//   dst[co][ci_off + ci][tap] += alpha * sum_b part[b][tap][ci][co]      (ci < I_real, co < O_real)
__global__ __launch_bounds__(256)
void wgrad_reduce_kernel(const float* __restrict__ part, int nparts, int ci_pad, int co_pad, int O_real,
                         int I_real, int I_dst, float alpha, float* __restrict__ dst,
                         const float* __restrict__ part_b, int nb, float* __restrict__ dst_b)
{
    const int total = 9 * ci_pad * co_pad, nblk_w = (total + 255) / 256;
    if ((int)blockIdx.x >= nblk_w) {
        // the blocks behind the weight elements sum the bias partial rows of the same launch (one column each): saves the
        // separate column-sum launch per weight-gradient launch
        __shared__ float s_red[256];
        const int c = blockIdx.x - nblk_w, tid = threadIdx.x;
        float s = 0.f;
        for (int r = tid; r < nb; r += 256) s += part_b[(size_t)r * O_real + c];
        s_red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        if (tid == 0) dst_b[c] += alpha * s_red[0];
        return;
    }
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int co = e % co_pad, ci = (e / co_pad) % ci_pad, tap = e / (co_pad * ci_pad);
    if (co >= O_real || ci >= I_real) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = 0;
    for (; b + 3 < nparts; b += 4) {
        s0 += part[(size_t)b * total + e];
        s1 += part[(size_t)(b + 1) * total + e];
        s2 += part[(size_t)(b + 2) * total + e];
        s3 += part[(size_t)(b + 3) * total + e];
    }
    for (; b < nparts; ++b) s0 += part[(size_t)b * total + e];
    float* o = dst + ((size_t)co * I_dst + ci) * 9 + tap;
    *o += alpha * ((s0 + s1) + (s2 + s3));
}

// first stage for many partial tiles: fold[f][e] = sum of the parts f*per .. f*per+per-1 (float4 columns, all of a
// thread's loads independent), so that the layout-changing second stage reads WGRAD_FOLD tiles instead of hundreds
__global__ __launch_bounds__(256)
void wgrad_fold_kernel(const float4* __restrict__ part, int nparts, int per, int total4, float4* __restrict__ fold)
{
    const int e = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (e >= total4) return;
    const int b0 = f * per, b1 = min(nparts, b0 + per);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    int b = b0;
    for (; b + 7 < b1; b += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(b + j) * total4 + e];
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            s0.x += v[j].x; s0.y += v[j].y; s0.z += v[j].z; s0.w += v[j].w;
            s1.x += v[j + 1].x; s1.y += v[j + 1].y; s1.z += v[j + 1].z; s1.w += v[j + 1].w;
        }
    }
    for (; b < b1; ++b) { const float4 v = part[(size_t)b * total4 + e]; s0.x += v.x; s0.y += v.y; s0.z += v.z; s0.w += v.w; }
    fold[(size_t)f * total4 + e] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
}

// Round 4: both stages in ONE launch (the two-launch form cost 28 x (7.7 + 5.4 us + a kernel boundary) per cfg3 training step).
// A block owns 64 consecutive elements of the [tap][ci][co] tile: thread (g = tid / 16, q = tid % 16) sums float4 column q of the
// parts g, g + 16, g + 32, ... (eight independent 16-byte loads in flight), the 16 group sums meet in LDS and are added in fixed order
// by the first 64 threads, which also do the layout change into OIHW.  Blocks behind the weight blocks sum the bias partial rows.
__global__ __launch_bounds__(256)
void wgrad_reduce_fused_kernel(const float4* __restrict__ part, int nparts, int ci_pad, int co_pad, int O_real, int I_real, int I_dst,
                               float alpha, float* __restrict__ dst, const float* __restrict__ part_b, int nb, float* __restrict__ dst_b)
{
    const int total = 9 * ci_pad * co_pad, total4 = total / 4, nblk_w = total / 64;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nblk_w) {
        __shared__ float s_red[256];
        const int c = blockIdx.x - nblk_w;
        float s = 0.f;
        for (int r = tid; r < nb; r += 256) s += part_b[(size_t)r * O_real + c];
        s_red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        if (tid == 0) dst_b[c] += alpha * s_red[0];
        return;
    }
    __shared__ float4 s_g[16][16];
    const int g = tid >> 4, q = tid & 15;
    const float4* col = part + (size_t)blockIdx.x * 16 + q;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    int b = g;
    for (; b + 7 * 16 < nparts; b += 8 * 16) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = col[(size_t)(b + 16 * j) * total4];
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            s0.x += v[j].x; s0.y += v[j].y; s0.z += v[j].z; s0.w += v[j].w;
            s1.x += v[j + 1].x; s1.y += v[j + 1].y; s1.z += v[j + 1].z; s1.w += v[j + 1].w;
        }
    }
    for (; b < nparts; b += 16) { const float4 v = col[(size_t)b * total4]; s0.x += v.x; s0.y += v.y; s0.z += v.z; s0.w += v.w; }
    s_g[g][q] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
    __syncthreads();
    if (tid < 64) {
        const float* sf = reinterpret_cast<const float*>(&s_g[0][0]);
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int j = 0; j < 16; j += 2) { t0 += sf[j * 64 + tid]; t1 += sf[(j + 1) * 64 + tid]; }
        const int e = blockIdx.x * 64 + tid;
        const int co = e % co_pad, ci = (e / co_pad) % ci_pad, tap = e / (co_pad * ci_pad);
        if (co < O_real && ci < I_real) {
            float* o = dst + ((size_t)co * I_dst + ci) * 9 + tap;
            *o += alpha * (t0 + t1);
        }
    }
}

// part_b / dst_b (optional): nb bias partial rows [nb][O_real] of the same launch, summed into dst_b with the same alpha
hipError_t launch_wgrad_reduce(hipStream_t st, const float* part, int nparts, int ci_pad, int co_pad, int O_real,
                               int I_real, int I_dst, float alpha, float* dst, float* fold, const float* part_b, int nb,
                               float* dst_b)
{
    IOD_XSKIP(1);
    if (nparts <= 0) return hipSuccess;
    const int total = 9 * ci_pad * co_pad;
    const bool with_b = part_b && dst_b && nb > 0;
    if (nparts >= 16 && total % 64 == 0) {
        hipLaunchKernelGGL(wgrad_reduce_fused_kernel, dim3(total / 64 + (with_b ? O_real : 0)), dim3(256), 0, st, (const float4*)part, nparts,
                           ci_pad, co_pad, O_real, I_real, I_dst, alpha, dst, part_b, nb, dst_b);
        return hipGetLastError();
    }
    if (fold && nparts >= 4 * WGRAD_FOLD && total % 4 == 0) {
        const int per = (nparts + WGRAD_FOLD - 1) / WGRAD_FOLD, nf = (nparts + per - 1) / per;
        hipLaunchKernelGGL(wgrad_fold_kernel, dim3((total / 4 + 255) / 256, nf), dim3(256), 0, st, (const float4*)part,
                           nparts, per, total / 4, (float4*)fold);
        part = fold;
        nparts = nf;
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((total + 255) / 256 + (with_b ? O_real : 0)), dim3(256), 0, st, part, nparts,
                       ci_pad, co_pad, O_real, I_real, I_dst, alpha, dst, part_b, nb, dst_b);
    return hipGetLastError();
}
