// Training-only kernels: parameter gradients of the spatial-broadcast layer, and the scalar helpers of the
// training step (loss, zero-fill, scale, axpy, the two logger means).
//
// They replace what autograd does for the outer ``loss.backward()`` (lib/engine/train.py:63) on the
// graph built by IODINE.forward (lib/modeling/iodine.py:115-158).  Because every ELBO_i reaches the
// decoder parameters only through decoder pass i, and the inner backward of iteration i already
// produced d(B*ELBO_i)/d(pre-activations) for every decoder layer, the decoder weight gradients are
// accumulated during the forward loop with the factor -w_i/B (w_i = (i+1)/(T+1), iodine.py:151-153).
#include "common.h"

// =========================================================================================
// spatial-broadcast layer parameter gradients
// =========================================================================================
// RT[n][tap][c] = sum over the border classes in which `tap` stays inside the image of Rc[n][cls][c]
__global__ void l0_tap_sums_kernel(const float* __restrict__ Rc, float* __restrict__ RT, int N, int C)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * 9 * C) return;
    const int c = i % C, tap = (i / C) % 9, n = i / (9 * C);
    const int dy = tap / 3, dx = tap % 3;
    float s = 0.f;
    for (int rc = 0; rc < 3; ++rc) {
        if ((rc == 0 && dy == 0) || (rc == 2 && dy == 2)) continue;
        for (int cc = 0; cc < 3; ++cc) {
            if ((cc == 0 && dx == 0) || (cc == 2 && dx == 2)) continue;
            s += Rc[((size_t)n * 9 + rc * 3 + cc) * C + c];
        }
    }
    RT[i] = s;
}

hipError_t launch_l0_tap_sums(hipStream_t st, const float* Rc, float* RT, int N, int C)
{
    hipLaunchKernelGGL(l0_tap_sums_kernel, dim3((N * 9 * C + 255) / 256), dim3(256), 0, st, Rc, RT, N, C);
    return hipGetLastError();
}

// Round 6: the latent-channel weight gradient of the broadcast layer in ONE launch where the fp32-MFMA GEMM does not apply (DIM_LATENT not a
// multiple of 32: the dSprites architectures) - tap sums, z^T . RT and the scatter into gw[co][ci][tap] were three launches of 5 - 7 us each,
// six times per training step.  One thread per (ci, tap, co); the sum over the slot-images runs in four interleaved partial sums (fixed order).
__global__ __launch_bounds__(256)
void l0_latent_wgrad_kernel(const float* __restrict__ Rc, const float* __restrict__ z, int N, int L, int C, float alpha,
                            float* __restrict__ gw)
{
    // block = 32 outputs (consecutive co of one (ci, tap) when C >= 32) x 8 slices of the slot-images; slice s takes n = s, s + 8, ...
    __shared__ float s_part[8][32];
    const int o = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    const bool live = i < L * 9 * C;
    const int ii = live ? i : 0;
    const int co = ii % C, tap = (ii / C) % 9, ci = ii / (9 * C);
    const int dy = tap / 3, dx = tap % 3;
    // border classes (row class rc, column class cc) in which the tap stays inside the image: rc in [r0, r1], cc in [c0, c1]
    const int r0 = dy == 0 ? 1 : 0, r1 = dy == 2 ? 1 : 2, c0 = dx == 0 ? 1 : 0, c1 = dx == 2 ? 1 : 2;
    float acc = 0.f;
#pragma unroll 4
    for (int n = sl; n < N; n += 8) {                                   // (unrolled: 36 independent loads in flight instead of 9)
        const float* r = Rc + (size_t)n * 9 * C + co;
        float t = 0.f;
#pragma unroll
        for (int rc = 0; rc < 3; ++rc)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const float v = r[(rc * 3 + cc) * C];                   // (all nine classes are loaded: no divergent addressing, 36 bytes per (n, co))
                t += (rc >= r0 && rc <= r1 && cc >= c0 && cc <= c1) ? v : 0.f;
            }
        acc = fmaf(z[(size_t)n * L + ci], t, acc);
    }
    s_part[sl][o] = acc;
    __syncthreads();
    if (sl == 0 && live) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += s_part[q][o];
        gw[((size_t)co * (L + 2) + ci) * 9 + tap] += alpha * t;
    }
}

hipError_t launch_l0_latent_wgrad(hipStream_t st, const float* Rc, const float* z, int N, int L, int C, float alpha, float* gw)
{
    hipLaunchKernelGGL(l0_latent_wgrad_kernel, dim3((L * 9 * C + 31) / 32), dim3(256), 0, st, Rc, z, N, L, C, alpha, gw);
    return hipGetLastError();
}

// coordinate-channel weights and the bias of layer 0 from D[p][c].  Stage 1: block b walks the pixels p = b, b + NB, ...
// with thread = (channel, pixel lane) so that D is read in full rows (the one-block-per-channel form read one float per
// 256-byte row: 151 us for a 4 MB map); 19 sums per channel (9 taps x {x, y} + bias) -> partial[b][19][C].
// Stage 2: fixed-order sum over the NB partials into the gradient accumulators.
constexpr int L0CG_BLOCKS = 512;
__global__ __launch_bounds__(256)
void l0_coord_partial_kernel(const float* __restrict__ D, const float* __restrict__ lin, int S, int C,
                             float* __restrict__ partial)
{
    extern __shared__ float s_cg[];                       // [pixel lanes][19][C]
    const int tid = threadIdx.x, c = tid % C, pl = tid / C, PL = 256 / C;
    float acc[19];
#pragma unroll
    for (int j = 0; j < 19; ++j) acc[j] = 0.f;
    for (int p = blockIdx.x * PL + pl; p < S * S; p += L0CG_BLOCKS * PL) {
        const float v = D[(size_t)p * C + c];
        const int y = p / S, x = p % S;
        acc[18] += v;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy < 0 || yy >= S || xx < 0 || xx >= S) continue;
            acc[tap] += lin[xx] * v;
            acc[9 + tap] += lin[yy] * v;
        }
    }
#pragma unroll
    for (int j = 0; j < 19; ++j) s_cg[(pl * 19 + j) * C + c] = acc[j];
    __syncthreads();
    for (int e = tid; e < 19 * C; e += 256) {
        float t = 0.f;
        for (int q = 0; q < PL; ++q) t += s_cg[q * 19 * C + e];
        partial[(size_t)blockIdx.x * 19 * C + e] = t;
    }
}

__global__ void l0_coord_final_kernel(const float* __restrict__ partial, int C, int L, float alpha, float* __restrict__ gw,
                                      float* __restrict__ gb)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 19 * C) return;
    const int j = e / C, co = e % C;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int b = 0; b < L0CG_BLOCKS; b += 4) {
        s0 += partial[(size_t)b * 19 * C + e]; s1 += partial[(size_t)(b + 1) * 19 * C + e];
        s2 += partial[(size_t)(b + 2) * 19 * C + e]; s3 += partial[(size_t)(b + 3) * 19 * C + e];
    }
    const float t = alpha * ((s0 + s1) + (s2 + s3));
    if (j < 9) gw[((size_t)co * (L + 2) + L) * 9 + j] += t;
    else if (j < 18) gw[((size_t)co * (L + 2) + L + 1) * 9 + (j - 9)] += t;
    else gb[co] += t;
}

// scratch: at least L0CG_BLOCKS * 19 * C floats
hipError_t launch_l0_coord_grads(hipStream_t st, const float* D, const float* lin, int S, int C, int L, float alpha,
                                 float* gw, float* gb, float* scratch)
{
    if (C > 256 || 256 % C != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(l0_coord_partial_kernel, dim3(L0CG_BLOCKS), dim3(256), (size_t)(256 / C) * 19 * C * sizeof(float), st, D,
                       lin, S, C, scratch);
    hipLaunchKernelGGL(l0_coord_final_kernel, dim3((19 * C + 255) / 256), dim3(256), 0, st, scratch, C, L, alpha, gw, gb);
    return hipGetLastError();
}

// The same gradients from Rsum[y][4][C] = sum over passes and slot-images of the per-row sums {left column, interior columns,
// right column, sum_x lin[x] * d} of d = d(pre-activation 0) (EPI_L0ROWSX epilogue -> l0_reduce_cls_tiles_x -> l0_rowsum_acc):
// no [pixels x C] gradient map is needed.  Per row y with L, M, R, X:
//   bias                          += L + M + R
//   y-channel, tap (ky, kx)       += lin[y + ky - 1] * {M + R, L + M + R, L + M}[kx]             (rows with y + ky - 1 inside)
//   x-channel, tap (ky, kx)       += {(X - lin[0] L) - step (M + R),  X,  (X - lin[S-1] R) + step (L + M)}[kx]
// where lin[x -+ 1] = lin[x] -+ step is used for the shifted weights (step = 2 / (S - 1); the table's own differences deviate
// from it by rounding only, <= 1.2e-7 absolute on weights in [-1, 1]).  One block: thread = (channel, row slice).
__global__ __launch_bounds__(256)
void l0_coord_rows_kernel(const float* __restrict__ Rsum, const float* __restrict__ lin, int S, int C, int L, float alpha,
                          float* __restrict__ gw, float* __restrict__ gb)
{
    __shared__ float s_cg[4 * 19 * 64];
    const int tid = threadIdx.x, c = tid % C, sl = tid / C, NSL = 256 / C;
    const float step = __fdiv_rn(2.f, (float)(S - 1)), lin0 = lin[0], linS = lin[S - 1];
    float acc[19];
#pragma unroll
    for (int j = 0; j < 19; ++j) acc[j] = 0.f;
    for (int y = sl; y < S; y += NSL) {
        const float* r = Rsum + (size_t)y * 4 * C + c;
        const float Lv = r[0], Mv = r[C], Rv = r[2 * C], Xv = r[3 * C];
        const float rs[3] = {Mv + Rv, (Lv + Mv) + Rv, Lv + Mv};
        const float ax[3] = {(Xv - lin0 * Lv) - step * (Mv + Rv), Xv, (Xv - linS * Rv) + step * (Lv + Mv)};
        acc[18] += rs[1];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            if (yy < 0 || yy >= S) continue;
            const float ly = lin[yy];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                acc[ky * 3 + kx] += ax[kx];
                acc[9 + ky * 3 + kx] += ly * rs[kx];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 19; ++j) s_cg[(sl * 19 + j) * C + c] = acc[j];
    __syncthreads();
    for (int e = tid; e < 19 * C; e += 256) {
        float t = 0.f;
        for (int q = 0; q < NSL; ++q) t += s_cg[q * 19 * C + e];
        t *= alpha;
        const int j = e / C, co = e % C;
        if (j < 9) gw[((size_t)co * (L + 2) + L) * 9 + j] += t;
        else if (j < 18) gw[((size_t)co * (L + 2) + L + 1) * 9 + (j - 9)] += t;
        else gb[co] += t;
    }
}

hipError_t launch_l0_coord_grads_rows(hipStream_t st, const float* Rsum, const float* lin, int S, int C, int L, float alpha,
                                      float* gw, float* gb)
{
    if (C > 64 || 256 % C != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(l0_coord_rows_kernel, dim3(1), dim3(256), 0, st, Rsum, lin, S, C, L, alpha, gw, gb);
    return hipGetLastError();
}

// =========================================================================================
// loss and the scalar helpers of the training step
// =========================================================================================
// loss = -sum_i w_i * ELBO_i, w_i = (i+1)/(T+1) (iodine.py:151-158) or - wtab != NULL - the objective's table of n weights
__global__ void loss_kernel(const float* __restrict__ scal, int n, float* __restrict__ loss, const float* __restrict__ wtab)
{
    if (threadIdx.x == 0) {
        double s = 0.0;
        if (wtab) {
            for (int i = 0; i < n; ++i) s += (double)wtab[i] * scal[3 * i];
        } else {
            for (int i = 0; i < n; ++i) s += (double)(i + 1) / n * scal[3 * i];
        }
        *loss = (float)(-s);
    }
}

hipError_t launch_loss(hipStream_t st, const float* scal, int n, float* loss, const float* wtab)
{
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(64), 0, st, scal, n, loss, wtab);
    return hipGetLastError();
}

// p[0 .. n) = 0.  Stands where hipMemsetAsync stood in the launch sequences that option "graph" captures: a memset NODE of a replayed
// hipGraph was seen to fill the gradient accumulators with a stale 16-byte pattern instead of zeros (every parameter gradient of the
// replayed step off by the same four values, period 4 floats) - a kernel node carries its arguments by value.
__global__ void zero_fill_kernel(float* __restrict__ p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}

hipError_t launch_zero_fill(hipStream_t st, float* p, size_t n)
{
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, p, n);
    return hipGetLastError();
}

__global__ void scale_kernel(const float* __restrict__ a, float alpha, float* __restrict__ o, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = alpha * a[i];
}

hipError_t launch_scale(hipStream_t st, const float* a, float alpha, float* o, int n)
{
    IOD_XSKIP(64);
    hipLaunchKernelGGL(scale_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a, alpha, o, n);
    return hipGetLastError();
}

// y = (accumulate ? y : 0) + alpha * (*alpha_dev) * x : the hand-over of the accumulated gradients to the caller's flat
// buffer with autograd's incoming grad_output read from device memory (no host round trip, no separate zero-fill)
__global__ void axpy_dev_kernel(const float* __restrict__ x, float alpha, const float* __restrict__ alpha_dev,
                                float* __restrict__ y, int n, int accumulate)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = alpha_dev ? alpha * alpha_dev[0] : alpha;
    y[i] = accumulate ? y[i] + a * x[i] : a * x[i];
}

hipError_t launch_axpy_dev(hipStream_t st, const float* x, float alpha, const float* alpha_dev, float* y, int n, int accumulate)
{
    hipLaunchKernelGGL(axpy_dev_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, alpha, alpha_dev, y, n, accumulate);
    return hipGetLastError();
}

// y = (*s_dev) * y + add in place (s_dev == NULL: the factor is 0 and y is not read; add == NULL: nothing added) - the backward with
// auxiliary cotangents (iodine_train_backward_aux) multiplies what carries the ELBO weights by autograd's d(out) / d(loss) BEFORE the
// auxiliary terms join, which that factor must not reach
__global__ void scale_dev_add_kernel(float* __restrict__ y, const float* __restrict__ s_dev, const float* __restrict__ add, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = s_dev ? s_dev[0] * y[i] : 0.f;
    y[i] = add ? v + add[i] : v;
}

hipError_t launch_scale_dev_add(hipStream_t st, float* y, const float* s_dev, const float* add, int n)
{
    hipLaunchKernelGGL(scale_dev_add_kernel, dim3((n + 255) / 256), dim3(256), 0, st, y, s_dev, add, n);
    return hipGetLastError();
}

// out[0] = mean(a[0..n)), out[1] = mean(b[0..n)): the two logger scalars of IODINE.forward (iodine.py:156-157)
__global__ void mean2_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, float* __restrict__ out)
{
    const float* src = blockIdx.x == 0 ? a : b;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s += (double)src[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s / n);
}

hipError_t launch_mean2(hipStream_t st, const float* a, const float* b, int n, float* out)
{
    hipLaunchKernelGGL(mean2_kernel, dim3(2), dim3(64), 0, st, a, b, n, out);
    return hipGetLastError();
}
