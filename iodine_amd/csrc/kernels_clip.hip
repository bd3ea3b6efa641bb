// Global-norm gradient clipping next to the fused Adam step (kernels_misc.hip, adam_multi_kernel).
//
// The paper clips the global gradient norm at 5.0; the reference carries the line commented out,
// `# clip_grad_norm_(model.parameters(), 5.0)` (lib/engine/train.py:64), between loss.backward() and optimizer.step().
// Semantics of torch.nn.utils.clip_grad_norm_ with norm_type = 2:
//     total_norm = || all gradients ||_2,   clip_coef = min(1, max_norm / (total_norm + 1e-6)),   grad *= clip_coef.
//
// The tables are the ones launch_adam_multi takes: ptrs[4*t + 1] = gradient of tensor t, offs[t] = its first flat element.
//
// Determinism: the grid and every block's range are functions of `total` alone (clip_grid), a thread's elements and their
// order are functions of (range, thread id), the wave step is a fixed shuffle tree, the block step and the final sum run
// in index order on one thread, and no floating-point atomic is used - the same gradients give the same bits on every
// run and on every rank.  Everything is accumulated in fp64 (a square of an fp32 value is exact there), so the only
// fp32 rounding of total_norm is the cast of the fp64 square root.
#include "common.h"

static constexpr int CLIP_THREADS = 256;
static constexpr long long CLIP_BLOCK_ELEMS = 4096;          // 256 threads x 4 floats x 4 rounds: ~270 blocks at the CLEVR architecture
static constexpr long long CLIP_MAX_BLOCKS = 1024;           // the finalize kernel keeps the partials in LDS

// blocks / elements per block (a multiple of 4, so 16-byte loads keep their alignment across blocks): pure functions of total
static inline void clip_grid(long long total, int* blocks, long long* chunk)
{
    const long long b = std::min<long long>(std::max<long long>((total + CLIP_BLOCK_ELEMS - 1) / CLIP_BLOCK_ELEMS, 1), CLIP_MAX_BLOCKS);
    long long c = (total + b - 1) / b;
    c = std::max<long long>((c + 3) & ~3LL, 4);
    *chunk = c;
    *blocks = (int)std::max<long long>((total + c - 1) / c, 1);
}

size_t grad_norm_scratch_bytes(long long total)
{
    int blocks; long long chunk;
    clip_grid(total < 1 ? 1 : total, &blocks, &chunk);
    return sizeof(double) * (size_t)blocks;
}

// last tensor whose offset <= i (as in adam_multi_kernel)
IOD_DEVINL int clip_find_tensor(const long long* __restrict__ offs, int n_tensors, long long i)
{
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

IOD_DEVINL double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                                 // lane 0 holds the sum
}

__global__ __launch_bounds__(CLIP_THREADS)
void grad_sumsq_multi_kernel(const long long* __restrict__ ptrs, const long long* __restrict__ offs, int n_tensors,
                             long long total, long long chunk, double* __restrict__ partials)
{
    __shared__ double s_wave[CLIP_THREADS / 64];
    const long long beg = (long long)blockIdx.x * chunk;
    const long long end = beg + chunk < total ? beg + chunk : total;
    double acc = 0.0;
    for (long long i = beg + 4 * (long long)threadIdx.x; i < end; i += 4 * CLIP_THREADS) {
        int t = clip_find_tensor(offs, n_tensors, i);
        const long long t_end = t + 1 < n_tensors ? offs[t + 1] : total;
        const float* g = reinterpret_cast<const float*>(ptrs[4 * t + 1]) + (i - offs[t]);
        if (i + 4 <= end && i + 4 <= t_end && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const float4 q = *reinterpret_cast<const float4*>(g);           // the flat case: four floats of one tensor, aligned
            acc += (double)q.x * (double)q.x;
            acc += (double)q.y * (double)q.y;
            acc += (double)q.z * (double)q.z;
            acc += (double)q.w * (double)q.w;
        } else {                                                            // tensor boundary, unaligned start or tail
            const int rem = (int)(end - i < 4 ? end - i : 4);
            for (int e = 0; e < rem; ++e) {
                const long long k = i + e;
                while (t + 1 < n_tensors && offs[t + 1] <= k) ++t;
                const float x = reinterpret_cast<const float*>(ptrs[4 * t + 1])[k - offs[t]];
                acc += (double)x * (double)x;
            }
        }
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_wave[0];
#pragma unroll
        for (int w = 1; w < CLIP_THREADS / 64; ++w) s += s_wave[w];
        partials[blockIdx.x] = s;
    }
}

// one block: out[0] = total_norm, out[1] = clip_coef, out[2] = 1 when total_norm is not finite, out[3] += out[2]
__global__ __launch_bounds__(CLIP_THREADS)
void grad_clip_finalize_kernel(const double* __restrict__ partials, int n_partials, float max_norm, float* __restrict__ out)
{
    __shared__ double s_part[CLIP_MAX_BLOCKS];
    for (int i = threadIdx.x; i < n_partials; i += CLIP_THREADS) s_part[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n_partials; ++i) s += s_part[i];                     // index order
    const float norm = (float)sqrt(s);
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    const float flag = (norm - norm == 0.f) ? 0.f : 1.f;                     // inf - inf and NaN - NaN are NaN
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;                                              // clamp(max = 1): a NaN stays a NaN, as in torch
    out[2] = flag;
    out[3] = out[3] + flag;
}

// g *= coef in place (the stand-alone clip_grad_norm_, which leaves .grad clipped as torch's does)
__global__ __launch_bounds__(CLIP_THREADS)
void grad_scale_multi_kernel(const long long* __restrict__ ptrs, const long long* __restrict__ offs, int n_tensors,
                             long long total, const float* __restrict__ coef_dev)
{
    const float coef = coef_dev[0];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int t = clip_find_tensor(offs, n_tensors, i);
        float* g = reinterpret_cast<float*>(ptrs[4 * t + 1]);
        const long long j = i - offs[t];
        g[j] = __fmul_rn(g[j], coef);
    }
}

hipError_t launch_grad_norm(hipStream_t st, const long long* ptrs, const long long* offs, int n_tensors, long long total,
                            double max_norm, double* partials, float* out4)
{
    int blocks; long long chunk;
    clip_grid(total, &blocks, &chunk);
    hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3(blocks), dim3(CLIP_THREADS), 0, st, ptrs, offs, n_tensors, total, chunk,
                       partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(CLIP_THREADS), 0, st, partials, blocks, (float)max_norm, out4);
    return hipGetLastError();
}

hipError_t launch_grad_scale(hipStream_t st, const long long* ptrs, const long long* offs, int n_tensors, long long total,
                             const float* coef_dev)
{
    const int blocks = (int)std::min<long long>((total + CLIP_THREADS - 1) / CLIP_THREADS, 2048);
    hipLaunchKernelGGL(grad_scale_multi_kernel, dim3(blocks), dim3(CLIP_THREADS), 0, st, ptrs, offs, n_tensors, total, coef_dev);
    return hipGetLastError();
}
