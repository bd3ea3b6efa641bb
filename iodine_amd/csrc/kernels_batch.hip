// Device-resident datasets (include/iodine_hip.h: iodine_batch_gather, iodine_synth_scenes; iodine_amd/resident.py).  Stateless like
// kernels_match.hip: no handle, no workspace, one launch per call, nothing synchronises.
//
// batch_gather_kernel: a batch assembled from a store that lives in device memory.  Item j of the batch is store entry index[j] (a frame of
// a clip counts as an entry: the caller resolves clip n, frame f to n F + f).  Images are uint8 HWC as decoded (kind 0: x = float(u) / 255.f,
// one IEEE division per element - the bits of ToTensor's .float().div_(255.0)) or float32 CHW (kind 1: copied).  Ground truth is one uint16
// per pixel, bit g = inside mask g, unpacked to `planes` uint8 0/1 planes (pack_gt's layout: a bit at or above `planes` is not written, a
// plane beyond an image's masks reads 0 because no word carries its bit).  HBM-bound: 3 (12) + 2 bytes read, 12 + planes written per pixel.
//   W = 4: P % 4 == 0 and every pointer aligned for it (launch_batch_gather decides) - a thread takes four consecutive pixels, loads their
//          12 image bytes as three dwords (or one float4 per channel) and their words as one 8-byte load, and stores one float4 per channel
//          plane and one dword per mask plane;
//   W = 1: any size, element-wise.
// Every offset is a size_t: N * P * 3 passes 2^31 for real data sets.  The indices are the caller's and are validated on the host before
// the launch (resident.py: ValueError outside [0, N)); the kernel does not look at N.
//
// synth_scenes_kernel: synth.make_images (and engine.SyntheticClips' rolled frames) evaluated on the device with the SAME BITS - splitmix64
// hashing in 64-bit integers, object parameters and the inside test in fp64 with contraction off (a fused multiply-add changes which border
// pixels are inside), painter's order, colours float32(v[3:6]).  One block per (item, frame): the first threads hash the item's uniforms
// into LDS, then all threads stride the pixels.
#include "common.h"

static constexpr int BG_THREADS = 256;
static constexpr int SY_THREADS = 256;
static constexpr int SY_MAX_OBJECTS = 16;                   // one bit of the mask word each

template <int W>
__global__ __launch_bounds__(BG_THREADS)
void batch_gather_kernel(const long long* __restrict__ index, const void* __restrict__ images, int kind,
                         const unsigned short* __restrict__ masks, int P, int planes, float* __restrict__ x, unsigned char* __restrict__ gt)
{
    const size_t j = blockIdx.x;
    const size_t p0 = ((size_t)blockIdx.y * BG_THREADS + threadIdx.x) * W;
    if (p0 >= (size_t)P) return;
    const size_t src = (size_t)index[j];
    float* xo = x + j * 3 * (size_t)P + p0;

    if (kind == 0) {
        const unsigned char* u8 = static_cast<const unsigned char*>(images) + (src * P + p0) * 3;
        if constexpr (W == 4) {
            const uint32_t* u32 = reinterpret_cast<const uint32_t*>(u8);   // (src P + p0) * 3 is a multiple of 4 where P and p0 are
            const uint32_t w0 = u32[0], w1 = u32[1], w2 = u32[2];
            unsigned char b[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) { b[i] = (w0 >> (8 * i)) & 255u; b[4 + i] = (w1 >> (8 * i)) & 255u; b[8 + i] = (w2 >> (8 * i)) & 255u; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4 v;
                v.x = (float)b[c] / 255.f; v.y = (float)b[3 + c] / 255.f; v.z = (float)b[6 + c] / 255.f; v.w = (float)b[9 + c] / 255.f;
                *reinterpret_cast<float4*>(xo + (size_t)c * P) = v;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) xo[(size_t)c * P] = (float)u8[c] / 255.f;
        }
    } else {
        const float* f32 = static_cast<const float*>(images) + src * 3 * (size_t)P + p0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (W == 4) *reinterpret_cast<float4*>(xo + (size_t)c * P) = *reinterpret_cast<const float4*>(f32 + (size_t)c * P);
            else xo[(size_t)c * P] = f32[(size_t)c * P];
        }
    }

    if (masks == nullptr || gt == nullptr) return;
    const unsigned short* mw = masks + src * P + p0;
    unsigned char* go = gt + j * planes * (size_t)P + p0;
    if constexpr (W == 4) {
        const uint2 t = *reinterpret_cast<const uint2*>(mw);
        const uint32_t m0 = t.x & 0xFFFFu, m1 = t.x >> 16, m2 = t.y & 0xFFFFu, m3 = t.y >> 16;
        for (int g = 0; g < planes; ++g) {
            const uint32_t v = ((m0 >> g) & 1u) | (((m1 >> g) & 1u) << 8) | (((m2 >> g) & 1u) << 16) | (((m3 >> g) & 1u) << 24);
            *reinterpret_cast<uint32_t*>(go + (size_t)g * P) = v;
        }
    } else {
        const uint32_t m = mw[0];
        for (int g = 0; g < planes; ++g) go[(size_t)g * P] = (unsigned char)((m >> g) & 1u);
    }
}

hipError_t launch_batch_gather(hipStream_t st, const long long* index, int count, const void* images, int kind, const unsigned short* masks,
                               int S, int planes, float* x, unsigned char* gt)
{
    if (count < 1 || S < 1 || planes < 1 || planes > SY_MAX_OBJECTS || (kind != 0 && kind != 1)) return hipErrorInvalidValue;
    const int P = S * S;
    auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    const bool vec = P % 4 == 0 && al(x, 16) && al(images, kind == 0 ? 4 : 16) && (!masks || !gt || (al(masks, 8) && al(gt, 4)));
    if (vec) {
        const dim3 grid((unsigned)count, (unsigned)((P / 4 + BG_THREADS - 1) / BG_THREADS));
        hipLaunchKernelGGL(batch_gather_kernel<4>, grid, dim3(BG_THREADS), 0, st, index, images, kind, masks, P, planes, x, gt);
    } else {
        const dim3 grid((unsigned)count, (unsigned)((P + BG_THREADS - 1) / BG_THREADS));
        hipLaunchKernelGGL(batch_gather_kernel<1>, grid, dim3(BG_THREADS), 0, st, index, images, kind, masks, P, planes, x, gt);
    }
    return hipGetLastError();
}

// ---- synthetic scenes -------------------------------------------------------------------------------------------------------------
IOD_DEVINL unsigned long long sy_splitmix(unsigned long long v)
{
    v += 0x9E3779B97F4A7C15ull;
    v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
    v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
    return v ^ (v >> 31);
}
// synth.uniform01: element i of the stream under `key`
IOD_DEVINL double sy_uniform(unsigned long long key, unsigned long long i)
{
    return (double)(sy_splitmix(i ^ key) >> 11) * (1.0 / 9007199254740992.0);
}

// kind 0 = 'uniform', 1 = 'blobs'.  Item i draws from (seed + i seed_step [+ 7919 for blobs], stream + i stream_step).  frames = 0: stills
// (one frame, no roll); frames = F: frame f is the scene rolled by (f, 2 f) pixels (rows, columns).
__global__ __launch_bounds__(SY_THREADS)
void synth_scenes_kernel(int S, unsigned long long seed, unsigned long long seed_step, unsigned long long stream, unsigned long long stream_step,
                         int kind, int max_objects, int frames, float* __restrict__ images, unsigned short* __restrict__ masks,
                         unsigned char* __restrict__ n_gt)
{
#pragma clang fp contract(off)
    __shared__ double s_u[8 * (SY_MAX_OBJECTS + 1)];
    const int F = frames > 0 ? frames : 1;
    const size_t item = blockIdx.x / F;
    const int f = (int)(blockIdx.x - item * F);
    const int P = S * S;
    const unsigned long long sd = seed + item * seed_step + (kind == 1 ? 7919ull : 0ull);
    const unsigned long long key = sy_splitmix(sd * 0x2545F4914F6CDD1Dull + (stream + item * stream_step));
    float* img = images + (size_t)blockIdx.x * 3 * P;
    const int dy = f % S, dx = (2 * f) % S;                  // torch.roll: out[y][x] = in[(y - f) mod S][(x - 2 f) mod S]

    if (kind == 0) {
        for (int p = threadIdx.x; p < P; p += SY_THREADS) {
            const int y = p / S, xq = p - y * S;
            const int sy = y - dy < 0 ? y - dy + S : y - dy, sx = xq - dx < 0 ? xq - dx + S : xq - dx;
            const int q = sy * S + sx;
#pragma unroll
            for (int c = 0; c < 3; ++c) img[(size_t)c * P + p] = (float)sy_uniform(key, (unsigned long long)c * P + q);
        }
        return;
    }

    const int nu = 8 * (max_objects + 1);
    for (int i = threadIdx.x; i < nu; i += SY_THREADS) s_u[i] = sy_uniform(key, (unsigned long long)i);
    __syncthreads();
    int n_obj = max_objects > 3 ? 3 + (int)(s_u[0] * (double)(max_objects - 2)) : max_objects;
    n_obj = n_obj < max_objects ? n_obj : max_objects;
    if (threadIdx.x == 0 && f == 0 && n_gt) n_gt[item] = (unsigned char)n_obj;
    const double dS = (double)S;
    const double r0 = dS / 16.0, r1 = dS / 6.0 - dS / 16.0;
    for (int p = threadIdx.x; p < P; p += SY_THREADS) {
        const int y = p / S, xq = p - y * S;
        const double yy = (double)(y - dy < 0 ? y - dy + S : y - dy), xx = (double)(xq - dx < 0 ? xq - dx + S : xq - dx);
        int owner = 0;
        for (int o = 0; o < n_obj; ++o) {
            const double* v = s_u + 8 * (o + 1);
            const double cx = v[0] * dS, cy = v[1] * dS;
            const double rad = r0 + v[2] * r1;
            const double ex = xx - cx, ey = yy - cy;
            bool in;
            if (v[6] < 0.5) {
                const double ex2 = ex * ex, ey2 = ey * ey;
                in = ex2 + ey2 <= rad * rad;
            } else {
                in = fabs(ex) <= rad && fabs(ey) <= rad;
            }
            if (in) owner = o + 1;                           // painter's order: the last object wins the pixel
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) img[(size_t)c * P + p] = owner ? (float)s_u[8 * owner + 3 + c] : 0.25f;
        if (masks) masks[(size_t)blockIdx.x * P + p] = owner ? (unsigned short)(1u << (owner - 1)) : (unsigned short)0;
    }
}

hipError_t launch_synth_scenes(hipStream_t st, int n, int S, unsigned long long seed, unsigned long long seed_step, unsigned long long stream,
                               unsigned long long stream_step, int kind, int max_objects, int frames, float* images, unsigned short* masks,
                               unsigned char* n_gt)
{
    if (n < 1 || S < 1 || S > 1024 || frames < 0 || (kind != 0 && kind != 1) || max_objects < 1 || max_objects > SY_MAX_OBJECTS)
        return hipErrorInvalidValue;
    const long long blocks = (long long)n * (frames > 0 ? frames : 1);
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(synth_scenes_kernel, dim3((unsigned)blocks), dim3(SY_THREADS), 0, st, S, seed, seed_step, stream, stream_step, kind,
                       max_objects, frames, images, masks, n_gt);
    return hipGetLastError();
}
