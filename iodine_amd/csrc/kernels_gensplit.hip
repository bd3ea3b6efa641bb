// Split-fp16 forms of the generic stride-1 conv C -> C (option gen_conv_precision 1): the forward conv and the data gradient (first kernel)
// and the weight + bias gradient (second kernel, further down) of the
// decoder layers that kernels_generic.hip runs on v_mfma_f32_16x16x4_f32 - KERNEL_SIZE 3 / 5 / 7 (the reference's default DEC.KERNEL_SIZE is
// 5, lib/config/defaults.py:100; configs/test.yaml:40,44), channel counts that are multiples of 16, any image size.  Operands stay fp32 in
// memory; in LDS they are fp16 hi + lo with a power-of-two scale (x * scale = hi + lo, 22 significant bits), a product is three
// v_mfma_f32_16x16x32_f16 (hi.hi, hi.lo, lo.hi) accumulated in fp32: 3 MFMAs of 16 cycles for a reduction of 32 where the fp32 kernel
// issues 8 of 32 cycles.
//
// Structure of gen_conv_mfma_kernel kept: a persistent block owns ONE group of 16 output channels, its weight slice is LDS-resident for all
// its tiles (hi + lo fp16 = the bytes of the fp32 slice), tiles of 16 x 16 pixels, the halo staged per chunk of CCH channels, blocks that
// share an input tile grouped on one XCD.  Differences:
//   * the weight slice arrives packed (gsplit_pack_kernel at set_params: one scale per slice = per 16 output channels and direction) in the
//     order the MFMA reads it: blocks of 1 KB [k-group kq][16 output channels][8 halves], lane l reads its 16 bytes at l * 16.
//   * CCH = 32: one tap per MFMA (K = 32 channels).  CCH = 16 (channel counts that are not multiples of 32, and 7 x 7 whose 32-channel
//     halo does not fit beside the slice): TWO taps per MFMA, k-groups 0-1 the 16 channels of tap 2g, k-groups 2-3 of tap 2g + 1 (each
//     lane reads its own halo pixel, so the tap shift costs nothing; an odd tap count pads the last pair with zero weights).
//   * the staged chunk is [k-group of 8 channels][halo pixel][8 halves], planes a multiple of 256 bytes apart: the 16 lanes of a
//     ds_read_b128 group (8 pixels of one k-group, 4 + 4 of the next) then cover all 64 banks once - no bank conflicts by construction;
//     the staging writes (ds_write_b64, 16 lanes = 8 pixels x 16 bytes of one plane) are conflict-free too.
//   * ONE scale per staged halo and chunk, from the values the block has just fetched (register maxima -> wave_max_f32 -> four words of
//     LDS); the chunk's MFMAs accumulate into their own registers, which are folded into the tile's accumulators with the exact inverse
//     scale (a power of two) - so a chunk with large values costs the other chunks nothing.
//   * the halo is single-buffered: the barrier that publishes the maxima also ends the reads of the previous chunk.  The global loads of
//     the next chunk are in flight under the MFMAs; conversion and LDS writes are exposed (profiles/gen_split_kernel_stats.md).
// No atomics; the order of every sum is fixed by (grid, tile sequence) - the same bits on every call.
#include "common.h"

namespace {

template <int KS, int CCH>
struct GSplitGeo {
    static constexpr int KK = KS * KS, PAD = KS / 2, TW = 16 + KS - 1, NPX = TW * TW;
    static constexpr int NPXP = (NPX + 15) / 16 * 16;         // plane = NPXP x 16 bytes: a multiple of 256
    static constexpr int TPM = 32 / CCH;                      // taps per MFMA
    static constexpr int NG = (KK + TPM - 1) / TPM;           // MFMA groups (of TPM taps) per chunk
    static constexpr int KGC = CCH / 8;                       // k-groups (8 channels) per chunk
    static constexpr int PLANE = NPXP * 16;                   // bytes
    static constexpr int HALF = KGC * PLANE;                  // hi image of a staged chunk (lo follows)
    static constexpr int PXW = 32 / KGC;                      // halo pixels one wave stages per load instruction
    static constexpr int NWL = (NPX + PXW - 1) / PXW;
    static constexpr int NLD = (NWL + 3) / 4;                 // 16-byte loads per thread and chunk
};

// bytes of one slice image (hi + lo) and of the kernel's LDS
inline size_t gsplit_slice_bytes(int k, int C, int cch) { return wpk_gen_split_slice_bytes(k, C, cch); }
inline size_t gsplit_lds_bytes(int k, int C, int cch)
{
    const int tw = 16 + k - 1, npxp = (tw * tw + 15) / 16 * 16;
    return gsplit_slice_bytes(k, C, cch) + (size_t)2 * (cch / 8) * npxp * 16 + 32;
}

// slice images of every 16-channel group from the generic pack wt [tap][ci][co] (W(tap, k, n) as in gen_conv_mfma_kernel), one block per group
__global__ __launch_bounds__(256)
void gsplit_pack_kernel(const float* __restrict__ wt, int KK, int C, int cch, int flip, int sT, int sK, int sN, unsigned* __restrict__ dst,
                        float* __restrict__ meta)
{
    __shared__ float red[4];
    const int cg = blockIdx.x, tid = threadIdx.x;
    const int tpm = 32 / cch, ng = (KK + tpm - 1) / tpm, kgc = cch / 8;
    const int nel = (C / cch) * ng * 512;                    // halves per image
    auto W = [&](int e) -> float {
        const int blk = e >> 9, kq = (e >> 7) & 3, n = (e >> 3) & 15, j = e & 7;
        const int c = blk / ng, g = blk % ng, tap = g * tpm + kq / kgc, ch = c * cch + (kq % kgc) * 8 + j;
        if (tap >= KK) return 0.f;
        return wt[(size_t)(flip ? KK - 1 - tap : tap) * sT + (size_t)ch * sK + (size_t)(cg * 16 + n) * sN];
    };
    float mx = 0.f;
    for (int e = tid; e < nel; e += 256) mx = fmaxf(mx, fabsf(W(e)));
    mx = wave_max_f32(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = tile_scale(mx, 1.f);
    unsigned* dh = dst + (size_t)cg * nel;                   // nel / 2 words of hi, then nel / 2 of lo
    unsigned* dl = dh + nel / 2;
    for (int p = tid; p < nel / 2; p += 256) {
        unsigned lo;
        const unsigned hi = pack_hi_lo(W(2 * p) * sc, W(2 * p + 1) * sc, lo);
        dh[p] = hi; dl[p] = lo;
    }
    if (tid == 0) meta[cg] = 1.f / sc;
}

template <int KS, int CCH>
__global__ __launch_bounds__(256)
void gsplit_conv_kernel(const float* __restrict__ in, const uint4* __restrict__ wpk, const float* __restrict__ wmeta,
                        const float* __restrict__ bias, const float* __restrict__ aux, float* __restrict__ out, int S, int C, int elu,
                        int ncg, int tiles, int ntiles)
{
    using G = GSplitGeo<KS, CCH>;
    constexpr int KK = G::KK, PAD = G::PAD, TW = G::TW, NPX = G::NPX, TPM = G::TPM, NG = G::NG, KGC = G::KGC, PLANE = G::PLANE, HALF = G::HALF,
                  PXW = G::PXW, NLD = G::NLD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_gs[];
    const int nchunk = C / CCH;
    const int wimg = nchunk * NG * 1024;                      // bytes of the hi (and of the lo) weight image
    const unsigned char* s_wh = smem_gs;
    const unsigned char* s_wl = smem_gs + wimg;
    unsigned char* s_in = smem_gs + 2 * wimg;                 // [hi, lo][KGC][NPXP][8 halves]
    float* s_red = reinterpret_cast<float*>(s_in + 2 * HALF); // [2][4] wave maxima of the chunk being staged
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int cg, pb;
    const int nb = gridDim.x / ncg;
    if (nb % 8 == 0) { const int x = blockIdx.x & 7, j = blockIdx.x >> 3; cg = j % ncg; pb = (j / ncg) * 8 + x; }
    else { cg = blockIdx.x % ncg; pb = blockIdx.x / ncg; }
    if (pb >= nb) return;
    // ---- weight slice image -> LDS, once ----
    {
        const uint4* src = wpk + (size_t)cg * (2 * wimg / 16);
        uint4* dstw = reinterpret_cast<uint4*>(smem_gs);
        for (int e0 = tid; e0 < 2 * wimg / 16; e0 += 4 * 256) {
            uint4 v[4] = {};
#pragma unroll
            for (int j = 0; j < 4; ++j) if (e0 + 256 * j < 2 * wimg / 16) v[j] = src[e0 + 256 * j];
#pragma unroll
            for (int j = 0; j < 4; ++j) if (e0 + 256 * j < 2 * wimg / 16) dstw[e0 + 256 * j] = v[j];
        }
    }
    const float winv = wmeta[cg];
    const int m = lane & 15, kq = lane >> 4;
    const int co0 = cg * 16 + 4 * kq;                         // D rows 4 kq + v = this lane's four output channels, column = pixel m
    float bv[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) bv[v] = bias ? bias[co0 + v] : 0.f;
    // ---- staging table: load i of wave wv covers halo pixels (wv + 4 i) PXW ..; lane -> (pixel, channel quad q) so that 16 consecutive lanes
    // write 8 pixels x 16 bytes of ONE plane ----
    const int skg = (lane >> 4) % KGC, sq = skg * 2 + (lane & 1);
    const int spx = ((lane >> 4) / KGC) * 8 + ((lane >> 1) & 7);
    int pyx[NLD], lw[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int px = (wv + 4 * i) * PXW + spx;
        pyx[i] = px < NPX ? ((px / TW) | (px % TW) << 8) : (255 | 255 << 8);     // (255: never inside the image)
        lw[i] = px < NPX ? skg * PLANE + px * 16 + (lane & 1) * 8 : -1;
    }
    u32x4 rin[NLD];
    unsigned tvo[NLD];
    __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, 0, 0x00020000);
    const int img_bytes = S * S * C * 4;
    auto setup_fetch = [&](int t) {
        const int tx = t % tiles, ty = (t / tiles) % tiles, n = t / (tiles * tiles);
        const int gy0 = ty * 16 - PAD, gx0 = tx * 16 - PAD;
        const bool live = t < ntiles;
        rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in + (size_t)(live ? n : 0) * S * S * C), 0, live ? img_bytes : 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int gy = gy0 + (pyx[i] & 255), gx = gx0 + (pyx[i] >> 8);
            tvo[i] = ((unsigned)gy < (unsigned)S && (unsigned)gx < (unsigned)S) ? (unsigned)(((gy * S + gx) * C + 4 * sq) * 4) : 0x80000000u;
        }
    };
    auto fetch = [&](int c) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) rin[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (int)tvo[i], c * CCH * 4, 0);
    };
    // the fetched chunk -> scale -> hi / lo planes.  The barrier inside ends every wave's reads of the previous chunk.  Returns 1 / scale.
    auto stage = [&](int par) -> float {
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(__uint_as_float(rin[i].x)), fabsf(__uint_as_float(rin[i].y)))),
                       fmaxf(fabsf(__uint_as_float(rin[i].z)), fabsf(__uint_as_float(rin[i].w))));
        mx = wave_max_f32(mx);
        if (lane == 0) s_red[par * 4 + wv] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(s_red[par * 4], s_red[par * 4 + 1]), fmaxf(s_red[par * 4 + 2], s_red[par * 4 + 3]));
        const float sc = tile_scale(mx, 1.f);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            if (lw[i] < 0) continue;
            uint2 hi, lo;
            hi.x = pack_hi_lo(__uint_as_float(rin[i].x) * sc, __uint_as_float(rin[i].y) * sc, lo.x);
            hi.y = pack_hi_lo(__uint_as_float(rin[i].z) * sc, __uint_as_float(rin[i].w) * sc, lo.y);
            *reinterpret_cast<uint2*>(s_in + lw[i]) = hi;
            *reinterpret_cast<uint2*>(s_in + HALF + lw[i]) = lo;
        }
        return 1.f / sc;
    };
    f32x4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto epilogue = [&](int t) {
        const int tx = t % tiles, ty = (t / tiles) % tiles, n = t / (tiles * tiles);
        const int x = tx * 16 + m;
        if (x >= S) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = ty * 16 + 4 * wv + r;
            if (y >= S) continue;
            const size_t o = (((size_t)n * S + y) * S + x) * C + co0;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = acc[r][j] + bv[j]; if (elu) v[j] = elu1_fast(v[j]); }
            if (aux) {
                const float4 a = *reinterpret_cast<const float4*>(aux + o);
                v[0] *= elu1_grad_from_out(a.x); v[1] *= elu1_grad_from_out(a.y);
                v[2] *= elu1_grad_from_out(a.z); v[3] *= elu1_grad_from_out(a.w);
            }
            *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    // this lane's halo read: plane of its k-group, tile row 4 wv, pixel m; with two taps per MFMA the upper k-groups read the second tap
    const int kgl = kq % KGC, th = kq / KGC;
    const unsigned char* sb = s_in + kgl * PLANE + ((4 * wv) * TW + m) * 16;
    int t = pb, c = 0, par = 0;
    setup_fetch(t);
    fetch(0);
    float inv = stage(par);
    par ^= 1;
    __syncthreads();                                          // weights and the first chunk staged
    while (t < ntiles) {
        const bool last_chunk = c + 1 == nchunk;
        const int tn = last_chunk ? t + nb : t, cn = last_chunk ? 0 : c + 1;
        if (last_chunk) setup_fetch(tn);                      // (past the last tile: an empty buffer, every load returns zeros)
        fetch(cn);                                            // in flight under this chunk's MFMAs
        f32x4 tacc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) tacc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char* wh = s_wh + (size_t)c * NG * 1024 + lane * 16;
        const unsigned char* wl = s_wl + (size_t)c * NG * 1024 + lane * 16;
        if constexpr (TPM == 1) {
            // one tap per MFMA: the (4 + KS - 1) halo rows of a kernel column kx are read once and shared by the taps (ky, kx) of the four tile rows
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                f16x8 bh[4 + KS - 1], bl[4 + KS - 1];
#pragma unroll
                for (int rr = 0; rr < 4 + KS - 1; ++rr) {
                    bh[rr] = *reinterpret_cast<const f16x8*>(sb + (rr * TW + kx) * 16);
                    bl[rr] = *reinterpret_cast<const f16x8*>(sb + HALF + (rr * TW + kx) * 16);
                }
#pragma unroll
                for (int ky = 0; ky < KS; ++ky) {
                    const f16x8 ah = *reinterpret_cast<const f16x8*>(wh + (ky * KS + kx) * 1024);
                    const f16x8 al = *reinterpret_cast<const f16x8*>(wl + (ky * KS + kx) * 1024);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        tacc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[r + ky], tacc[r], 0, 0, 0);
                        tacc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[r + ky], tacc[r], 0, 0, 0);
                        tacc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[r + ky], tacc[r], 0, 0, 0);
                    }
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int tA = g * TPM, tB = g * TPM + 1 < KK ? g * TPM + 1 : tA;      // (a padded second tap: zero weights, any valid address)
                const int offA = ((tA / KS) * TW + tA % KS) * 16, offB = ((tB / KS) * TW + tB % KS) * 16;
                const int off = th ? offB : offA;
                const f16x8 ah = *reinterpret_cast<const f16x8*>(wh + g * 1024);
                const f16x8 al = *reinterpret_cast<const f16x8*>(wl + g * 1024);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f16x8 bh = *reinterpret_cast<const f16x8*>(sb + off + r * TW * 16);
                    const f16x8 bl = *reinterpret_cast<const f16x8*>(sb + HALF + off + r * TW * 16);
                    tacc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, tacc[r], 0, 0, 0);
                    tacc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, tacc[r], 0, 0, 0);
                    tacc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, tacc[r], 0, 0, 0);
                }
            }
        }
        const float f = inv * winv;                           // exact: both powers of two
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[r][j] = fmaf(tacc[r][j], f, acc[r][j]);
        inv = stage(par);                                     // (its barrier: every wave is done with this chunk's planes)
        par ^= 1;
        if (last_chunk) {
            epilogue(t);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();                                      // the next chunk's planes are complete
        t = tn; c = cn;
    }
}

template <int KS, int CCH>
hipError_t gsplit_launch(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias, const float* aux, float* out,
                         int N, int S, int C, int elu)
{
    int n_cu = 0;
    if (hipError_t e = iod_cu_count(&n_cu); e != hipSuccess) return e;
    const size_t lds = gsplit_lds_bytes(KS, C, CCH);
    const int ncg = C / 16, tiles = (S + 15) / 16, ntiles = N * tiles * tiles;
    const int per_cu = lds <= 80 * 1024 ? 2 : 1;
    const int nb = std::max(1, std::min(ntiles, per_cu * n_cu / ncg));
    return iod_launch<gsplit_conv_kernel<KS, CCH>>(st, dim3(ncg * nb), dim3(256), lds, 160 * 1024, in, reinterpret_cast<const uint4*>(wpk), wmeta, bias,
                                                   aux, out, S, C, elu, ncg, tiles, ntiles);
}


// =====================================================================================================================================
// Weight + bias gradient of the same conv in split form: dW[tap][ci][co] = sum_px in[px + tap][ci] * dout[px][co], K = pixels.
// As in gen_wgrad_rows_kernel a block owns ONE kernel row ky and one slice of the work and writes partial tiles part[slice][tap][ci][co]
// (+ the bias partial from the blocks of ky = 0) for gen_conv_wgrad_reduce_kernel, whose fixed summation order is reused unchanged.
// The unit of work is 8 image rows x 16 columns of one slot-image.  The K = 32 of an MFMA is 4 columns (one per k-group) x 8 ROWS (the 8
// halves of a lane), so the staged planes are [channel][column][8 rows] halves: a tap shift kx moves a lane's read by whole 16-byte slots
// (no unaligned fragment, no transposing read), and the row shift ky is applied when the input rows are fetched.  A staging thread loads the
// 8 rows of one (column, channel quad) straight from NHWC and writes one ds_write_b128 per channel and hi / lo.  Channel rows are 34 (input,
// 16 + KS - 1 columns used) and 18 (gradient) slots apart: = 2 (mod 16), which makes the 16 lanes of every ds_read_b128 group (8 channels
// at column x, 8 at x + 1) hit 16 different slots.  One scale per unit for the input and one for the gradient, from the fetched registers;
// a unit's MFMAs accumulate in their own registers and are folded with the exact inverse scales.  The bias sum is an MFMA against a
// fragment of ones.  The next unit's loads are in flight under the MFMAs.  No atomics, fixed order.
// =====================================================================================================================================
constexpr int GSW_SEG = 16, GSW_WA = 34, GSW_WB = 18, GSW_NIT = 3;
inline size_t gsplit_wgrad_lds_bytes(int C) { return (size_t)C * (GSW_WA + GSW_WB) * 32 + 32; }

template <int KS, int NP>
__global__ __launch_bounds__(256)
void gsplit_wgrad_kernel(const float* __restrict__ in, const float* __restrict__ dout, float* __restrict__ part, int N, int S, int C, int nsl)
{
    constexpr int KK = KS * KS, PAD = KS / 2, SEG = GSW_SEG, WA = GSW_WA, WB = GSW_WB, NIT = GSW_NIT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_gsw[];
    const int ky = blockIdx.x % KS, slice = blockIdx.x / KS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, kq = lane >> 4;
    const int nt = C / 16, npair = nt * nt, Q = C / 4;
    const int a_img = C * WA * 16, b_img = C * WB * 16;      // bytes of one hi (or lo) image
    unsigned char* s_ah = smem_gsw;                           // [hi, lo][C][WA][8 rows] halves
    unsigned char* s_bh = smem_gsw + 2 * a_img;               // [hi, lo][C][WB][8 rows] halves
    float* s_red = reinterpret_cast<float*>(s_bh + 2 * b_img);   // [input, gradient][4] wave maxima
    const int rgs = (S + 7) / 8, sgs = (S + SEG - 1) / SEG;
    const long long U = (long long)N * rgs * sgs;
    const long long u0 = U * slice / nsl, u1 = U * (slice + 1) / nsl;
    const int per = KK * C * C + C;
    // ---- staging items of this thread: item = (column, channel quad) of the input window (kind 0) or of the gradient (kind 1) ----
    const int nA = (SEG + KS - 1) * Q, nB = SEG * Q;
    int kind[NIT], ixl[NIT], ich[NIT], woff[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        int it = tid + 256 * i;
        kind[i] = it < nA ? 0 : (it < nA + nB ? 1 : 2);
        if (kind[i] == 1) it -= nA;
        ixl[i] = it / Q; ich[i] = 4 * (it % Q);
        woff[i] = kind[i] == 0 ? (ich[i] * WA + ixl[i]) * 16 : 2 * a_img + (ich[i] * WB + ixl[i]) * 16;
    }
    float4 rv[NIT][8];
    auto fetch = [&](long long u) {
        const int sg = (int)(u % sgs), rg = (int)((u / sgs) % rgs);
        const size_t n = (size_t)(u / ((long long)sgs * rgs));
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const float* base = (kind[i] == 0 ? in : dout) + n * S * S * C + ich[i];
            const int gx = sg * SEG + ixl[i] - (kind[i] == 0 ? PAD : 0);
            const int gy0 = rg * 8 + (kind[i] == 0 ? ky - PAD : 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gy = gy0 + j;
                const bool ok = kind[i] != 2 && (unsigned)gx < (unsigned)S && (unsigned)gy < (unsigned)S;
                rv[i][j] = ok ? *reinterpret_cast<const float4*>(base + ((size_t)gy * S + gx) * C) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    // fetched unit -> two scales -> hi / lo planes; its barrier ends every wave's reads of the previous unit.  Returns 1 / (scale_a scale_b),
    // inv_b = 1 / scale_b (the bias sum carries the gradient's scale only)
    auto stage = [&](float& inv_b) -> float {
        float ma = 0.f, mb = 0.f;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                m = fmaxf(fmaxf(m, fmaxf(fabsf(rv[i][j].x), fabsf(rv[i][j].y))), fmaxf(fabsf(rv[i][j].z), fabsf(rv[i][j].w)));
            if (kind[i] == 0) ma = fmaxf(ma, m); else mb = fmaxf(mb, m);
        }
        ma = wave_max_f32(ma); mb = wave_max_f32(mb);
        if (lane == 0) { s_red[wv] = ma; s_red[4 + wv] = mb; }
        __syncthreads();
        const float sa = tile_scale(fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])), 1.f);
        const float sb = tile_scale(fmaxf(fmaxf(s_red[4], s_red[5]), fmaxf(s_red[6], s_red[7])), 1.f);
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            if (kind[i] == 2) continue;
            const float sc = kind[i] == 0 ? sa : sb;
            const int chs = (kind[i] == 0 ? WA : WB) * 16, lod = kind[i] == 0 ? a_img : b_img;
            auto put = [&](int c, float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
                uint4 hi, lo;
                hi.x = pack_hi_lo(v0 * sc, v1 * sc, lo.x); hi.y = pack_hi_lo(v2 * sc, v3 * sc, lo.y);
                hi.z = pack_hi_lo(v4 * sc, v5 * sc, lo.z); hi.w = pack_hi_lo(v6 * sc, v7 * sc, lo.w);
                unsigned char* d = smem_gsw + woff[i] + c * chs;
                *reinterpret_cast<uint4*>(d) = hi;
                *reinterpret_cast<uint4*>(d + lod) = lo;
            };
            put(0, rv[i][0].x, rv[i][1].x, rv[i][2].x, rv[i][3].x, rv[i][4].x, rv[i][5].x, rv[i][6].x, rv[i][7].x);
            put(1, rv[i][0].y, rv[i][1].y, rv[i][2].y, rv[i][3].y, rv[i][4].y, rv[i][5].y, rv[i][6].y, rv[i][7].y);
            put(2, rv[i][0].z, rv[i][1].z, rv[i][2].z, rv[i][3].z, rv[i][4].z, rv[i][5].z, rv[i][6].z, rv[i][7].z);
            put(3, rv[i][0].w, rv[i][1].w, rv[i][2].w, rv[i][3].w, rv[i][4].w, rv[i][5].w, rv[i][6].w, rv[i][7].w);
        }
        inv_b = 1.f / sb;
        return (1.f / sa) * inv_b;
    };
    // ---- the (ci tile, co tile) pairs of this wave ----
    bool pon[NP], pbias[NP];
    int aoff[NP], boff[NP];
    f32x4 acc[NP][KS], bacc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = wv + 4 * i;
        pon[i] = p < npair;
        const int cit = pon[i] ? p / nt : 0, cot = pon[i] ? p % nt : 0;
        pbias[i] = pon[i] && ky == 0 && cit == 0;
        aoff[i] = ((cit * 16 + r16) * WA + kq) * 16;
        boff[i] = 2 * a_img + ((cot * 16 + r16) * WB + kq) * 16;
        bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) acc[i][kx] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (_Float16)1.0f;
    if (u0 < u1) fetch(u0);
    for (long long u = u0; u < u1; ++u) {
        float fb;
        const float f = stage(fb);
        __syncthreads();                                      // planes complete
        if (u + 1 < u1) fetch(u + 1);                         // in flight under this unit's MFMAs
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (!pon[i]) continue;                            // (wave-uniform)
            f32x4 tacc[KS], tb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) tacc[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int x0 = 0; x0 < SEG; x0 += 4) {
                const f16x8 bh = *reinterpret_cast<const f16x8*>(smem_gsw + boff[i] + x0 * 16);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(smem_gsw + boff[i] + b_img + x0 * 16);
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const f16x8 ah = *reinterpret_cast<const f16x8*>(s_ah + aoff[i] + (x0 + kx) * 16);
                    const f16x8 al = *reinterpret_cast<const f16x8*>(s_ah + aoff[i] + a_img + (x0 + kx) * 16);
                    tacc[kx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, tacc[kx], 0, 0, 0);
                    tacc[kx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, tacc[kx], 0, 0, 0);
                    tacc[kx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, tacc[kx], 0, 0, 0);
                }
                if (pbias[i]) {                               // (wave-uniform) every row of the result: sum over the 32 pixels
                    tb = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, bl, tb, 0, 0, 0);
                    tb = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, bh, tb, 0, 0, 0);
                }
            }
#pragma unroll
            for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][kx][j] = fmaf(tacc[kx][j], f, acc[i][kx][j]);
            bacc[i][0] = fmaf(tb[0], fb, bacc[i][0]);
        }
    }
    float* pw = part + (size_t)slice * per;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (!pon[i]) continue;
        const int p = wv + 4 * i, cit = p / nt, cot = p % nt;
        const int co = cot * 16 + r16;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx)
#pragma unroll
            for (int j = 0; j < 4; ++j) pw[((size_t)(ky * KS + kx) * C + cit * 16 + 4 * kq + j) * C + co] = acc[i][kx][j];
        if (pbias[i] && kq == 0) pw[(size_t)KK * C * C + co] = bacc[i][0];
    }
}

}  // namespace

// chunk width of the split kernel for a conv k x k, C -> C: 32 (one tap per MFMA) when the channel count allows it and the LDS holds the
// slice beside a 32-channel halo, else 16 (two taps per MFMA); 0 = the shape stays on the fp32 kernels
int gen_split_cch(int k, int C)
{
    if ((k != 3 && k != 5 && k != 7) || C < 16 || (C & 15)) return 0;
    if (C % 32 == 0 && gsplit_lds_bytes(k, C, 32) <= 160 * 1024) return 32;
    return gsplit_lds_bytes(k, C, 16) <= 160 * 1024 ? 16 : 0;
}

size_t gen_split_pack_bytes(int k, int C)
{
    const int cch = gen_split_cch(k, C);
    return cch ? wpk_gen_split_bytes(k, C, cch) : 0;
}

// wt: the generic pack [tap][ci][co] of a C -> C layer; dgrad = 1: the slices of the data gradient (flipped taps, reduction over co)
hipError_t launch_gen_split_pack(hipStream_t st, const float* wt, int k, int C, int dgrad, void* dst, float* meta)
{
    const int cch = gen_split_cch(k, C);
    if (!cch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gsplit_pack_kernel, dim3(C / 16), dim3(256), 0, st, wt, k * k, C, cch, dgrad, C * C, dgrad ? 1 : C, dgrad ? C : 1,
                       reinterpret_cast<unsigned*>(dst), meta);
    return hipGetLastError();
}

// split weight + bias gradient: covered where the forward kernel is and the (ci, co) tile pairs fit four waves' registers (C <= 64)
bool gen_split_wgrad_ok(int k, int C) { return gen_split_cch(k, C) != 0 && C <= 64 && (k < 7 || C <= 32) && gsplit_wgrad_lds_bytes(C) <= 160 * 1024; }

// gw [C][C][k][k] += alpha dW, gb [C] += alpha db; scratch: gen_wgrad_scratch_floats(C, C, k) floats (partials of <= GEN_WGRAD_SLICES_MAX slices)
hipError_t launch_gen_split_wgrad(hipStream_t st, const float* in, const float* dout, float* scratch, int N, int S, int C, int k, float alpha,
                                  float* gw, float* gb)
{
    if (!gen_split_wgrad_ok(k, C)) return hipErrorInvalidValue;
    int n_cu = 0;
    if (hipError_t e = iod_cu_count(&n_cu); e != hipSuccess) return e;
    const long long U = (long long)N * ((S + 7) / 8) * ((S + GSW_SEG - 1) / GSW_SEG);
    const int per_cu = gsplit_wgrad_lds_bytes(C) <= 80 * 1024 ? 2 : 1;
    const int nsl = (int)std::max<long long>(1, std::min<long long>(std::min(GEN_WGRAD_SLICES_MAX, per_cu * n_cu / k), U));
    const int np = (C / 16) * (C / 16) <= 4 ? 1 : 4;         // tile pairs per wave (7 x 7: C <= 32, always one)
    const hipError_t e = iod_dispatch<3, 5, 7>(k, [&](auto ks) {
        return iod_dispatch<1, 4>(np, [&](auto npc) {
            if constexpr (ks < 7 || npc == 1)
                return iod_launch<gsplit_wgrad_kernel<ks, npc>>(st, dim3(ks * nsl), dim3(256), gsplit_wgrad_lds_bytes(C), 160 * 1024, in, dout, scratch,
                                                                N, S, C, nsl);
            else
                return hipErrorInvalidValue;
        });
    });
    if (e != hipSuccess) return e;
    return launch_gen_wgrad_reduce(st, scratch, nsl, C, C, C, k * k, alpha, gw, gb);
}

// out = act(bias + conv(in)) (bias, elu) or ELU'(aux) x data gradient (aux), in / out / aux [N][S][S][C]
hipError_t launch_gen_split_conv(hipStream_t st, const float* in, const void* wpk, const float* wmeta, const float* bias, const float* aux,
                                 float* out, int N, int S, int C, int k, int elu)
{
    const int cch = gen_split_cch(k, C);
    if (!cch) return hipErrorInvalidValue;
    return iod_dispatch<3, 5, 7>(k, [&](auto ks) {               // (gen_split_cch: k is 3, 5 or 7, cch 32 or 16)
        return iod_dispatch<32, 16>(cch, [&](auto cc) { return gsplit_launch<ks, cc>(st, in, wpk, wmeta, bias, aux, out, N, S, C, elu); });
    });
}
