// Object-level read-outs of the tensors reconstruct / decode / trajectory return (include/iodine_hip.h: iodine_slot_table,
// iodine_seg_overlap).  Stateless like launch_ari_table: no handle, no workspace, NCHW fp32 in.
//
// slot_table_kernel: one block per (image b, slot k).  Its 1024 threads stride the image in 16-byte vectors, read the K mask planes of
// their pixels to find the winner (strict `v > best` from -inf upwards: the lowest index wins a tie, a NaN never wins) and keep slot k's
// terms in registers.  The block of slot 0 also writes the segmentation map.  Every block of an image reads all K planes, so K - 1 of
// the K reads are meant to come from L2; the block-id remap below puts the blocks of one image on one XCD for that (speed only).
//
// Arithmetic: counts, sum of columns / rows and the box are integers (sum col <= 1023 * 2^20 / 2 < 2^32).  The soft sums add the <= 4
// non-negative fp32 terms of one vector in a fixed tree and continue in fp64: per thread in loop order, per wave in a fixed xor
// butterfly, across the 16 waves in index order on thread 0.  No atomics, no scratch: the same input gives the same bits.
#include "common.h"
#include <limits.h>

static constexpr int OBJ_THREADS = 1024;
static constexpr int OBJ_WAVES = OBJ_THREADS / 64;
static constexpr int OBJ_COLS = 14;

// fixed tree over the W terms of one vector
template <int W> IOD_DEVINL float obj_tree(const float (&v)[W])
{
    if constexpr (W == 4) return (v[0] + v[1]) + (v[2] + v[3]);
    else return v[0];
}

// W = 4: P % 4 == 0, S >= 4 and every base pointer aligned for its vector (launch_slot_table decides); W = 1: anything.
template <int W>
__global__ __launch_bounds__(OBJ_THREADS)
void slot_table_kernel(const float* __restrict__ mask, const float* __restrict__ mean, int K, int S, int P,
                       float* __restrict__ table, unsigned char* __restrict__ seg)
{
    __shared__ double s_d[OBJ_WAVES][6];
    __shared__ unsigned s_u[OBJ_WAVES][3];
    __shared__ int s_i[OBJ_WAVES][4];
    __shared__ float s_f[OBJ_WAVES];

    // blocks id, id + 8, ... share an XCD: give each such group a contiguous run of (b, k), so an image's K blocks read its planes through
    // one L2.  A bijection of [0, n) for every n; a different placement changes speed only.
    const int n = gridDim.x, id = blockIdx.x;
    const int xg = id & 7, q = n >> 3, r = n & 7;
    const int w = (xg < r ? xg * (q + 1) : r * (q + 1) + (xg - r) * q) + (id >> 3);
    const int b = w / K, k = w - b * K;
    const int tid = threadIdx.x;

    const float* mb = mask + (size_t)b * K * P;
    const float* cb = mean ? mean + ((size_t)b * K + k) * 3 * P : nullptr;
    unsigned char* sb = (seg && k == 0) ? seg + (size_t)b * P : nullptr;

    double a_area = 0.0, a_cx = 0.0, a_cy = 0.0, a_r = 0.0, a_g = 0.0, a_b = 0.0;
    float peak = -INFINITY;
    unsigned cnt = 0, sc = 0, sr = 0;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;

    const int nvec = P / W;                                   // W == 4 only where P % 4 == 0
    const int stride = OBJ_THREADS * W;
    const int dcol = stride % S, drow = stride / S;
    int col = (tid * W) % S, row = (tid * W) / S;             // of the vector's first pixel (tid * W < 4096 <= any P that reaches it)
    for (int v = tid; v < nvec; v += OBJ_THREADS) {
        const int p0 = v * W;
        float bv[W], mk[W];
        int best[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { bv[j] = -INFINITY; best[j] = 0; mk[j] = 0.f; }
#pragma unroll 4
        for (int kk = 0; kk < K; ++kk) {
            float m[W];
            vec_load<W>(mb + (size_t)kk * P + p0, m);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (m[j] > bv[j]) { bv[j] = m[j]; best[j] = kk; }
                if (kk == k) mk[j] = m[j];
            }
        }
        float tx[W], ty[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            int c = col + j, rr = row;
            if (c >= S) { c -= S; ++rr; }                     // W == 4 runs with S >= 4: one wrap at the most
            tx[j] = mk[j] * (float)c; ty[j] = mk[j] * (float)rr;
            peak = fmaxf(peak, mk[j]);
            if (best[j] == k) {
                ++cnt; sc += (unsigned)c; sr += (unsigned)rr;
                x0 = min(x0, c); x1 = max(x1, c); y0 = min(y0, rr); y1 = max(y1, rr);
            }
        }
        a_area += (double)obj_tree<W>(mk);
        a_cx += (double)obj_tree<W>(tx);
        a_cy += (double)obj_tree<W>(ty);
        if (cb) {
            float c0[W], c1[W], c2[W];
            vec_load<W>(cb + p0, c0);
            vec_load<W>(cb + (size_t)P + p0, c1);
            vec_load<W>(cb + 2 * (size_t)P + p0, c2);
#pragma unroll
            for (int j = 0; j < W; ++j) { c0[j] *= mk[j]; c1[j] *= mk[j]; c2[j] *= mk[j]; }
            a_r += (double)obj_tree<W>(c0);
            a_g += (double)obj_tree<W>(c1);
            a_b += (double)obj_tree<W>(c2);
        }
        if (sb) {
            if constexpr (W == 4)
                *reinterpret_cast<uchar4*>(sb + p0) = make_uchar4((unsigned char)best[0], (unsigned char)best[1],
                                                                  (unsigned char)best[2], (unsigned char)best[3]);
            else
                sb[p0] = (unsigned char)best[0];
        }
        col += dcol; row += drow;
        if (col >= S) { col -= S; ++row; }
    }

    // wave step: fixed butterflies; block step: thread 0, waves in index order
    a_area = wave_sum(a_area); a_cx = wave_sum(a_cx); a_cy = wave_sum(a_cy);
    a_r = wave_sum(a_r); a_g = wave_sum(a_g); a_b = wave_sum(a_b);
    cnt = wave_sum(cnt); sc = wave_sum(sc); sr = wave_sum(sr);
    x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
    peak = wave_max_f32(peak);
    const int wv = tid >> 6;
    if ((tid & 63) == 0) {
        s_d[wv][0] = a_area; s_d[wv][1] = a_cx; s_d[wv][2] = a_cy; s_d[wv][3] = a_r; s_d[wv][4] = a_g; s_d[wv][5] = a_b;
        s_u[wv][0] = cnt; s_u[wv][1] = sc; s_u[wv][2] = sr;
        s_i[wv][0] = x0; s_i[wv][1] = y0; s_i[wv][2] = x1; s_i[wv][3] = y1;
        s_f[wv] = peak;
    }
    __syncthreads();
    if (tid != 0) return;
    double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    cnt = 0; sc = 0; sr = 0; x0 = INT_MAX; y0 = INT_MAX; x1 = -1; y1 = -1; peak = -INFINITY;
#pragma unroll 1
    for (int i = 0; i < OBJ_WAVES; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) d[j] += s_d[i][j];
        cnt += s_u[i][0]; sc += s_u[i][1]; sr += s_u[i][2];
        x0 = min(x0, s_i[i][0]); y0 = min(y0, s_i[i][1]); x1 = max(x1, s_i[i][2]); y1 = max(y1, s_i[i][3]);
        peak = fmaxf(peak, s_f[i]);
    }
    float* t = table + ((size_t)b * K + k) * OBJ_COLS;
    const float area = (float)d[0];
    const bool soft = area != 0.f;
    t[0] = area;
    t[1] = (float)cnt;
    t[2] = soft ? (float)(d[1] / d[0]) : 0.f;
    t[3] = soft ? (float)(d[2] / d[0]) : 0.f;
    t[4] = cnt ? (float)((double)sc / (double)cnt) : -1.f;
    t[5] = cnt ? (float)((double)sr / (double)cnt) : -1.f;
    t[6] = cnt ? (float)x0 : -1.f;
    t[7] = cnt ? (float)y0 : -1.f;
    t[8] = cnt ? (float)x1 : -1.f;
    t[9] = cnt ? (float)y1 : -1.f;
    t[10] = soft && cb ? (float)(d[3] / d[0]) : 0.f;
    t[11] = soft && cb ? (float)(d[4] / d[0]) : 0.f;
    t[12] = soft && cb ? (float)(d[5] / d[0]) : 0.f;
    t[13] = peak;
}

hipError_t launch_slot_table(hipStream_t st, const float* mask, const float* mean, int B, int K, int S, float* table,
                             unsigned char* seg)
{
    const int P = S * S;
    const bool vec = P % 4 == 0 && S >= 4 && ((uintptr_t)mask & 15) == 0 && ((uintptr_t)mean & 15) == 0 && ((uintptr_t)seg & 3) == 0;
    const unsigned grid = (unsigned)B * (unsigned)K;
    if (vec)
        hipLaunchKernelGGL(slot_table_kernel<4>, dim3(grid), dim3(OBJ_THREADS), 0, st, mask, mean, K, S, P, table, seg);
    else
        hipLaunchKernelGGL(slot_table_kernel<1>, dim3(grid), dim3(OBJ_THREADS), 0, st, mask, mean, K, S, P, table, seg);
    return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------
// Contingency table of two label maps, table[b][i][j] = #{p : seg_a[b][p] == i and seg_b[b][p] == j}: int32 atomics on an LDS copy,
// one flush per block (as ari_table_kernel).  The labels are the caller's: one >= Ka or >= Kb is skipped before it indexes anything.
// W = 4: four labels per 32-bit load (P % 4 == 0, both maps 4-byte aligned).
// -----------------------------------------------------------------------------------------------
static constexpr int OVL_THREADS = 256;
static constexpr int OVL_MAX_SLOTS = 16;

template <int W>
__global__ __launch_bounds__(OVL_THREADS)
void seg_overlap_kernel(const unsigned char* __restrict__ seg_a, const unsigned char* __restrict__ seg_b, int Ka, int Kb, int P,
                        int bx, int* __restrict__ table)
{
    __shared__ int s_tab[OVL_MAX_SLOTS * OVL_MAX_SLOTS];
    const int b = blockIdx.x / bx, blk = blockIdx.x - b * bx, tid = threadIdx.x;
    const int cells = Ka * Kb;                                // <= 256: the entry point refuses more than 16 labels a side
    for (int i = tid; i < cells; i += OVL_THREADS) s_tab[i] = 0;
    __syncthreads();
    const unsigned char* pa = seg_a + (size_t)b * P;
    const unsigned char* pb = seg_b + (size_t)b * P;
    const int nvec = P / W;
    for (int v = blk * OVL_THREADS + tid; v < nvec; v += bx * OVL_THREADS) {
        unsigned la, lb;
        if constexpr (W == 4) {
            la = *reinterpret_cast<const unsigned*>(pa + (size_t)v * 4);
            lb = *reinterpret_cast<const unsigned*>(pb + (size_t)v * 4);
        } else {
            la = pa[v]; lb = pb[v];
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned i = (la >> (8 * j)) & 255u, c = (lb >> (8 * j)) & 255u;
            if (i < (unsigned)Ka && c < (unsigned)Kb) atomicAdd(&s_tab[i * Kb + c], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < cells; i += OVL_THREADS)
        if (s_tab[i]) atomicAdd(&table[(size_t)b * cells + i], s_tab[i]);
}

hipError_t launch_seg_overlap(hipStream_t st, const unsigned char* seg_a, const unsigned char* seg_b, int B, int Ka, int Kb, int P,
                              int* table)
{
    if (Ka < 1 || Kb < 1 || Ka > OVL_MAX_SLOTS || Kb > OVL_MAX_SLOTS) return hipErrorInvalidValue;   // the LDS table is 16 x 16
    hipError_t e = hipMemsetAsync(table, 0, sizeof(int) * (size_t)B * Ka * Kb, st);
    if (e != hipSuccess) return e;
    const bool vec = P % 4 == 0 && ((uintptr_t)seg_a & 3) == 0 && ((uintptr_t)seg_b & 3) == 0;
    const int per = OVL_THREADS * (vec ? 4 : 1) * 4;          // about four loads per thread
    const int bx = std::max(1, std::min((P + per - 1) / per, 64));
    const unsigned grid = (unsigned)B * (unsigned)bx;
    if (vec)
        hipLaunchKernelGGL(seg_overlap_kernel<4>, dim3(grid), dim3(OVL_THREADS), 0, st, seg_a, seg_b, Ka, Kb, P, bx, table);
    else
        hipLaunchKernelGGL(seg_overlap_kernel<1>, dim3(grid), dim3(OVL_THREADS), 0, st, seg_a, seg_b, Ka, Kb, P, bx, table);
    return hipGetLastError();
}
