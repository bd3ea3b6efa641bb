// Refinement restarts (include/iodine_hip.h: iodine_chain_score, iodine_chain_consensus): C decodes of the same B images - the chains of
// IODINE.restarts, row c B + b as reconstruct returns them - scored against the image, labelled, and folded into one labelling.  Stateless
// like kernels_objects.hip: no handle, no workspace, NCHW fp32 in, no float atomics, nothing synchronises.
//
// chain_score_kernel<W, JOINT>: one block per (image b, group of chains).  A thread owns the pixels tid, tid + 1024, .. (vectors of W) of
// its image and loops over the chains of its group, so an image and its weights are fetched from HBM once per group and every mask and
// mean plane once; the launcher cuts the C chains into just enough groups to put a block on every CU, and a chain's sum never leaves its
// block, so the grouping changes speed only.  Per pixel and chain, over the slots in index order:
//   * the arg-max of the mask, strict `v > best` from -inf upwards (slot_table_kernel's rule: lowest index on a tie, a NaN never wins);
//   * a_kc = logf(m_k + 1e-12f) + l_kc, l_kc = -(x_c - mu_kc)^2 inv2s2 + lconst (pixel_terms.h), into a running logsumexp per channel
//     (JOINT: one, over a_k = logf(..) + ((l_k0 + l_k1) + l_k2)): the maximum so far is subtracted from every exponent and the sum is
//     rescaled when the maximum rises, so no exponent is above 0 and nothing per slot has to stay in registers (K is a run-time 1..16).
//     The bounded exponential is v_exp_f32(x log2 e) as in pixel_terms.h's default path; the two logarithms are libm's.
//   * w_p LL_p in fp64 (the product is exact), added per thread in pixel order, per wave in a fixed xor butterfly, across the 16 waves in
//     index order on thread 0: the same input gives the same bits on every call.
//
// chain_votes_kernel<W>: grid (blocks of 256 W pixels, image); the image's perm rows sit in LDS as bytes (255 = outside 0..K-1), next to,
// per chain and common slot j, the bit set of the chain's slots that map to j.  A thread owns W pixels: it counts the relabelled labels
// of the C chains in sixteen 16-bit fields (C <= 1024 fits), writes votes / consensus / agreement, then forms mask_mean slot by slot,
// adding mask[c][i] for the i of chain c's bit set, c ascending, i ascending - every mask plane is read once.
// chain_match_kernel<W>: one block per (chain, image) counts the pixels on which the chain and the image's reference chain carry the same
// valid common label; integer sums, one division.
// Device data is never an index unchecked: labels and perm / ref entries outside their range drop out before they address anything.
#include "common.h"

static constexpr int CHN_THREADS = 1024;
static constexpr int CHN_WAVES = CHN_THREADS / 64;
static constexpr int CHN_TARGET_BLOCKS = 256;                 // one block of 16 waves per CU
static constexpr int CNS_THREADS = 256;
static constexpr int CNS_MAX_SLOTS = 16;

// one term of a running logsumexp: (mx, s) stand for mx + log s; every exponent is <= 0.  From (-inf, 0) the first term gives (a, 1).
IOD_DEVINL void chn_lse_step(float a, float& mx, float& s)
{
    const bool up = a > mx;
    const float e = __builtin_amdgcn_exp2f((up ? mx - a : a - mx) * 1.44269504088896341f);
    s = up ? fmaf(s, e, 1.f) : s + e;
    mx = up ? a : mx;
}

// W = 4: P % 4 == 0 and every base pointer aligned for its vector (launch_chain_score decides); W = 1: anything.
template <int W, bool JOINT>
__global__ __launch_bounds__(CHN_THREADS)
void chain_score_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ mask,
                        const float* __restrict__ mean, int C, int B, int K, int P, int G, float inv2s2, float lconst,
                        float* __restrict__ ll, unsigned char* __restrict__ seg)
{
    constexpr int NS = JOINT ? 1 : 3;
    __shared__ double s_red[2][CHN_WAVES];                    // two sets: one barrier per chain
    const int b = blockIdx.x / G, g = blockIdx.x - b * G, tid = threadIdx.x;
    const int q = C / G, r = C - q * G;                       // balanced: the first r groups take q + 1 chains
    const int c0 = g * q + min(g, r), c1 = c0 + q + (g < r ? 1 : 0);
    const size_t sP = (size_t)P;
    const float* xb = x + (size_t)b * 3 * sP;
    const float* wb = w ? w + (size_t)b * sP : nullptr;
    const int nvec = P / W;                                   // W == 4 only where P % 4 == 0

    for (int c = c0; c < c1; ++c) {
        const size_t row = (size_t)c * B + b;
        const float* mb = mask + row * K * sP;
        const float* ub = mean + row * K * 3 * sP;
        unsigned char* sb = seg ? seg + row * sP : nullptr;
        double acc = 0.0;
        for (int v = tid; v < nvec; v += CHN_THREADS) {
            const size_t p0 = (size_t)v * W;
            float xs[3][W], wt[W];
            if (ll) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) vec_load<W>(xb + ch * sP + p0, xs[ch]);
                if (wb) vec_load<W>(wb + p0, wt);
            }
            float mx[NS][W], sm[NS][W], bv[W];
            int best[W];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                bv[j] = -INFINITY; best[j] = 0;
#pragma unroll
                for (int n = 0; n < NS; ++n) { mx[n][j] = -INFINITY; sm[n][j] = 0.f; }
            }
#pragma unroll 2
            for (int k = 0; k < K; ++k) {
                float m[W];
                vec_load<W>(mb + (size_t)k * sP + p0, m);
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (m[j] > bv[j]) { bv[j] = m[j]; best[j] = k; }
                if (!ll) continue;
                float mu[3][W];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) vec_load<W>(ub + ((size_t)k * 3 + ch) * sP + p0, mu[ch]);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const float lm = logf(m[j] + 1e-12f);
                    float l[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float d = xs[ch][j] - mu[ch][j];
                        l[ch] = -(d * d) * inv2s2 + lconst;
                    }
                    if constexpr (JOINT) {
                        chn_lse_step(lm + ((l[0] + l[1]) + l[2]), mx[0][j], sm[0][j]);
                    } else {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) chn_lse_step(lm + l[ch], mx[ch][j], sm[ch][j]);
                    }
                }
            }
            if (ll) {
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    float t = mx[0][j] + logf(sm[0][j]);
                    if constexpr (!JOINT) t = (t + (mx[1][j] + logf(sm[1][j]))) + (mx[2][j] + logf(sm[2][j]));
                    acc += (wb ? (double)wt[j] : 1.0) * (double)t;
                }
            }
            if (sb) {
                if constexpr (W == 4)
                    *reinterpret_cast<uchar4*>(sb + p0) = make_uchar4((unsigned char)best[0], (unsigned char)best[1],
                                                                      (unsigned char)best[2], (unsigned char)best[3]);
                else
                    sb[p0] = (unsigned char)best[0];
            }
        }
        if (!ll) continue;                                    // (block-uniform: no barrier is skipped by a part of the block)
        acc = wave_sum(acc);
        const int set = (c - c0) & 1;
        if ((tid & 63) == 0) s_red[set][tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            double a = 0.0;
#pragma unroll 1
            for (int i = 0; i < CHN_WAVES; ++i) a += s_red[set][i];
            ll[row] = (float)a;
        }
    }
}

hipError_t launch_chain_score(hipStream_t st, const float* x, const float* w, const float* mask, const float* mean, int C, int B, int K,
                              int S, double sigma, int joint, float* ll, unsigned char* seg)
{
    const int P = S * S;
    const int G = std::max(1, std::min(C, (CHN_TARGET_BLOCKS + B - 1) / B));
    if ((long long)B * G > 0x7fffffffLL) return hipErrorInvalidValue;
    const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const bool vec = P % 4 == 0 && a16(x) && a16(w) && a16(mask) && a16(mean) && ((uintptr_t)seg & 3) == 0;
    const float inv2s2 = (float)(1.0 / (2.0 * sigma * sigma));
    const float lconst = (float)(-log(sigma) - 0.5 * log(2.0 * M_PI));
    const dim3 grid((unsigned)B * (unsigned)G), block(CHN_THREADS);
#define CS(WW, JT) hipLaunchKernelGGL((chain_score_kernel<WW, JT>), grid, block, 0, st, x, w, mask, mean, C, B, K, P, G, inv2s2, lconst, ll, seg)
    if (vec) { if (joint) CS(4, true); else CS(4, false); }
    else { if (joint) CS(1, true); else CS(1, false); }
#undef CS
    return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------
// consensus of C labelled chains
// -----------------------------------------------------------------------------------------------
IOD_DEVINL unsigned chn_relabel(const unsigned char* __restrict__ perm_row, unsigned label, int K)
{
    return label < (unsigned)K ? perm_row[label] : 255u;      // perm_row holds 255 for an entry outside 0..K-1
}

// dynamic LDS: C * 16 bytes of perm, then C * 16 uint16 bit sets (slots of chain c that map to common slot j)
template <int W>
__global__ __launch_bounds__(CNS_THREADS)
void chain_votes_kernel(const unsigned char* __restrict__ seg, const int* __restrict__ perm, const float* __restrict__ mask, int C, int B,
                        int K, int P, int nblk, int* __restrict__ votes, unsigned char* __restrict__ consensus,
                        float* __restrict__ agreement, float* __restrict__ mask_mean)
{
    extern __shared__ __align__(16) unsigned char s_raw[];
    unsigned char* s_perm = s_raw;
    unsigned short* s_inv = reinterpret_cast<unsigned short*>(s_raw + (size_t)C * CNS_MAX_SLOTS);
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, tid = threadIdx.x;
    const size_t sP = (size_t)P;
    for (int i = tid; i < C * CNS_MAX_SLOTS; i += CNS_THREADS) {
        const int c = i >> 4, k = i & 15;
        int t = 255;
        if (k < K) {
            const int pv = perm[((size_t)c * B + b) * K + k];
            if (pv >= 0 && pv < K) t = pv;
        }
        s_perm[i] = (unsigned char)t;
    }
    __syncthreads();
    if (mask_mean)
        for (int i = tid; i < C * CNS_MAX_SLOTS; i += CNS_THREADS) {
            const int c = i >> 4, j = i & 15;
            unsigned bits = 0;
            for (int k = 0; k < K; ++k) bits |= s_perm[c * CNS_MAX_SLOTS + k] == j ? 1u << k : 0u;
            s_inv[i] = (unsigned short)bits;
        }
    __syncthreads();

    const int v = blk * CNS_THREADS + tid;
    if (v >= P / W) return;
    const size_t p0 = (size_t)v * W;

    if (votes || consensus || agreement) {
        unsigned long long cnt[W][4];                         // sixteen 16-bit counters per pixel: a chain adds 1 to one of them, C <= 1024
#pragma unroll
        for (int j = 0; j < W; ++j) { cnt[j][0] = 0; cnt[j][1] = 0; cnt[j][2] = 0; cnt[j][3] = 0; }
        for (int c = 0; c < C; ++c) {
            const unsigned char* sc = seg + ((size_t)c * B + b) * sP + p0;
            unsigned lab;
            if constexpr (W == 4) lab = *reinterpret_cast<const unsigned*>(sc);
            else lab = *sc;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const unsigned t = chn_relabel(s_perm + c * CNS_MAX_SLOTS, (lab >> (8 * j)) & 255u, K);
                const unsigned long long one = t < (unsigned)K ? 1ull << (16 * (t & 3)) : 0ull;
                const unsigned word = t >> 2;
#pragma unroll
                for (int n = 0; n < 4; ++n) cnt[j][n] += word == (unsigned)n ? one : 0ull;
            }
        }
        int top[W], win[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { top[j] = 0; win[j] = 0; }
#pragma unroll
        for (int k = 0; k < CNS_MAX_SLOTS; ++k) {
            if (k < K) {
                int n[W];
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    n[j] = (int)((cnt[j][k >> 2] >> (16 * (k & 3))) & 0xffffull);
                    if (n[j] > top[j]) { top[j] = n[j]; win[j] = k; }         // lowest index on a tie
                }
                if (votes) {
                    int* vp = votes + ((size_t)b * K + k) * sP + p0;
                    if constexpr (W == 4) *reinterpret_cast<int4*>(vp) = make_int4(n[0], n[1], n[2], n[3]);
                    else *vp = n[0];
                }
            }
        }
        if (consensus) {
            unsigned char* cp = consensus + (size_t)b * sP + p0;
            if constexpr (W == 4)
                *reinterpret_cast<uchar4*>(cp) = make_uchar4((unsigned char)win[0], (unsigned char)win[1], (unsigned char)win[2],
                                                             (unsigned char)win[3]);
            else *cp = (unsigned char)win[0];
        }
        if (agreement) {
            float* ap = agreement + (size_t)b * sP + p0;
            const float fc = (float)C;
            if constexpr (W == 4) *reinterpret_cast<float4*>(ap) = make_float4((float)top[0] / fc, (float)top[1] / fc, (float)top[2] / fc, (float)top[3] / fc);
            else *ap = (float)top[0] / fc;
        }
    }

    if (mask_mean) {
        const float fc = (float)C;
        for (int j = 0; j < K; ++j) {
            float acc[W];
#pragma unroll
            for (int n = 0; n < W; ++n) acc[n] = 0.f;
            for (int c = 0; c < C; ++c) {
                unsigned bits = s_inv[c * CNS_MAX_SLOTS + j];                   // block-uniform
                while (bits) {
                    const int i = __ffs((int)bits) - 1;                         // < K by construction
                    bits &= bits - 1;
                    float m[W];
                    vec_load<W>(mask + (((size_t)c * B + b) * K + i) * sP + p0, m);
#pragma unroll
                    for (int n = 0; n < W; ++n) acc[n] += m[n];
                }
            }
            float* op = mask_mean + ((size_t)b * K + j) * sP + p0;
            if constexpr (W == 4) *reinterpret_cast<float4*>(op) = make_float4(acc[0] / fc, acc[1] / fc, acc[2] / fc, acc[3] / fc);
            else *op = acc[0] / fc;
        }
    }
}

template <int W>
__global__ __launch_bounds__(CNS_THREADS)
void chain_match_kernel(const unsigned char* __restrict__ seg, const int* __restrict__ perm, const int* __restrict__ ref, int C, int B,
                        int K, int P, float* __restrict__ match)
{
    __shared__ unsigned char s_perm[2][CNS_MAX_SLOTS];        // 0: this chain, 1: the image's reference chain
    __shared__ unsigned s_cnt[CNS_THREADS / 64];
    const int row = blockIdx.x, c = row / B, b = row - c * B, tid = threadIdx.x;
    const int rc = ref[b];
    const bool has_ref = rc >= 0 && rc < C;                   // block-uniform
    if (!has_ref) {                                           // no reference chain: nothing can be counted
        if (tid == 0) match[row] = 0.f;
        return;
    }
    if (tid < 2 * CNS_MAX_SLOTS) {
        const int which = tid >> 4, k = tid & 15;
        int t = 255;
        if (k < K) {
            const int pv = perm[((size_t)(which ? rc : c) * B + b) * K + k];
            if (pv >= 0 && pv < K) t = pv;
        }
        s_perm[which][k] = (unsigned char)t;
    }
    __syncthreads();
    const unsigned char* sa = seg + (size_t)row * P;
    const unsigned char* sr = seg + ((size_t)rc * B + b) * P;
    unsigned n = 0;
    for (int v = tid; v < P / W; v += CNS_THREADS) {
        unsigned la, lr;
        if constexpr (W == 4) {
            la = *reinterpret_cast<const unsigned*>(sa + (size_t)v * 4);
            lr = *reinterpret_cast<const unsigned*>(sr + (size_t)v * 4);
        } else {
            la = sa[v]; lr = sr[v];
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned ta = chn_relabel(s_perm[0], (la >> (8 * j)) & 255u, K);
            const unsigned tr = chn_relabel(s_perm[1], (lr >> (8 * j)) & 255u, K);
            n += (ta < (unsigned)K && ta == tr) ? 1u : 0u;
        }
    }
    n = wave_sum(n);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = n;
    __syncthreads();
    if (tid != 0) return;
    unsigned total = 0;
#pragma unroll
    for (int i = 0; i < CNS_THREADS / 64; ++i) total += s_cnt[i];
    match[row] = (float)((double)total / (double)P);
}

hipError_t launch_chain_consensus(hipStream_t st, const unsigned char* seg, const int* perm, const int* ref, const float* mask, int C,
                                  int B, int K, int S, int* votes, unsigned char* consensus, float* agreement, float* match,
                                  float* mask_mean)
{
    const int P = S * S;
    const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const auto a4 = [](const void* p) { return ((uintptr_t)p & 3) == 0; };
    if (votes || consensus || agreement || mask_mean) {
        const bool vec = P % 4 == 0 && a4(seg) && a16(mask) && a16(votes) && a4(consensus) && a16(agreement) && a16(mask_mean);
        const int per = CNS_THREADS * (vec ? 4 : 1);
        const int nblk = (P + per - 1) / per;
        if ((long long)B * nblk > 0x7fffffffLL) return hipErrorInvalidValue;
        const size_t lds = (size_t)C * CNS_MAX_SLOTS * 3;     // bytes of perm + uint16 bit sets
        const dim3 grid((unsigned)B * (unsigned)nblk), block(CNS_THREADS);
        if (vec)
            hipLaunchKernelGGL(chain_votes_kernel<4>, grid, block, lds, st, seg, perm, mask, C, B, K, P, nblk, votes, consensus, agreement, mask_mean);
        else
            hipLaunchKernelGGL(chain_votes_kernel<1>, grid, block, lds, st, seg, perm, mask, C, B, K, P, nblk, votes, consensus, agreement, mask_mean);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (match) {
        const dim3 grid((unsigned)C * (unsigned)B), block(CNS_THREADS);
        if (P % 4 == 0 && a4(seg))
            hipLaunchKernelGGL(chain_match_kernel<4>, grid, block, 0, st, seg, perm, ref, C, B, K, P, match);
        else
            hipLaunchKernelGGL(chain_match_kernel<1>, grid, block, 0, st, seg, perm, ref, C, B, K, P, match);
    }
    return hipGetLastError();
}
