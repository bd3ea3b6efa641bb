// Adaptive refinement (include/iodine_hip.h: iodine_adaptive_select, iodine_adaptive_move): the two device steps between two rounds of
// iodine_reconstruct_adaptive - which images stop, and the rows of the state that follow them.  Stateless like kernels_chains.hip: plain
// pointers, no handle, no workspace, no atomics, nothing synchronises; plain HIP C++.
//
// adaptive_select_kernel: ONE block of 1024 threads = 16 waves walks the n active images in chunks of 1024, position order.  A thread
// scatters its image's R x {ll, kl} into the traces, applies the stopping rule (tests/adaptive_reference.py) and votes; a wave's ballot
// and the popcount of the lanes below give the rank within the wave, the 16 per-wave counts in LDS the rank within the chunk, and the
// running offsets of the chunks before are carried in LDS.  The two lists (continue / stop) therefore keep position order - a stable
// compaction - and the same input gives the same bits on every call, for any n >= 1.
// The rule's fp64 expression is evaluated with __dmul_rn / __dadd_rn / __dsub_rn: one multiply, one add, one subtract, one compare and
// no fused multiply-add, whatever the compiler's contraction setting, so that it matches numpy bit for bit.
//
// adaptive_move_kernel<W>: grid (blocks, entry).  Entry e copies `rows` rows of row_floats floats, row r from src row src_index[r] (r
// without an index) to dst row dst_index[r]; W = 4 moves float4 where the row size and both base pointers allow it (the launcher
// decides per entry).  An index outside its array's extent moves nothing: device data is never an address unchecked.  Source and
// destination of an entry never overlap (the entry point refuses): a block may read a row long after another block wrote its own.
#include "common.h"

static constexpr int ADS_THREADS = 1024;
static constexpr int ADS_WAVES = ADS_THREADS / 64;
static constexpr int ADM_THREADS = 256;

__global__ __launch_bounds__(ADS_THREADS)
void adaptive_select_kernel(const float* __restrict__ terms, const int* __restrict__ idx_in, int n, int R, int t, int B, AdaptiveRule rule,
                            const int* __restrict__ budget, int* __restrict__ idx_out, int* __restrict__ pos_out, int* __restrict__ stop_idx,
                            int* __restrict__ stop_pos, int* __restrict__ counts, int* __restrict__ iters, float* __restrict__ ll,
                            float* __restrict__ kl)
{
    __shared__ int s_cont[ADS_WAVES], s_stop[ADS_WAVES];
    __shared__ int s_base[2];                                 // images before this chunk: {continue, stop}
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_base[0] = 0; s_base[1] = 0; }
    __syncthreads();
    const bool last = t >= rule.max_iters;
    const bool check = !last && t % rule.check_every == 0;    // decisions are taken after R, 2R, .. updates only
    const bool by_score = check && t >= (rule.min_iters > 2 ? rule.min_iters : 2);
    for (int p0 = 0; p0 < n; p0 += ADS_THREADS) {
        const int p = p0 + tid;
        const bool active = p < n;
        bool stop = false;
        int orig = 0;
        if (active) {
            orig = idx_in ? idx_in[p] : p;
            const bool ok = (unsigned)orig < (unsigned)B;     // (an index outside the batch addresses nothing and stops)
            stop = last || !ok;
            if (ok) {
                for (int r = 0; r < R; ++r) {
                    const size_t row = (size_t)(t - R + r) * B + orig, e = ((size_t)r * n + p) * 2;
                    ll[row] = terms[e];
                    kl[row] = terms[e + 1];
                }
                if (check && budget && t >= budget[orig]) stop = true;
                if (by_score && !stop) {
                    // s_{t-1} is the round's last evaluation; s_{t-2} the one before it, or (R = 1) what the round before left in the traces
                    const size_t e1 = ((size_t)(R - 1) * n + p) * 2;
                    const double ll1 = (double)terms[e1], kl1 = (double)terms[e1 + 1];
                    double ll0, kl0;
                    if (R >= 2) {
                        const size_t e0 = ((size_t)(R - 2) * n + p) * 2;
                        ll0 = (double)terms[e0]; kl0 = (double)terms[e0 + 1];
                    } else {
                        const size_t row0 = (size_t)(t - 2) * B + orig;
                        ll0 = (double)ll[row0]; kl0 = (double)kl[row0];
                    }
                    const double s1 = __dsub_rn(ll1, __dmul_rn(rule.beta, kl1)), s0 = __dsub_rn(ll0, __dmul_rn(rule.beta, kl0));
                    const double lhs = __dsub_rn(s1, s0), rhs = __dadd_rn(rule.tol, __dmul_rn(rule.rtol, fabs(s0)));
                    stop = lhs < rhs;                         // (false with a NaN on either side: the image continues)
                }
            }
        }
        const unsigned long long bs = __ballot(active && stop), bc = __ballot(active && !stop);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) { s_stop[wave] = __popcll(bs); s_cont[wave] = __popcll(bc); }
        __syncthreads();
        int oc = s_base[0], os = s_base[1];
        for (int w = 0; w < wave; ++w) { oc += s_cont[w]; os += s_stop[w]; }
        if (active) {
            if (stop) {
                const int j = os + __popcll(bs & below);
                stop_pos[j] = p; stop_idx[j] = orig;
                if ((unsigned)orig < (unsigned)B) iters[orig] = t;
            } else {
                const int j = oc + __popcll(bc & below);
                pos_out[j] = p; idx_out[j] = orig;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int c = 0, s = 0;
            for (int w = 0; w < ADS_WAVES; ++w) { c += s_cont[w]; s += s_stop[w]; }
            s_base[0] += c; s_base[1] += s;
        }
        __syncthreads();
    }
    if (tid == 0) { counts[0] = s_base[0]; counts[1] = s_base[1]; }
}

hipError_t launch_adaptive_select(hipStream_t st, const float* terms, const int* idx_in, int n, int R, int t, int B, const AdaptiveRule& rule,
                                  const int* budget, int* idx_out, int* pos_out, int* stop_idx, int* stop_pos, int* counts, int* iters,
                                  float* ll, float* kl)
{
    hipLaunchKernelGGL(adaptive_select_kernel, dim3(1), dim3(ADS_THREADS), 0, st, terms, idx_in, n, R, t, B, rule, budget, idx_out, pos_out,
                       stop_idx, stop_pos, counts, iters, ll, kl);
    return hipGetLastError();
}

struct MoveTable { MoveEntry e[ADAPTIVE_MOVE_MAX]; };

template <typename V>
IOD_DEVINL void adaptive_move_rows(const MoveEntry& e, long long per_row)
{
    const V* __restrict__ src = reinterpret_cast<const V*>(e.src);
    V* __restrict__ dst = reinterpret_cast<V*>(e.dst);
    const long long total = (long long)e.rows * per_row, step = (long long)gridDim.x * ADM_THREADS;
    for (long long i = (long long)blockIdx.x * ADM_THREADS + threadIdx.x; i < total; i += step) {
        const long long r = i / per_row, c = i - r * per_row;
        const int s = e.src_index ? e.src_index[r] : (int)r, d = e.dst_index ? e.dst_index[r] : (int)r;
        if ((unsigned)s >= (unsigned)e.src_rows || (unsigned)d >= (unsigned)e.dst_rows) continue;
        dst[(long long)d * per_row + c] = src[(long long)s * per_row + c];
    }
}

__global__ __launch_bounds__(ADM_THREADS)
void adaptive_move_kernel(MoveTable tab)
{
    const MoveEntry& e = tab.e[blockIdx.y];
    if (e.vec) adaptive_move_rows<float4>(e, e.row_floats / 4);
    else adaptive_move_rows<float>(e, e.row_floats);
}

// entries: src_rows / dst_rows are the extents in rows (>= 1); `vec` is decided here
hipError_t launch_adaptive_move(hipStream_t st, const MoveEntry* entries, int count)
{
    if (count < 1 || count > ADAPTIVE_MOVE_MAX) return hipErrorInvalidValue;
    MoveTable tab;
    long long most = 1;
    for (int i = 0; i < count; ++i) {
        MoveEntry e = entries[i];
        e.vec = e.row_floats % 4 == 0 && (((uintptr_t)e.src | (uintptr_t)e.dst) & 15) == 0;
        tab.e[i] = e;
        most = std::max(most, (long long)e.rows * (e.vec ? e.row_floats / 4 : e.row_floats));
    }
    for (int i = count; i < ADAPTIVE_MOVE_MAX; ++i) tab.e[i] = MoveEntry{nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0, 0};
    int cus = 256;
    if (hipError_t e = iod_cu_count(&cus); e != hipSuccess) return e;
    const long long want = (most + ADM_THREADS - 1) / ADM_THREADS;
    const unsigned gx = (unsigned)std::max(1LL, std::min(want, (long long)cus * 8));
    hipLaunchKernelGGL(adaptive_move_kernel, dim3(gx, (unsigned)count), dim3(ADM_THREADS), 0, st, tab);
    return hipGetLastError();
}
