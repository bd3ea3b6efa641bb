// Minimum-cost assignment of the real rows of a (G x K) fp32 cost matrix to its columns, G, K <= 16: the one function behind
// iodine_assign, iodine_assign_host and iodine_mask_match (include/iodine_hip.h).  Host and device run the same code.
//
// Problem: R = rows with valid[g] != 0 (all rows when valid is NULL), M = min(|R|, K).  Find an injective map pi from exactly M rows of R
// to columns that minimises sum cost[g][pi(g)].  |R| <= K: every real row is matched; |R| > K: every column is, and the solver runs on the
// transpose.  Unmatched and padding rows read -1.
//
// Method: shortest augmenting paths with row / column potentials (the O(n^2 m) Hungarian), potentials and reduced costs in fp64.  The only
// arithmetic is fp64 add / subtract / compare on values converted from fp32 - nothing a compiler may contract - so host and device return the
// same bits.  Ties: the lowest column index with the smallest reduced cost is taken (strict `<`), so the choice among equal-cost optima is a
// fixed function of the input.
//
// Bounded loops: every loop below runs a number of times fixed by G and K alone.  The path search marks one new column per step and is a
// `for` over at most m + 1 steps, the augmentation walks at most m + 1 links; neither is a `while` on data.  A non-finite cost in a real
// row is refused BEFORE the search (all -1, total NaN, return -1): with finite fp32 costs every reduced cost is a finite fp64 number (sums of
// <= 35 values below 2^129), every comparison is decided, and a free column is found within the step bound.  Should the search ever end
// without one (it cannot on finite input), the image is refused the same way instead of looping.
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IOD_ASSIGN_HD __host__ __device__ inline
#else
#define IOD_ASSIGN_HD inline
#endif

constexpr int IOD_ASSIGN_MAX = 16;

// The solver's working set: potentials, reduced-cost minima, the matching and the path links (17 entries each, index 0 = the virtual
// column).  The caller owns it - a stack object on the host, one LDS object per image on the device, so no thread-private array is indexed
// at run time there.
struct IodAssignWork {
    double u[IOD_ASSIGN_MAX + 1], v[IOD_ASSIGN_MAX + 1], minv[IOD_ASSIGN_MAX + 1];
    int p[IOD_ASSIGN_MAX + 1], way[IOD_ASSIGN_MAX + 1];       // p[j]: the row matched to column j (0: none)
    int rows[IOD_ASSIGN_MAX];                                 // the real rows, in order
};

// cost [G][K] row-major, valid [G] or NULL, assign [G] (out), total (out) = sum of the matched costs, added in fp64 in row order and rounded
// once.  Returns the number of matched rows M, or -1 when the matrix is refused.  1 <= G, K <= IOD_ASSIGN_MAX is the caller's to check.
IOD_ASSIGN_HD int iod_assign_solve(const float* cost, const unsigned char* valid, int G, int K, int* assign, float* total,
                                   IodAssignWork* work)
{
    constexpr int N = IOD_ASSIGN_MAX;
    int* rows = work->rows;
    double *u = work->u, *v = work->v, *minv = work->minv;
    int *p = work->p, *way = work->way;
    int nR = 0;
    for (int g = 0; g < G; ++g) {
        assign[g] = -1;
        if (!valid || valid[g]) rows[nR++] = g;
    }
    bool bad = false;
    for (int r = 0; r < nR; ++r)
        for (int k = 0; k < K; ++k)
            if (!(fabsf(cost[rows[r] * K + k]) <= FLT_MAX)) bad = true;        // NaN and +-inf both fail this
    if (bad) { *total = NAN; return -1; }
    if (nR == 0) { *total = 0.f; return 0; }

    const bool tr = nR > K;                                   // more real rows than columns: rows and columns swap roles
    const int n = tr ? K : nR, m = tr ? nR : K;               // n <= m; row i (1-based) is matched to a column j (1-based)
    for (int j = 0; j <= N; ++j) { u[j] = 0.0; v[j] = 0.0; p[j] = 0; way[j] = 0; minv[j] = 0.0; }
    bool ok = true;
    for (int i = 1; i <= n && ok; ++i) {
        p[0] = i;
        int j0 = 0;
        unsigned used = 0;
        for (int j = 0; j <= m; ++j) { minv[j] = DBL_MAX; way[j] = 0; }
        bool found = false;
        for (int step = 0; step <= m; ++step) {               // each step marks one more column: m + 1 at the most
            used |= 1u << j0;
            const int i0 = p[j0];
            double delta = DBL_MAX;
            int j1 = -1;
            for (int j = 1; j <= m; ++j) {
                if ((used >> j) & 1u) continue;
                const int idx = tr ? rows[j - 1] * K + (i0 - 1) : rows[i0 - 1] * K + (j - 1);
                const double cur = (double)cost[idx] - u[i0] - v[j];
                if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                if (minv[j] < delta) { delta = minv[j]; j1 = j; }
            }
            if (j1 < 0) break;
            for (int j = 0; j <= m; ++j) {
                if ((used >> j) & 1u) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            }
            j0 = j1;
            if (p[j0] == 0) { found = true; break; }
        }
        if (!found) { ok = false; break; }
        for (int step = 0; step <= m && j0 != 0; ++step) {   // flip the path back to column 0
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        }
    }
    if (!ok) {
        for (int g = 0; g < G; ++g) assign[g] = -1;
        *total = NAN;
        return -1;
    }
    int matched = 0;
    for (int j = 1; j <= m; ++j) {
        if (p[j] == 0) continue;
        const int g = tr ? rows[j - 1] : rows[p[j] - 1];
        assign[g] = tr ? p[j] - 1 : j - 1;
        ++matched;
    }
    double sum = 0.0;
    for (int g = 0; g < G; ++g)
        if (assign[g] >= 0) sum += (double)cost[g * K + assign[g]];
    *total = (float)sum;
    return matched;
}
