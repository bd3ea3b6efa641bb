// Connected components of segmentation maps (include/iodine_hip.h: iodine_seg_components).  Stateless like launch_slot_table: no handle,
// no allocation, no synchronise, every launch on the caller's stream; integers only, so the same input gives the same bits.
//
// The parent array.  par[p] is -1 for an invalid pixel (seg >= slots) and otherwise the index of a pixel of the same component with
// par[p] <= p; p is a root while par[p] == p.  Every write to it is the initial one (the first pixel of p's horizontal run within its
// wave's 64 pixels, which starts as a root), or an atomicMin with a smaller value, or the store of a root found from p: a parent only ever
// falls, and a root is the smallest pixel of the set it stands for.  When all unions are done the root of a component is therefore
// first(c), whatever the order the hardware ran them in.
//
// Termination, for ANY content of the array (so a wrong array costs a wrong answer, never a hang):
//   cc_find(x) steps to n = par[x] only while 0 <= n < x, so x falls strictly with every step: at most x steps.
//   cc_unite(a, b) finds both roots, returns when they are equal, and otherwise calls atomicMin(&par[hi], lo) with lo < hi.  It returns
//     unless the word held a value below hi (another thread had hung hi under a smaller pixel meanwhile), and then goes on with that
//     value in place of hi.  The larger of the two pixels it holds falls strictly with every retry: at most hi retries.
//   No kernel waits for another thread's write, no loop runs "until nothing changes", and every other loop is a counted one.
//
// Two forms of the union-find step, one kernel (cc_tile_kernel): a block owns a tile of an image, keeps the parent array of the tile in
// LDS, unites every pixel with its left / upper (8: and both upper diagonal) neighbours inside the tile - leaving out the unions that
// other pixels' unions imply (cc_need_up and its neighbours) - and writes each pixel's root to `labels` as a global pixel index.  Raster
// order inside a tile is raster order in the image, so the invariants above carry over.
//   LDS form, size <= CC_LDS_MAX_SIZE: the tile is the image (4 bytes of parent and 1 byte of label per pixel: 80 KiB at 128 x 128).
//   Global form: tiles of CC_TILE x CC_TILE, then cc_border_kernel unites across the tile borders in `labels` itself with the same
//   cc_unite on global memory.
// Both forms continue through the same kernels, on `labels` and the caller's scratch (area, id: int32 per pixel; best: 64 bits per pixel;
// one int32 per 1024 pixels):
//   cc_area_kernel    labels[p] = root, area[root] += 1 (one atomic per distinct root of a wave, the first of each wave folded per block)
//   cc_count_kernel   kept roots per chunk of 1024 pixels
//   cc_number_kernel  id of a kept root = kept roots in earlier chunks + earlier kept roots of its chunk: the prefix count over the roots
//                     in pixel order; per-component rows of count / per_slot / table
//   cc_vote_kernel    (clean only) every pixel of a small component offers its kept 4-neighbours: atomicMax of (area, ~first)
//   cc_output_kernel  labels, area_map, clean, the per-pixel sums and boxes of the table, the pixel counts
#include "../../include/iodine_hip.h"
#include "common.h"
#include <limits.h>

static constexpr int CC_THREADS = 1024;
static constexpr int CC_LDS_MAX_SIZE = 128;     // = IODINE_COMPONENTS_LDS_MAX_SIZE (include/iodine_hip.h)
static constexpr int CC_TILE = 64;
static constexpr int CC_CHUNK = 1024;           // pixels per block of the per-pixel kernels
static constexpr int CC_MAX_SLOTS = 16;
static_assert(CC_LDS_MAX_SIZE == IODINE_COMPONENTS_LDS_MAX_SIZE, "the header exports the LDS form's limit");

// the root above x: see the header comment for why this ends whatever par holds
IOD_DEVINL int cc_find(const int* par, int x)
{
    for (;;) {
        const int n = par[x];
        if (n < 0 || n >= x) return x;
        x = n;
    }
}

IOD_DEVINL void cc_unite(int* par, int a, int b)
{
    for (;;) {
        a = cc_find(par, a);
        b = cc_find(par, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(&par[hi], lo);
        if (old >= hi || old < 0) return;       // hi was a root and now hangs under lo
        a = old; b = lo;                        // old < hi: max(a, b) has fallen
    }
}

// Which of the unions of pixel p with its earlier neighbours are needed, given that every pixel makes its own: L / U / UL / UR say whether the
// left, upper, upper-left and upper-right neighbour exists and holds p's value.  Up is implied where left and upper-left both match (the
// left pixel makes the union with the upper-left one, which touches the upper one); a diagonal is implied where the upper pixel matches
// (it touches both diagonals), the upper-left one also where the left pixel matches (whose upper neighbour it is).  The border kernel asks
// the same questions across tiles: the implied unions are then made by the tile kernel or by another pixel of the border kernel.
IOD_DEVINL bool cc_need_up(bool L, bool U, bool UL) { return U && !(L && UL); }
IOD_DEVINL bool cc_need_up_left(bool L, bool U, bool UL) { return UL && !U && !L; }
IOD_DEVINL bool cc_need_up_right(bool U, bool UR) { return UR && !U; }

// unite local pixel l (value v) with its earlier neighbours inside a w-wide tile; `left`: false where the run start already stands in par
template <bool EIGHT>
IOD_DEVINL void cc_unite_back(int* par, const unsigned char* sg, int l, int lr, int lc, int w, unsigned char v, bool left)
{
    const bool L = lc > 0 && sg[l - 1] == v, U = lr > 0 && sg[l - w] == v;
    const bool UL = lr > 0 && lc > 0 && sg[l - w - 1] == v, UR = lr > 0 && lc + 1 < w && sg[l - w + 1] == v;
    if (left && L) cc_unite(par, l, l - 1);
    if (cc_need_up(L, U, UL)) cc_unite(par, l, l - w);
    if constexpr (EIGHT) {
        if (cc_need_up_left(L, U, UL)) cc_unite(par, l, l - w - 1);
        if (cc_need_up_right(U, UR)) cc_unite(par, l, l - w + 1);
    }
}

// grid (tiles_x * tiles_y, B); dynamic LDS = 5 bytes per pixel of the largest tile.  Also clears what the later kernels add into.
template <bool EIGHT>
__global__ __launch_bounds__(CC_THREADS)
void cc_tile_kernel(const unsigned char* __restrict__ seg, int slots, int S, int tile, int tiles_x, int* __restrict__ labels,
                    int* __restrict__ area, unsigned long long* __restrict__ best, int* __restrict__ count, int* __restrict__ per_slot,
                    int* __restrict__ table, int M)
{
    extern __shared__ __attribute__((aligned(16))) int s_par[];
    const int b = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, tid = threadIdx.x;
    const int x0 = tx * tile, y0 = ty * tile;
    const int w = min(tile, S - x0), h = min(tile, S - y0), n = w * h;
    unsigned char* s_seg = reinterpret_cast<unsigned char*>(s_par + n);
    const size_t img = (size_t)b * S * S;

    if (blockIdx.x == 0) {
        if (tid < 4) count[b * 4 + tid] = 0;
        if (per_slot) for (int i = tid; i < slots * 4; i += CC_THREADS) per_slot[(size_t)b * slots * 4 + i] = 0;
        if (table) for (int i = tid; i < M * 8; i += CC_THREADS) table[(size_t)b * M * 8 + i] = -1;
    }
    // The 64 lanes of a wave hold 64 consecutive pixels of the tile's raster: a pixel starts below the first pixel of its horizontal run
    // inside that stretch (a ballot of the run starts; lane 0 and column 0 always start one), so only lane 0 still has to look left.
    const int lane = tid & 63;
    for (int l = tid; l < n; l += CC_THREADS) {
        const int lr = l / w, lc = l - lr * w;
        const size_t g = img + (size_t)(y0 + lr) * S + x0 + lc;
        const unsigned char v = seg[g];
        const int left = __shfl_up((int)v, 1);
        const unsigned long long starts = __ballot(lane == 0 || lc == 0 || left != (int)v);
        const int start = 63 - __clzll((long long)(starts & ((2ull << lane) - 1ull)));      // bit 0 is set: start is in 0..lane
        s_seg[l] = v;
        s_par[l] = v < slots ? l - (lane - start) : -1;
        area[g] = 0;
        best[g] = 0ull;
    }
    __syncthreads();
    for (int l = tid; l < n; l += CC_THREADS) {
        const unsigned char v = s_seg[l];
        if (v >= slots) continue;
        const int lr = l / w, lc = l - lr * w;
        cc_unite_back<EIGHT>(s_par, s_seg, l, lr, lc, w, v, lane == 0);
    }
    __syncthreads();
    for (int l = tid; l < n; l += CC_THREADS) {
        const int lr = l / w, lc = l - lr * w;
        int root = -1;
        if (s_par[l] >= 0) {
            const int r = cc_find(s_par, l), rr = r / w;
            root = (y0 + rr) * S + x0 + (r - rr * w);
        }
        labels[img + (size_t)(y0 + lr) * S + x0 + lc] = root;
    }
}

// global form: unite every pixel with its earlier neighbours in ANOTHER tile.  grid (chunks, B)
template <bool EIGHT>
__global__ __launch_bounds__(CC_THREADS)
void cc_border_kernel(const unsigned char* __restrict__ seg, int slots, int S, int tile, int* __restrict__ labels)
{
    const int P = S * S, p = blockIdx.x * CC_CHUNK + threadIdx.x;
    if (p >= P) return;
    const unsigned char* sg = seg + (size_t)blockIdx.y * P;
    int* par = labels + (size_t)blockIdx.y * P;
    const unsigned char v = sg[p];
    if (v >= slots) return;
    const int row = p / S, col = p - row * S;
    const bool left = col > 0 && col % tile == 0, up = row > 0 && row % tile == 0;          // the neighbour lies in another tile
    if (!left && !up && !(EIGHT && row > 0 && col + 1 < S && (col + 1) % tile == 0)) return;
    const bool L = col > 0 && sg[p - 1] == v, U = row > 0 && sg[p - S] == v;
    const bool UL = row > 0 && col > 0 && sg[p - S - 1] == v, UR = row > 0 && col + 1 < S && sg[p - S + 1] == v;
    if (left && L && !(U && UL && !up)) cc_unite(par, p, p - 1);                             // (implied: the pixel above makes it)
    if (up && cc_need_up(L && !left, U, UL)) cc_unite(par, p, p - S);
    if constexpr (EIGHT) {
        if ((left || up) && cc_need_up_left(L, U, UL)) cc_unite(par, p, p - S - 1);
        if ((up || (col + 1) % tile == 0) && cc_need_up_right(U, UR)) cc_unite(par, p, p - S + 1);
    }
}

// labels[p] = root of p; area[root] = pixels.  A wave adds once per distinct root: the loop takes at least one lane out per turn.
__global__ __launch_bounds__(CC_THREADS)
void cc_area_kernel(int P, int* __restrict__ labels, int* __restrict__ area)
{
    const int p = blockIdx.x * CC_CHUNK + threadIdx.x;
    int* par = labels + (size_t)blockIdx.y * P;
    int* ar = area + (size_t)blockIdx.y * P;
    int root = -1;
    if (p < P && par[p] >= 0) {
        root = cc_find(par, p);
        par[p] = root;                          // a root again: other threads' finds through p stay right
    }
    // the first root of every wave waits in LDS: thread 0 adds runs of equal roots once (a block inside one region: one atomic)
    __shared__ int s_root[CC_THREADS / 64], s_n[CC_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_root[wv] = -1;
    bool todo = root >= 0;
    for (int turn = 0; turn < 64; ++turn) {
        const unsigned long long live = __ballot(todo);
        if (!live) break;
        const int lead = __shfl(root, __ffsll((long long)live) - 1);
        const unsigned long long same = __ballot(todo && root == lead);
        if (lane == 0) {
            if (turn == 0) { s_root[wv] = lead; s_n[wv] = __popcll(same); }
            else atomicAdd(&ar[lead], __popcll(same));
        }
        if (root == lead) todo = false;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int cur = -1, n = 0;
    for (int i = 0; i < CC_THREADS / 64; ++i) {
        if (s_root[i] < 0) continue;
        if (s_root[i] != cur) {
            if (cur >= 0) atomicAdd(&ar[cur], n);
            cur = s_root[i]; n = 0;
        }
        n += s_n[i];
    }
    if (cur >= 0) atomicAdd(&ar[cur], n);
}

IOD_DEVINL bool cc_kept_root(const int* par, const int* ar, int p, int P, int min_area)
{
    return p < P && par[p] == p && ar[p] >= min_area;
}

// chunk_kept[b][chunk] = kept roots among the chunk's pixels
__global__ __launch_bounds__(CC_THREADS)
void cc_count_kernel(int P, int min_area, const int* __restrict__ labels, const int* __restrict__ area, int* __restrict__ chunk_kept)
{
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int p = blockIdx.x * CC_CHUNK + threadIdx.x;
    const bool kept = cc_kept_root(labels + (size_t)blockIdx.y * P, area + (size_t)blockIdx.y * P, p, P, min_area);
    const unsigned long long m = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_n, __popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) chunk_kept[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s_n;
}

// ids of the kept roots, and everything that is one entry per component
__global__ __launch_bounds__(CC_THREADS)
void cc_number_kernel(const unsigned char* __restrict__ seg, int slots, int P, int min_area, int M, const int* __restrict__ labels,
                      const int* __restrict__ area, const int* __restrict__ chunk_kept, int* __restrict__ id, int* __restrict__ count,
                      int* __restrict__ per_slot, int* __restrict__ table)
{
    __shared__ int s_wave[CC_THREADS / 64];
    __shared__ int s_base, s_small;
    __shared__ int s_ps[CC_MAX_SLOTS][3];
    const int b = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * CC_CHUNK + tid;
    const int* par = labels + (size_t)b * P;
    const int* ar = area + (size_t)b * P;
    if (tid == 0) { s_base = 0; s_small = 0; }
    if (tid < CC_MAX_SLOTS * 3) (&s_ps[0][0])[tid] = 0;
    __syncthreads();
    // kept roots of the earlier chunks (at most 1024 of them)
    int before = 0;
    for (int c = tid; c < (int)blockIdx.x; c += CC_THREADS) before += chunk_kept[(size_t)b * gridDim.x + c];
    before = (int)wave_sum((unsigned)before);
    if ((tid & 63) == 0 && before) atomicAdd(&s_base, before);

    const bool root = p < P && par[p] == p;
    const int a = root ? ar[p] : 0;
    const bool kept = root && a >= min_area;
    const unsigned long long m = __ballot(kept);
    const int lane = tid & 63, wv = tid >> 6;
    const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int my = s_base + in_wave, block_kept = 0;
    for (int i = 0; i < CC_THREADS / 64; ++i) {
        const int c = s_wave[i];
        if (i < wv) my += c;
        block_kept += c;
    }
    if (root) {
        const int s = seg[(size_t)b * P + p];                 // < slots: p is valid
        if (kept) {
            id[(size_t)b * P + p] = my;
            if (table && my < M) {
                int* t = table + ((size_t)b * M + my) * 8;
                t[0] = s; t[1] = a; t[2] = 0; t[3] = 0; t[4] = INT_MAX; t[5] = INT_MAX; t[6] = -1; t[7] = -1;
            }
        } else {
            atomicAdd(&s_small, 1);
        }
        if (per_slot) {
            atomicAdd(&s_ps[s][kept ? 0 : 1], 1);
            atomicMax(&s_ps[s][2], a);
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (block_kept) atomicAdd(&count[b * 4 + 0], block_kept);
        if (s_small) atomicAdd(&count[b * 4 + 1], s_small);
    }
    if (per_slot && tid < slots * 3) {
        const int s = tid / 3, j = tid - s * 3, v = s_ps[s][j];
        int* dst = per_slot + ((size_t)b * slots + s) * 4 + j;
        if (v) { if (j == 2) atomicMax(dst, v); else atomicAdd(dst, v); }
    }
}

// a small component's candidates: the kept components holding a 4-neighbour of one of its pixels; the largest area, then the smaller first
__global__ __launch_bounds__(CC_THREADS)
void cc_vote_kernel(int S, int min_area, const int* __restrict__ labels, const int* __restrict__ area, unsigned long long* __restrict__ best)
{
    const int P = S * S, p = blockIdx.x * CC_CHUNK + threadIdx.x;
    if (p >= P) return;
    const int* par = labels + (size_t)blockIdx.y * P;
    const int* ar = area + (size_t)blockIdx.y * P;
    const int r = par[p];
    if (r < 0 || ar[r] >= min_area) return;
    const int row = p / S, col = p - row * S;
    unsigned long long key = 0ull;
    const int q[4] = {col > 0 ? p - 1 : -1, col + 1 < S ? p + 1 : -1, row > 0 ? p - S : -1, row + 1 < S ? p + S : -1};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (q[i] < 0) continue;
        const int d = par[q[i]];
        if (d < 0 || d == r) continue;
        const int ad = ar[d];
        if (ad < min_area) continue;
        const unsigned long long k = ((unsigned long long)(unsigned)ad << 32) | (unsigned)(INT_MAX - d);
        key = k > key ? k : key;
    }
    if (key) atomicMax(&best[(size_t)blockIdx.y * P + r], key);
}

// sums and box of some pixels of one kept component into its table row (cc_number_kernel wrote 0, 0, INT_MAX, INT_MAX, -1, -1 there)
IOD_DEVINL void cc_table_add(int* t, int sc, int sr, int xa, int ya, int xb, int yb)
{
    atomicAdd(&t[2], sc); atomicAdd(&t[3], sr);
    atomicMin(&t[4], xa); atomicMin(&t[5], ya); atomicMax(&t[6], xb); atomicMax(&t[7], yb);
}

__global__ __launch_bounds__(CC_THREADS)
void cc_output_kernel(const unsigned char* __restrict__ seg, int slots, int S, int min_area, int M, int* __restrict__ labels,
                      const int* __restrict__ area, const int* __restrict__ id, const unsigned long long* __restrict__ best,
                      int* __restrict__ area_map, int* __restrict__ count, int* __restrict__ per_slot, int* __restrict__ table,
                      unsigned char* __restrict__ clean)
{
    __shared__ int s_small_px[CC_MAX_SLOTS];
    __shared__ int s_invalid;
    __shared__ int s_row[CC_THREADS / 64], s_val[CC_THREADS / 64][6];
    const int P = S * S, b = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * CC_CHUNK + tid;
    const size_t img = (size_t)b * P;
    if (tid < CC_MAX_SLOTS) s_small_px[tid] = 0;
    if (tid == 0) s_invalid = 0;
    __syncthreads();
    int comp = -1, col = 0, row = 0;                         // id of a kept component below M: a table row
    if (p < P) {
        const unsigned char v = seg[img + p];
        const int r = labels[img + p];
        unsigned char out = v;
        int lab = -1, a = 0;
        if (r < 0 || v >= slots) {
            atomicAdd(&s_invalid, 1);
        } else {
            a = area[img + r];
            if (a >= min_area) {
                lab = id[img + r];
                if (table && lab < M) { comp = lab; row = p / S; col = p - row * S; }
            } else {
                atomicAdd(&s_small_px[v], 1);
                const unsigned long long k = clean ? best[img + r] : 0ull;
                if (k) {
                    const int d = INT_MAX - (int)(unsigned)(k & 0xffffffffull);
                    if (d >= 0 && d < P) out = seg[img + d];
                }
            }
        }
        labels[img + p] = lab;
        if (area_map) area_map[img + p] = a;
        if (clean) clean[img + p] = out;
    }
    if (table) {
        // a wave adds once per table row it touches (at most 64 turns: each takes a lane out); the first row of every wave waits in LDS,
        // where thread 0 folds runs of equal rows: a block inside one component adds once
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) s_row[wv] = -1;
        bool todo = comp >= 0;
        for (int turn = 0; turn < 64; ++turn) {
            const unsigned long long live = __ballot(todo);
            if (!live) break;
            const int lead = __shfl(comp, __ffsll((long long)live) - 1);
            const bool mine = todo && comp == lead;
            const int sc = (int)wave_sum((unsigned)(mine ? col : 0)), sr = (int)wave_sum((unsigned)(mine ? row : 0));
            const int xa = wave_min(mine ? col : INT_MAX), ya = wave_min(mine ? row : INT_MAX);
            const int xb = wave_max(mine ? col : -1), yb = wave_max(mine ? row : -1);
            if (lane == 0) {
                if (turn == 0) {
                    s_row[wv] = lead;
                    s_val[wv][0] = sc; s_val[wv][1] = sr; s_val[wv][2] = xa; s_val[wv][3] = ya; s_val[wv][4] = xb; s_val[wv][5] = yb;
                } else {
                    cc_table_add(table + ((size_t)b * M + lead) * 8, sc, sr, xa, ya, xb, yb);
                }
            }
            if (mine) todo = false;
        }
        __syncthreads();
        if (tid == 0) {
            int cur = -1, v[6] = {0, 0, INT_MAX, INT_MAX, -1, -1};
            for (int i = 0; i <= CC_THREADS / 64; ++i) {
                const int r = i < CC_THREADS / 64 ? s_row[i] : -2;                     // -2: flush the last run
                if (r == -1) continue;
                if (r != cur) {
                    if (cur >= 0) cc_table_add(table + ((size_t)b * M + cur) * 8, v[0], v[1], v[2], v[3], v[4], v[5]);
                    if (r < 0) break;
                    cur = r; v[0] = 0; v[1] = 0; v[2] = INT_MAX; v[3] = INT_MAX; v[4] = -1; v[5] = -1;
                }
                v[0] += s_val[i][0]; v[1] += s_val[i][1];
                v[2] = min(v[2], s_val[i][2]); v[3] = min(v[3], s_val[i][3]); v[4] = max(v[4], s_val[i][4]); v[5] = max(v[5], s_val[i][5]);
            }
        }
    }
    __syncthreads();
    if (tid < slots) {
        const int n = s_small_px[tid];
        if (n) {
            atomicAdd(&count[b * 4 + 2], n);
            if (per_slot) atomicAdd(&per_slot[((size_t)b * slots + tid) * 4 + 3], n);
        }
    }
    if (tid == 0 && s_invalid) atomicAdd(&count[b * 4 + 3], s_invalid);
}

// scratch layout, 8-byte aligned inside the caller's buffer: best (B P) u64, area (B P), id (B P), chunk_kept (B chunks) int32
size_t seg_components_scratch_bytes(int B, int S)
{
    const size_t P = (size_t)S * S, chunks = (P + CC_CHUNK - 1) / CC_CHUNK;
    return 8 + (size_t)B * (P * 16 + chunks * 4);
}

hipError_t launch_seg_components(hipStream_t st, const unsigned char* seg, int B, int slots, int S, int conn, int min_area, int M,
                                 int* labels, int* area_map, int* count, int* per_slot, int* table, unsigned char* clean, void* scratch)
{
    if (slots < 1 || slots > CC_MAX_SLOTS || S < 1 || S > 1024 || B < 1 || B > 65535) return hipErrorInvalidValue;
    const int P = S * S, chunks = (P + CC_CHUNK - 1) / CC_CHUNK;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(((uintptr_t)scratch + 7) & ~(uintptr_t)7);
    int* area = reinterpret_cast<int*>(best + (size_t)B * P);
    int* id = area + (size_t)B * P;
    int* chunk_kept = id + (size_t)B * P;
    const bool lds_form = S <= CC_LDS_MAX_SIZE;
    const int tile = lds_form ? S : CC_TILE, tiles = (S + tile - 1) / tile;
    const int lds = tile * tile * 5;
    const dim3 tgrid((unsigned)(tiles * tiles), (unsigned)B), pgrid((unsigned)chunks, (unsigned)B), block(CC_THREADS);
    const int max_lds = CC_LDS_MAX_SIZE * CC_LDS_MAX_SIZE * 5;
    hipError_t e;
    if (conn == 8) {
        e = iod_launch<cc_tile_kernel<true>>(st, tgrid, block, (size_t)lds, max_lds, seg, slots, S, tile, tiles, labels, area, best, count,
                                             per_slot, table, M);
        if (e == hipSuccess && !lds_form) e = iod_launch<cc_border_kernel<true>>(st, pgrid, block, 0, 0, seg, slots, S, tile, labels);
    } else {
        e = iod_launch<cc_tile_kernel<false>>(st, tgrid, block, (size_t)lds, max_lds, seg, slots, S, tile, tiles, labels, area, best, count,
                                              per_slot, table, M);
        if (e == hipSuccess && !lds_form) e = iod_launch<cc_border_kernel<false>>(st, pgrid, block, 0, 0, seg, slots, S, tile, labels);
    }
    if (e != hipSuccess) return e;
    if ((e = iod_launch<cc_area_kernel>(st, pgrid, block, 0, 0, P, labels, area)) != hipSuccess) return e;
    if ((e = iod_launch<cc_count_kernel>(st, pgrid, block, 0, 0, P, min_area, (const int*)labels, (const int*)area, chunk_kept)) != hipSuccess) return e;
    if ((e = iod_launch<cc_number_kernel>(st, pgrid, block, 0, 0, seg, slots, P, min_area, M, (const int*)labels, (const int*)area,
                                          (const int*)chunk_kept, id, count, per_slot, table)) != hipSuccess) return e;
    if (clean)
        if ((e = iod_launch<cc_vote_kernel>(st, pgrid, block, 0, 0, S, min_area, (const int*)labels, (const int*)area, best)) != hipSuccess) return e;
    return iod_launch<cc_output_kernel>(st, pgrid, block, 0, 0, seg, slots, S, min_area, M, labels, (const int*)area, (const int*)id,
                                        (const unsigned long long*)best, area_map, count, per_slot, table, clean);
}
