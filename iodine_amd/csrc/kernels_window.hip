// Windowed batches (include/iodine_hip.h: iodine_batch_window; iodine_amd/windows.py).  Stateless like kernels_batch.hip: no handle, no
// workspace, one launch per call, nothing synchronises, no atomics.
//
// batch_window_kernel: item j of the batch is a window of store entry index[j] - frames kept at their native H x W - resampled to S x S:
// crop, triangle-filter resize with antialiasing (PIL's BILINEAR on the cut-out window), optional mirror, per-channel gain, clamp to
// [0, 1]; the mask word of the nearest source pixel, unpacked like batch_gather_kernel does.  tests/window_reference.py is the rule in
// fp64.  Per axis (bw_axis): scale = len / S, support = max(scale, 1), centre = o0 + (i + 0.5) scale, taps the whole pixels of
// [centre - support, centre + support) rounded like PIL does, clamped to the window rounded outward and to the frame; weights
// max(0, 1 - |r + 0.5 - centre| / support) normalised by their sum.  Coordinates, tap ranges and weights are fp64 with contraction off (a
// fused multiply-add moves a border tap), weights rounded to fp32 once; both passes accumulate in fp32.  scale <= 4: at most 9 taps.
//
// One block of 256 threads per (item, tile of output rows, chunk of <= 256 output columns; one chunk up to S = 256).  The first threads
// build the chunk's column table and the tile's row table in LDS (first tap, tap count, nearest pixel, <= 9 weights).  The block then
// stages the HORIZONTAL pass of the source rows the tile needs into LDS, [rows][columns][3] floats (48 KB: with the tables below 64 KB, two
// blocks per CU), does the vertical pass, gain and clamp from there and writes each channel plane with consecutive threads on consecutive x.
// A tile whose rows need more source rows than the stage holds (the launcher sizes the tile for scale <= 1.5; the stage always holds >= 16
// rows, a row needs <= 9) is done in several passes.  The horizontal pass is bound by load latency, not bytes: it takes its taps in threes
// with the loads of a three issued together, a uint8 value becomes a float through a 256-entry table of (float)u / 255.f in LDS (the IEEE
// division once per block), and the launcher halves the tile (down to 8 rows) while the grid has fewer than two blocks per CU.
//   DW = true:  uint8 frames with W % 4 == 0 and a 4-byte aligned store (launch_batch_window decides): every row starts on a dword and a
//               pixel's three bytes come out of the one or two aligned dwords that hold them;
//   DW = false: byte loads (and every float32 store: its taps are single floats).
// Every offset is a size_t.  THE INDICES AND WINDOWS ARE THE CALLER'S (windows.py validates both on the host before the launch); whatever a
// window holds, every tap is clamped into the frame and every tap count to 0..9, so nothing is read outside the store or the stage.
#include "common.h"

static constexpr int BW_THREADS = 256;
static constexpr int BW_TAPS = 9;
static constexpr int BW_COLS = 256;                         // output columns per block
static constexpr int BW_ROWS = 32;                          // output rows per block, at most
static constexpr int BW_STAGE = 4096;                       // staged pixels of three floats: 48 KB

struct BwTap { int first, count, nearest; float w[BW_TAPS]; };

// output pixel i of one axis: the window [o0, o0 + len) of an axis of n_src pixels resampled to S
IOD_DEVINL void bw_axis(double o0, double len, int n_src, int S, int i, BwTap* t)
{
#pragma clang fp contract(off)
    const double scale = len / (double)S;
    const double support = scale > 1.0 ? scale : 1.0;
    const double centre = o0 + ((double)i + 0.5) * scale;
    int lo = (int)(centre - support + 0.5), hi = (int)(centre + support + 0.5);
    int wlo = (int)floor(o0), whi = (int)ceil(o0 + len);
    wlo = wlo > 0 ? wlo : 0;
    whi = whi < n_src ? whi : n_src;
    lo = lo > wlo ? lo : wlo;
    hi = hi < whi ? hi : whi;
    lo = lo < n_src - 1 ? lo : n_src - 1;                    // (only a window outside the contract gets here with lo >= n_src)
    int n = len > 0.0 ? hi - lo : 0;
    n = n < 0 ? 0 : (n > BW_TAPS ? BW_TAPS : n);
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double w = 1.0 - fabs((double)(lo + k) + 0.5 - centre) / support;
        sum += w > 0.0 ? w : 0.0;
    }
    for (int k = 0; k < BW_TAPS; ++k) {                      // (zero beyond the taps: the passes read them in threes)
        const double w = 1.0 - fabs((double)(lo + k) + 0.5 - centre) / support;
        t->w[k] = k < n && sum > 0.0 ? (float)((w > 0.0 ? w : 0.0) / sum) : 0.f;
    }
    int near = (int)floor(centre);
    near = near > 0 ? near : 0;
    t->first = lo;
    t->count = n;
    t->nearest = near < n_src - 1 ? near : n_src - 1;
}

template <bool DW>
__global__ __launch_bounds__(BW_THREADS)
void batch_window_kernel(const long long* __restrict__ index, const void* __restrict__ images, int kind,
                         const unsigned short* __restrict__ masks, int H, int W, const float* __restrict__ windows, int S, int planes,
                         int tile_rows, float* __restrict__ x, unsigned char* __restrict__ gt)
{
    __shared__ BwTap s_col[BW_COLS];
    __shared__ BwTap s_row[BW_ROWS];
    __shared__ float s_stage[BW_STAGE * 3];
    __shared__ float s_lut[256];                            // u -> (float)u / 255.f: the IEEE division once per block, not per tap
    const size_t item = blockIdx.x;
    const int chunks = (S + BW_COLS - 1) / BW_COLS;
    const int tile = (int)blockIdx.y / chunks, chunk = (int)blockIdx.y - tile * chunks;
    const int j0 = chunk * BW_COLS, i0 = tile * tile_rows;
    const int nj = S - j0 < BW_COLS ? S - j0 : BW_COLS, ni = S - i0 < tile_rows ? S - i0 : tile_rows;
    const float* win = windows + item * 8;                  // y0, x0, h, w, flip, gain r g b
    const bool flip = win[4] != 0.f;
    const float gain[3] = {win[5], win[6], win[7]};

    s_lut[threadIdx.x] = (float)threadIdx.x / 255.f;        // (BW_THREADS == 256)
    for (int e = threadIdx.x; e < nj + ni; e += BW_THREADS) {
        if (e < nj) bw_axis((double)win[1], (double)win[3], W, S, j0 + e, &s_col[e]);
        else bw_axis((double)win[0], (double)win[2], H, S, i0 + e - nj, &s_row[e - nj]);
    }
    __syncthreads();

    const size_t src = (size_t)index[item];
    const size_t plane = (size_t)H * W;
    const unsigned char* u8 = static_cast<const unsigned char*>(images) + src * plane * 3;
    const float* f32 = static_cast<const float*>(images) + src * plane * 3;
    const int cap = BW_STAGE / nj;                           // source rows the stage holds: >= 16
    const size_t P = (size_t)S * S;

    for (int a = 0; a < ni;) {                               // output rows a .. b - 1 of the tile: their source rows fit the stage
        const int rlo = s_row[a].first;
        int b = a + 1;
        while (b < ni && s_row[b].first + s_row[b].count - rlo <= cap) ++b;
        const int nr = s_row[b - 1].first + s_row[b - 1].count - rlo;

        for (int e = threadIdx.x; e < nr * nj; e += BW_THREADS) {        // horizontal pass of source row rlo + rr, output column j0 + jj
            const int rr = e / nj, jj = e - rr * nj;
            const BwTap& c = s_col[jj];
            const size_t r = (size_t)(rlo + rr);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            // taps in threes, every load of a three issued before its first use; a tap beyond the count repeats the last one at weight 0
            if (kind == 0) {
                const unsigned char* row = u8 + r * W * 3;
                for (int k0 = 0; k0 < c.count; k0 += 3) {
                    uint32_t px[3];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const int o = 3 * (c.first + (k0 + u < c.count ? k0 + u : c.count - 1));
                        if constexpr (DW) {
                            const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row);   // r W 3 is a multiple of 4 where W is
                            const uint64_t two = ((uint64_t)r32[(o + 2) >> 2] << 32) | r32[o >> 2];   // (3 W - 1) >> 2 is inside the row
                            px[u] = (uint32_t)(two >> (8 * (o & 3)));
                        } else {
                            px[u] = (uint32_t)row[o] | ((uint32_t)row[o + 1] << 8) | ((uint32_t)row[o + 2] << 16);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const float w = c.w[k0 + u];
                        a0 += w * s_lut[px[u] & 255u]; a1 += w * s_lut[(px[u] >> 8) & 255u]; a2 += w * s_lut[(px[u] >> 16) & 255u];
                    }
                }
            } else {
                const float* row = f32 + r * W;
                for (int k0 = 0; k0 < c.count; k0 += 3) {
                    float v[3][3];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const int q = c.first + (k0 + u < c.count ? k0 + u : c.count - 1);
                        v[u][0] = row[q]; v[u][1] = row[plane + q]; v[u][2] = row[2 * plane + q];
                    }
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const float w = c.w[k0 + u];
                        a0 += w * v[u][0]; a1 += w * v[u][1]; a2 += w * v[u][2];
                    }
                }
            }
            float* s = s_stage + (size_t)e * 3;
            s[0] = a0; s[1] = a1; s[2] = a2;
        }
        __syncthreads();

        for (int e = threadIdx.x; e < (b - a) * nj; e += BW_THREADS) {    // vertical pass, gain, clamp; the mask word
            const int ii = e / nj, jj = e - ii * nj;
            const BwTap& t = s_row[a + ii];
            float acc[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < t.count; ++k) {
                const float* s = s_stage + ((size_t)(t.first + k - rlo) * nj + jj) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += t.w[k] * s[c];
            }
            const size_t io = (size_t)(i0 + a + ii), jo = (size_t)(flip ? S - 1 - (j0 + jj) : j0 + jj);
            float* xo = x + item * 3 * P + io * S + jo;
#pragma unroll
            for (int c = 0; c < 3; ++c) xo[(size_t)c * P] = fminf(fmaxf(gain[c] * acc[c], 0.f), 1.f);
            if (masks != nullptr && gt != nullptr) {
                const uint32_t m = masks[src * plane + (size_t)t.nearest * W + s_col[jj].nearest];
                unsigned char* go = gt + item * planes * P + io * S + jo;
                for (int g = 0; g < planes; ++g) go[(size_t)g * P] = (unsigned char)((m >> g) & 1u);
            }
        }
        __syncthreads();
        a = b;
    }
}

hipError_t launch_batch_window(hipStream_t st, const long long* index, int count, const void* images, int kind, const unsigned short* masks,
                               int H, int W, const float* windows, int S, int planes, float* x, unsigned char* gt)
{
    if (count < 1 || H < 1 || W < 1 || S < 1 || S > 512 || planes < 1 || planes > 16 || (kind != 0 && kind != 1)) return hipErrorInvalidValue;
    const int cols = S < BW_COLS ? S : BW_COLS;
    int tile_rows = BW_STAGE / cols / 2;                     // at scale <= 1.5 a tile's source rows fit the stage in one pass
    tile_rows = tile_rows < BW_ROWS ? tile_rows : BW_ROWS;
    tile_rows = tile_rows < S ? tile_rows : S;
    const int chunks = (S + BW_COLS - 1) / BW_COLS;
    // two blocks per CU hide each other's load latency: halve the tile while the grid is below that (8 rows re-read 3 of 15 at scale 1.5)
    while (tile_rows > 8 && (long long)count * chunks * ((S + tile_rows - 1) / tile_rows) < 512) tile_rows /= 2;
    const int tiles = (S + tile_rows - 1) / tile_rows;
    const dim3 grid((unsigned)count, (unsigned)(tiles * chunks));
    const bool dw = kind == 0 && W % 4 == 0 && ((uintptr_t)images & 3) == 0;
    if (dw)
        hipLaunchKernelGGL(batch_window_kernel<true>, grid, dim3(BW_THREADS), 0, st, index, images, kind, masks, H, W, windows, S, planes,
                           tile_rows, x, gt);
    else
        hipLaunchKernelGGL(batch_window_kernel<false>, grid, dim3(BW_THREADS), 0, st, index, images, kind, masks, H, W, windows, S, planes,
                           tile_rows, x, gt);
    return hipGetLastError();
}
