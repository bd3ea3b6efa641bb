// Decomposition sheets (include/iodine_hip.h: iodine_render_sheet): image, reconstruction, segmentation and slot panels of a few scenes
// written as one uint8 HWC picture.  Stateless like launch_slot_table: no handle, no workspace, NCHW fp32 in, one launch.
//
// sheet_kernel: one block per (sheet row r, panel c, band of source rows).  A band is at most SHT_BAND source pixels, whole rows, which are
// contiguous in every plane.  Three steps, block-uniform in the panel kind:
//   1. seg / overlay only: the argmax label of every band pixel into LDS (one more row below the band when edges are drawn: that row is
//      read by two bands).  `v > best` from -inf: the lowest index wins a tie, a NaN never wins (slot_table_kernel's rule).
//   2. the colour of every SOURCE pixel of the band, packed r | g << 8 | b << 16, into LDS.  The K planes are read here and in step 1 only,
//      never per replicated output pixel.  L = 4: 16-byte loads (4-byte for gt), L = 1: element loads.
//   3. the output rows of the band with the padding the cell owns - left of and above the panel, right of / below it for the last panel /
//      row - so that the cells tile the sheet and every byte is written once.  W4: aligned 32-bit words, byte stores at the two ends of a
//      row's run (the neighbouring cell writes the other bytes of such a word itself); otherwise byte by byte.  A wave takes an output
//      row at a time, its lanes consecutive words / bytes.
// Arithmetic: every float operation is one IEEE operation rounded on its own (no contraction in this file), so float32 numpy gives the
// same bytes.  No atomics, no scratch: the same input gives the same bytes.  All sheet offsets fit 32 bits (the entry point refuses more).
#include "common.h"
#include "../../include/iodine_hip.h"

#pragma clang fp contract(off)

static constexpr int SHT_THREADS = 256;
static constexpr int SHT_BAND = 1024;                        // source pixels of a band (S <= 32: the whole panel)
static constexpr int SHT_MAX_SIZE = 1024;

struct sheet_inputs {
    const float* x;
    const float* pred;
    const float* mask;
    const float* mean;
    const unsigned char* gt;
    const unsigned char* slot_color;
    const unsigned char* gt_color;
};

// clamp to [0, 1] with a NaN going to 0, then round half up
IOD_DEVINL unsigned sht_quant(float v)
{
    v = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;
    return (unsigned)(int)__fadd_rn(__fmul_rn(v, 255.f), 0.5f);
}

IOD_DEVINL unsigned sht_pack(unsigned r, unsigned g, unsigned b) { return r | g << 8 | b << 16; }

// n / z for the replication factor z in 1..8 (block-uniform) and n >= 0: constant divisors instead of a run-time division per byte
IOD_DEVINL int sht_div(int n, int z)
{
    const unsigned u = (unsigned)n;
    switch (z) {
    case 1: return (int)u;
    case 2: return (int)(u >> 1);
    case 3: return (int)(u / 3u);
    case 4: return (int)(u >> 2);
    case 5: return (int)(u / 5u);
    case 6: return (int)(u / 6u);
    case 7: return (int)(u / 7u);
    default: return (int)(u >> 3);
    }
}

// rows per band and bands per panel for image size S (also used by the launcher)
static inline __host__ __device__ int sht_band_rows(int S) { const int nb = SHT_BAND / S; return nb < 1 ? 1 : (nb > S ? S : nb); }

template <int L, bool W4>
__global__ __launch_bounds__(SHT_THREADS)
void sheet_kernel(const iodine_sheet_spec sp, const sheet_inputs in, unsigned char* __restrict__ sheet, int W)
{
    __shared__ unsigned s_rgb[SHT_BAND];
    __shared__ unsigned char s_lab[SHT_BAND + SHT_MAX_SIZE];
    __shared__ float s_pal[51];                               // palette / 255, for the blends
    __shared__ unsigned s_pcol[17];                           // palette, packed

    const int tid = threadIdx.x;
    const int S = sp.size, K = sp.slots, G = sp.n_gt, z = sp.scale, pad = sp.pad, C = sp.n_panels, R = sp.rows;
    const int P = S * S;
    const int nb = sht_band_rows(S), nbands = (S + nb - 1) / nb;
    const int band = blockIdx.x % nbands, cell = blockIdx.x / nbands;
    const int c = cell % C, r = cell / C;
    const int y0 = band * nb, y1 = min(S, y0 + nb);
    const int kind = sp.panel_kind[c], slot = sp.panel_slot[c];
    const int p0 = y0 * S, n = (y1 - y0) * S;                 // the band's pixels: [p0, p0 + n) of every plane

    if (tid < 51) s_pal[tid] = __fdiv_rn((float)sp.palette[tid], 255.f);
    if (tid < 17) s_pcol[tid] = sht_pack(sp.palette[3 * tid], sp.palette[3 * tid + 1], sp.palette[3 * tid + 2]);

    const bool labels = kind == IODINE_SHEET_SEG || kind == IODINE_SHEET_OVERLAY;
    const bool edges = kind == IODINE_SHEET_OVERLAY && sp.draw_edges != 0;
    if (labels) {
        const int nl = n + ((edges && y1 < S) ? S : 0);
        const float* mb = in.mask + (size_t)r * K * P + p0;
        for (int v = tid; v < nl / L; v += SHT_THREADS) {
            float bv[L];
            int best[L];
#pragma unroll
            for (int j = 0; j < L; ++j) { bv[j] = -INFINITY; best[j] = 0; }
#pragma unroll 4
            for (int kk = 0; kk < K; ++kk) {
                float m[L];
                vec_load<L>(mb + (size_t)kk * P + v * L, m);
#pragma unroll
                for (int j = 0; j < L; ++j)
                    if (m[j] > bv[j]) { bv[j] = m[j]; best[j] = kk; }
            }
#pragma unroll
            for (int j = 0; j < L; ++j) s_lab[v * L + j] = (unsigned char)best[j];
        }
    }
    __syncthreads();

    const unsigned char* sc = in.slot_color ? in.slot_color + (size_t)r * K : nullptr;
    const unsigned char* gc = in.gt_color ? in.gt_color + (size_t)r * G : nullptr;
    const float oma = __fsub_rn(1.f, sp.alpha);
    for (int v = tid; v < n / L; v += SHT_THREADS) {
        const int q0 = v * L;                                 // band-local index of the group's first pixel
        unsigned out[L];
        switch (kind) {
        case IODINE_SHEET_IMAGE:
        case IODINE_SHEET_PRED:
        case IODINE_SHEET_SLOT_MEAN: {
            const float* src = kind == IODINE_SHEET_IMAGE ? in.x + (size_t)r * 3 * P
                             : kind == IODINE_SHEET_PRED ? in.pred + (size_t)r * 3 * P
                                                         : in.mean + ((size_t)r * K + slot) * 3 * P;
            float c0[L], c1[L], c2[L];
            vec_load<L>(src + p0 + q0, c0);
            vec_load<L>(src + (size_t)P + p0 + q0, c1);
            vec_load<L>(src + 2 * (size_t)P + p0 + q0, c2);
#pragma unroll
            for (int j = 0; j < L; ++j) out[j] = sht_pack(sht_quant(c0[j]), sht_quant(c1[j]), sht_quant(c2[j]));
            break;
        }
        case IODINE_SHEET_SEG: {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int lab = s_lab[q0 + j];
                const int ci = min(sc ? (int)sc[lab] : lab, 16);
                out[j] = s_pcol[ci];
            }
            break;
        }
        case IODINE_SHEET_OVERLAY: {
            const float* src = in.x + (size_t)r * 3 * P;
            float c0[L], c1[L], c2[L];
            vec_load<L>(src + p0 + q0, c0);
            vec_load<L>(src + (size_t)P + p0 + q0, c1);
            vec_load<L>(src + 2 * (size_t)P + p0 + q0, c2);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int q = q0 + j;
                const int lab = s_lab[q];
                bool edge = false;
                if (edges) {
                    const int lr = q / S, col = q - lr * S;
                    if (col + 1 < S && s_lab[q + 1] != lab) edge = true;
                    if (y0 + lr + 1 < S && s_lab[q + S] != lab) edge = true;
                }
                if (edge) {
                    out[j] = sht_pack(sp.edge[0], sp.edge[1], sp.edge[2]);
                } else {
                    const int ci = min(sc ? (int)sc[lab] : lab, 16);
                    const float a = sp.alpha;
                    out[j] = sht_pack(sht_quant(__fadd_rn(__fmul_rn(oma, c0[j]), __fmul_rn(a, s_pal[3 * ci]))),
                                      sht_quant(__fadd_rn(__fmul_rn(oma, c1[j]), __fmul_rn(a, s_pal[3 * ci + 1]))),
                                      sht_quant(__fadd_rn(__fmul_rn(oma, c2[j]), __fmul_rn(a, s_pal[3 * ci + 2]))));
                }
            }
            break;
        }
        case IODINE_SHEET_GT: {
            int first[L];
#pragma unroll
            for (int j = 0; j < L; ++j) first[j] = -1;
            const unsigned char* gb = in.gt + (size_t)r * G * P + p0 + q0;
            for (int g = G - 1; g >= 0; --g) {                // downwards: the lowest covering row is kept
                unsigned w;
                if constexpr (L == 4) w = *reinterpret_cast<const unsigned*>(gb + (size_t)g * P);
                else w = gb[(size_t)g * P];
#pragma unroll
                for (int j = 0; j < L; ++j)
                    if ((w >> (8 * j)) & 255u) first[j] = g;
            }
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int ci = first[j] < 0 ? 16 : min(gc ? (int)gc[first[j]] : first[j], 16);
                out[j] = s_pcol[ci];
            }
            break;
        }
        case IODINE_SHEET_ERROR: {
            const float* xs = in.x + (size_t)r * 3 * P + p0 + q0;
            const float* ps = in.pred + (size_t)r * 3 * P + p0 + q0;
            float a0[L], a1[L], a2[L], b0[L], b1[L], b2[L];
            vec_load<L>(xs, a0); vec_load<L>(xs + (size_t)P, a1); vec_load<L>(xs + 2 * (size_t)P, a2);
            vec_load<L>(ps, b0); vec_load<L>(ps + (size_t)P, b1); vec_load<L>(ps + 2 * (size_t)P, b2);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const float s = __fadd_rn(__fadd_rn(fabsf(__fsub_rn(a0[j], b0[j])), fabsf(__fsub_rn(a1[j], b1[j]))),
                                          fabsf(__fsub_rn(a2[j], b2[j])));
                const unsigned g = sht_quant(__fdiv_rn(__fmul_rn(sp.error_gain, s), 3.f));
                out[j] = sht_pack(g, g, g);
            }
            break;
        }
        case IODINE_SHEET_SLOT_MASKED: {
            const float* mu = in.mean + ((size_t)r * K + slot) * 3 * P + p0 + q0;
            float m[L], c0[L], c1[L], c2[L];
            vec_load<L>(in.mask + ((size_t)r * K + slot) * P + p0 + q0, m);
            vec_load<L>(mu, c0); vec_load<L>(mu + (size_t)P, c1); vec_load<L>(mu + 2 * (size_t)P, c2);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const float om = __fsub_rn(1.f, m[j]);
                out[j] = sht_pack(sht_quant(__fadd_rn(__fmul_rn(m[j], c0[j]), __fmul_rn(om, sp.background[0]))),
                                  sht_quant(__fadd_rn(__fmul_rn(m[j], c1[j]), __fmul_rn(om, sp.background[1]))),
                                  sht_quant(__fadd_rn(__fmul_rn(m[j], c2[j]), __fmul_rn(om, sp.background[2]))));
            }
            break;
        }
        default: {                                            // IODINE_SHEET_SLOT_MASK (the entry point refuses unknown kinds)
            float m[L];
            vec_load<L>(in.mask + ((size_t)r * K + slot) * P + p0 + q0, m);
#pragma unroll
            for (int j = 0; j < L; ++j) { const unsigned g = sht_quant(m[j]); out[j] = sht_pack(g, g, g); }
            break;
        }
        }
#pragma unroll
        for (int j = 0; j < L; ++j) s_rgb[q0 + j] = out[j];
    }
    __syncthreads();

    // the cell's rectangle of the sheet: columns [xb, xe), rows [ry0, ry1) of this band
    const int side = S * z, cw = side + pad;
    const int xb = c * cw, xe = xb + cw + (c == C - 1 ? pad : 0);
    const int px0 = xb + pad, py0 = r * cw + pad;             // the panel's origin
    const int ry0 = band == 0 ? r * cw : py0 + y0 * z;
    const int ry1 = py0 + y1 * z + ((band == nbands - 1 && r == R - 1) ? pad : 0);
    const int row_bytes = W * 3;
    const unsigned padv = sht_pack(sp.pad_value[0], sp.pad_value[1], sp.pad_value[2]);

    const int a = xb * 3, b = xe * 3;                         // the cell's bytes of a row: [a, b)
    const int wa = a & ~3;                                    // W4: row_bytes % 4 == 0, so a word aligned in one row is aligned in every row
    const int wave = tid >> 6, lane = tid & 63;
    // one wave per output row (no division by a run length), its lanes on consecutive words / bytes of the run
    for (int oy = ry0 + wave; oy < ry1; oy += SHT_THREADS / 64) {
        const int pr = oy - py0;                              // row inside the panel; outside [y0 z, y1 z) the row is padding
        const bool prow = pr >= y0 * z && pr < y1 * z;
        const unsigned* src = s_rgb + (prow ? (sht_div(pr, z) - y0) * S : 0);
        unsigned char* drow = sheet + oy * row_bytes;
        // byte `rel` of sheet row oy
        auto byte_at = [&](int rel) -> unsigned {
            const int px = rel / 3, ch = rel - 3 * px;
            unsigned v = padv;
            if (prow && px >= px0 && px < px0 + side) v = src[sht_div(px - px0, z)];
            return (v >> (8 * ch)) & 255u;
        };
        if constexpr (W4) {
            for (int rel = wa + 4 * lane; rel < b; rel += 4 * 64) {
                if (rel >= a && rel + 4 <= b) {
                    *reinterpret_cast<unsigned*>(drow + rel) = byte_at(rel) | byte_at(rel + 1) << 8 | byte_at(rel + 2) << 16 | byte_at(rel + 3) << 24;
                } else {                                      // a run's first or last word: the neighbouring cell owns the other bytes
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (rel + k >= a && rel + k < b) drow[rel + k] = (unsigned char)byte_at(rel + k);
                }
            }
        } else {
            for (int rel = a + lane; rel < b; rel += 64) drow[rel] = (unsigned char)byte_at(rel);
        }
    }
}

// bit 0: 16-byte loads, bit 1: word stores
int sheet_form(const iodine_sheet_spec& sp, const float* x, const float* pred, const float* mask, const float* mean,
               const unsigned char* gt, const unsigned char* sheet, int W)
{
    const uintptr_t f = (uintptr_t)x | (uintptr_t)pred | (uintptr_t)mask | (uintptr_t)mean;
    const bool lv = sp.size % 4 == 0 && (f & 15) == 0 && ((uintptr_t)gt & 3) == 0;
    const bool sv = W % 4 == 0 && ((uintptr_t)sheet & 3) == 0;
    return (lv ? 1 : 0) | (sv ? 2 : 0);
}

hipError_t launch_render_sheet(hipStream_t st, const iodine_sheet_spec& sp, const float* x, const float* pred, const float* mask,
                               const float* mean, const unsigned char* gt, const unsigned char* slot_color, const unsigned char* gt_color,
                               unsigned char* sheet, int W)
{
    const int S = sp.size, nb = sht_band_rows(S), nbands = (S + nb - 1) / nb;
    const unsigned grid = (unsigned)sp.rows * (unsigned)sp.n_panels * (unsigned)nbands;
    const sheet_inputs in = {x, pred, mask, mean, gt, slot_color, gt_color};
    const int form = sheet_form(sp, x, pred, mask, mean, gt, sheet, W);
    const dim3 g(grid), b(SHT_THREADS);
    switch (form) {
    case 3: hipLaunchKernelGGL((sheet_kernel<4, true>), g, b, 0, st, sp, in, sheet, W); break;
    case 1: hipLaunchKernelGGL((sheet_kernel<4, false>), g, b, 0, st, sp, in, sheet, W); break;
    case 2: hipLaunchKernelGGL((sheet_kernel<1, true>), g, b, 0, st, sp, in, sheet, W); break;
    default: hipLaunchKernelGGL((sheet_kernel<1, false>), g, b, 0, st, sp, in, sheet, W); break;
    }
    return hipGetLastError();
}
