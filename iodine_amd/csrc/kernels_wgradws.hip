// Training-only kernel: the warp-specialised split-fp16 weight gradient of the stride-1 3x3 convs (producer waves
// stage and split the tiles, consumer waves run the MFMAs) and its launcher.
#include "common.h"
#include <vector>
#include <cstdio>

#ifdef IODINE_TILE_PROF
__device__ unsigned g_wgrad_prof[TP_MAXBLK * 8];            // [block][phase]: consumer wave 0 in 0-1, producer wave 4 in 2-7
#endif

// =========================================================================================
// Warp-specialised form of conv3x3_wgrad_f16x3_kernel (same arithmetic, same partial-tile output).
// The one-role kernel spends 42 % of a tile waiting for its global loads and 31 % splitting / transposing them into
// LDS; only 21 % is MFMA (tools/tile_phase_prof.md), and its 144 accumulator registers leave no room to prefetch.
// Here 512 threads = one block per CU:
//   waves 0-3  CONSUMERS  hold the 9 x 32x32 accumulators, read fragments from plane buffer (t & 1), 108 MFMAs per tile
//   waves 4-7  PRODUCERS  tile t+3 in flight (three register sets), tile t+1 split + transposed into buffer ((t+1) & 1),
//                         max |a|, max |d| of tile t+2 published for the scale choice of the next step
// One s_barrier per tile.  The tile loop is unrolled by three so that the register sets are named, not indexed.
// =========================================================================================
// The producers write the split tile in NATURAL order (per pixel: 64 hi channels | 64 lo channels, 8-byte
// stores, no rotation) and the consumers fetch K-major fragments with the gfx950 transposing LDS read
// ds_read_b64_tr_b16 (tools/experiments/tr_b16_probe.hip: in a 16-lane group lane i supplies row i/4, columns 4(i%4)..+3
// of a 4x16 halfword matrix, lane c receives column c): lane = channel, 4 consecutive pixels per read, the +-1 column
// taps are plain address offsets (no v_alignbit, no neighbour reads).  Pixel slots are padded to a stride of 64 mod 256
// bytes so that the 4 pixels x 64 bytes of one read fall into different bank quarters.
// (TR is a leftover template flag of the retired transposing-stager variant, always true.)
template <int CI, int NCO, bool TR>
__global__ __launch_bounds__(512, 2)
void conv3x3_wgrad_f16x3_ws_kernel(const float* __restrict__ a, const float* __restrict__ d, float* __restrict__ part,
                                   float* __restrict__ part_b, int S, int ntiles, int tiles_x, int tiles_y, float alpha, int accum)
{
    constexpr int MT = CI / 32, NTT = NCO / 32, KS = 4 / (MT * NTT);
    constexpr int TH = 4, HH = TH + 2;
    static_assert(TR, "only the natural-order staging + ds_read_b64_tr_b16 form is built");
    constexpr int A4 = CI / 4, D4 = NCO / 4;
    constexpr int NA_UNITS = HH * 10 * A4, ND_UNITS = TH * 8 * D4;
    constexpr int NAU = (NA_UNITS + 255) / 256, NDU = (ND_UNITS + 255) / 256;
    constexpr int RW = TH / KS;
    constexpr int AST = 2 * CI * 2 + 64, DST = 2 * NCO * 2 + 64;            // TR: bytes per pixel slot (hi | lo | pad)
    constexpr int A_BYTES = HH * 20 * AST, D_BYTES = TH * 16 * DST;
    static_assert(AST % 256 == 64 || AST % 256 == 192, "TR pixel stride must be an odd multiple of 64 bytes");
    constexpr int BUF_DW = (A_BYTES + D_BYTES) / 4;

    extern __shared__ __attribute__((aligned(16))) unsigned smem_ws[];
    float* s_max = reinterpret_cast<float*>(smem_ws + 2 * BUF_DW);          // [3][8]
    float* s_scale = s_max + 24;                                            // [2]: sa * sd of the tile in buffer b

    const int tid = threadIdx.x;
    const int lane = tid & 63, kh = lane >> 5, li = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Round 6: XCD-aware tile order (block b runs on XCD b % 8 - observed, speed only): every XCD walks one contiguous eighth of the tile
    // list and its blocks take neighbouring tiles at about the same time, so that the halo rows / columns two tiles share are L2 hits.  With
    // the plain order (tile = block + q * blocks) neighbouring tiles sat on different XCDs and every halo was fetched from memory again:
    // PMC at the cfg2 shapes 286 MB per launch against 210 MB of operands + partial tiles (profiles/r06_pmc_dsprites.json).  Needs a grid
    // that is a multiple of 8; the tile -> block map only changes WHICH partial tile a product lands in (fixed: results stay deterministic).
    // (xcd_span(.., xcd_order) of xcd_sched.h, spelled out: through the function the compiler orders these scalar instructions differently)
    const bool xcd_order = (gridDim.x & 7) == 0;
    const int bpx = xcd_order ? (int)(gridDim.x >> 3) : (int)gridDim.x;              // tile stride of a block
    const int per_xcd = (ntiles + 7) >> 3;
    const int t_begin = xcd_order ? (int)(blockIdx.x & 7) * per_xcd : 0;
    const int t_end = xcd_order ? min(ntiles, t_begin + per_xcd) : ntiles;
    const int t_first = t_begin + (xcd_order ? (int)(blockIdx.x >> 3) : (int)blockIdx.x);
    const int my_tiles = t_first < t_end ? (t_end - 1 - t_first) / bpx + 1 : 0;
    const int nq = my_tiles;

    if (wv >= 4) {
        // ------------------------------------------------------------------ PRODUCERS ----
        const int ptid = tid - 256, pw = wv - 4;
        float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
        float sa = 1.f, sd = 1.f;
        struct Set { f32x4 ra[NAU][2]; f32x4 rd[NDU][2]; };     // native vectors: they are inline-asm operands
#define VM_WAIT(n) do { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(n) : "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
        // the wait names every register of the set as read-write, so no use of the loaded values can be placed above it
        auto wait_set = [&](auto nc, Set& r) {
            constexpr int n = decltype(nc)::value;
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(n) : "memory");
#pragma unroll
            for (int k = 0; k < NAU; ++k) { asm volatile("" : "+v"(r.ra[k][0])); asm volatile("" : "+v"(r.ra[k][1])); }
#pragma unroll
            for (int k = 0; k < NDU; ++k) { asm volatile("" : "+v"(r.rd[k][0])); asm volatile("" : "+v"(r.rd[k][1])); }
            __builtin_amdgcn_sched_barrier(0);
        };
        using std::integral_constant;
        // Tile loads are raw BUFFER loads: one descriptor per (tensor, slot-image) with num_records = one image, so rows
        // above / below the image are out of range and return 0 in hardware; only the two halo columns left / right of
        // the image need an explicit invalid offset.  Per load: one v_add (tile offset + the thread's constant unit
        // offset) and, for the edge columns, one v_cndmask - instead of ~15 VALU of 64-bit address arithmetic each.
        // (a lambda of its own, not iod_make_rsrc: through the helper hipcc swaps two scalar moves of this kernel)
        auto make_rsrc = [&](const float* base, unsigned bytes) {
            const unsigned long long p = (unsigned long long)base;
            i32x4 r;
            r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)p);
            r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32));          // stride 0, no swizzle
            r.z = __builtin_amdgcn_readfirstlane((int)bytes);
            r.w = 0x00020000;                                                         // raw dword buffer (gfx9 / CDNA)
            return r;
        };
#define BLOAD4(dst, voff, rsrc, imm) \
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(dst) : "v"(voff), "s"(rsrc), "n"(imm) : "memory")
        unsigned aoff[NAU], doff[NDU];                     // the thread's constant byte offsets inside a tile (pixel j = 0)
        bool a_left[NAU], a_right[NAU];
#pragma unroll
        for (int k = 0; k < NAU; ++k) {
            const int u = ptid + k * 256;
            const int c4 = u % A4, tt = u / A4, p = tt % 10, row = tt / 10;
            aoff[k] = u < NA_UNITS ? (unsigned)(((row * S + 2 * p) * CI + c4 * 4) * 4) : 0x80000000u;
            a_left[k] = p == 0; a_right[k] = p == 9;
        }
#pragma unroll
        for (int k = 0; k < NDU; ++k) {
            const int u = ptid + k * 256;
            const int c4 = u % D4, tt = u / D4, p = tt % 8, row = tt / 8;
            doff[k] = u < ND_UNITS ? (unsigned)(((row * S + 2 * p) * NCO + c4 * 4) * 4) : 0x80000000u;
        }
        // tile coordinates of the load stream advance by gridDim.x per step: carried additions instead of two integer
        // divisions per tile (those were ~1 k ticks of a 6 k-tick step)
        int ltx, lty, ln, lq = 0;
        {
            int t = min(t_first, ntiles - 1);                   // (a block without tiles still issues its first loads: keep them inside the tensor)
            ltx = t % tiles_x; t /= tiles_x;
            lty = t % tiles_y; ln = t / tiles_y;
        }
        int gsx, gsy, gsn;
        {
            int t = bpx;
            gsx = t % tiles_x; t /= tiles_x;
            gsy = t % tiles_y; gsn = t / tiles_y;
        }
        auto G = [&](int, Set& r) {                                         // called for steps 0, 1, 2, ... in order
            const int tx = ltx, ty = lty, n = ln;
            if (lq + 1 < nq) {                                              // steps past the end re-read the last tile
                ltx += gsx;
                const int cx = ltx >= tiles_x ? 1 : 0;
                ltx -= cx ? tiles_x : 0;
                lty += gsy + cx;
                const int cy = lty >= tiles_y ? 1 : 0;
                lty -= cy ? tiles_y : 0;
                ln += gsn + cy;
            }
            ++lq;
            const i32x4 ra_rsrc = make_rsrc(a + (size_t)n * S * S * CI, (unsigned)(S * S * CI * 4));
            const i32x4 rd_rsrc = make_rsrc(d + (size_t)n * S * S * NCO, (unsigned)(S * S * NCO * 4));
            // first halo pixel of the tile is (ty*TH - 1, tx*16 - 2); negative offsets wrap above num_records -> 0
            const unsigned a_tile = (unsigned)(((ty * TH - 1) * S + tx * 16 - 2) * CI * 4);
            const unsigned d_tile = (unsigned)(((ty * TH) * S + tx * 16) * NCO * 4);
            const bool at_left = tx == 0, at_right = tx == tiles_x - 1;     // block-uniform
            // SGPRs written by the SALU need 5 wait states before a VMEM instruction reads them; hipcc's hazard recognizer
            // does not look inside inline asm
            asm volatile("s_nop 4" :: "s"(ra_rsrc), "s"(rd_rsrc) : "memory");
#pragma unroll
            for (int k = 0; k < NAU; ++k) {
                const bool bad = (a_left[k] && at_left) || (a_right[k] && at_right);
                const unsigned vo = bad ? 0x80000000u : aoff[k] + a_tile;   // both pixels of an edge unit are outside
                BLOAD4(r.ra[k][0], vo, ra_rsrc, 0);
                BLOAD4(r.ra[k][1], vo, ra_rsrc, CI * 4);
            }
#pragma unroll
            for (int k = 0; k < NDU; ++k) {
                const unsigned vo = doff[k] + d_tile;
                BLOAD4(r.rd[k][0], vo, rd_rsrc, 0);
                BLOAD4(r.rd[k][1], vo, rd_rsrc, NCO * 4);
            }
        };
        // The loads are inline asm, so hipcc does not count them: its own vmcnt bookkeeping would drain vmcnt(0) at the
        // loop header (every third tile) and expose the latency the three register sets are there to hide.  Loads return
        // in order; a set is (2 NAU + 2 NDU) loads, so "at most n younger sets outstanding" = vmcnt(n * SET_LOADS).
        constexpr int SET_LOADS = 2 * NAU + 2 * NDU;
        auto MAXPUB = [&](int q, int slot, const Set& r) {
            float ma = 0.f, md = 0.f;
#pragma unroll
            for (int k = 0; k < NAU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    ma = fmaxf(ma, fmaxf(fmaxf(fabsf(r.ra[k][j].x), fabsf(r.ra[k][j].y)), fmaxf(fabsf(r.ra[k][j].z), fabsf(r.ra[k][j].w))));
            const bool real = q < nq;                                       // block-uniform: the bias sums count each tile once
#pragma unroll
            for (int k = 0; k < NDU; ++k)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    md = fmaxf(md, fmaxf(fmaxf(fabsf(r.rd[k][j].x), fabsf(r.rd[k][j].y)), fmaxf(fabsf(r.rd[k][j].z), fabsf(r.rd[k][j].w))));
                    if (real) { bsum.x += r.rd[k][j].x; bsum.y += r.rd[k][j].y; bsum.z += r.rd[k][j].z; bsum.w += r.rd[k][j].w; }
                }
            ma = wave_max_f32(ma);
            md = wave_max_f32(md);
            if (lane == 0) { s_max[slot * 8 + pw] = ma; s_max[slot * 8 + 4 + pw] = md; }
        };
        auto WIN = [&](int q, int slot, const Set& r) {
            const float* m = s_max + slot * 8;
            const float ma = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])), md = fmaxf(fmaxf(m[4], m[5]), fmaxf(m[6], m[7]));
            sa = tile_scale(ma, sa);
            sd = tile_scale(md, sd);
            if (ptid == 0) s_scale[q & 1] = sa * sd;
            if constexpr (TR) {
                unsigned char* sb = reinterpret_cast<unsigned char*>(smem_ws + (q & 1) * BUF_DW);
                auto split_store = [&](const f32x4 w, float scale, unsigned char* dst, int lo_off) {
                    const float x = w.x * scale, y = w.y * scale, z = w.z * scale, t = w.w * scale;
                    typedef __fp16 h2_ __attribute__((ext_vector_type(2)));
                    const h2_ h01 = __builtin_amdgcn_cvt_pkrtz(x, y), h23 = __builtin_amdgcn_cvt_pkrtz(z, t);      // (rounding toward zero = the 11 leading bits)
                    const h2_ l01 = __builtin_amdgcn_cvt_pkrtz(x - (float)h01.x, y - (float)h01.y), l23 = __builtin_amdgcn_cvt_pkrtz(z - (float)h23.x, t - (float)h23.y);   // v_fma_mix_f32
                    uint2 hi, lo;
                    __builtin_memcpy(&hi.x, &h01, 4); __builtin_memcpy(&hi.y, &h23, 4);
                    __builtin_memcpy(&lo.x, &l01, 4); __builtin_memcpy(&lo.y, &l23, 4);
                    *reinterpret_cast<uint2*>(dst) = hi;
                    *reinterpret_cast<uint2*>(dst + lo_off) = lo;
                };
#pragma unroll
                for (int k = 0; k < NAU; ++k) {
                    const int u = ptid + k * 256;
                    if (u < NA_UNITS) {
                        const int c4 = u % A4, tt = u / A4, p = tt % 10, row = tt / 10;
                        unsigned char* dst = sb + (row * 20 + 2 * p) * AST + c4 * 8;
                        split_store(r.ra[k][0], sa, dst, CI * 2);
                        split_store(r.ra[k][1], sa, dst + AST, CI * 2);
                    }
                }
#pragma unroll
                for (int k = 0; k < NDU; ++k) {
                    const int u = ptid + k * 256;
                    if (u < ND_UNITS) {
                        const int c4 = u % D4, tt = u / D4, p = tt % 8, row = tt / 8;
                        unsigned char* dst = sb + A_BYTES + (row * 16 + 2 * p) * DST + c4 * 8;
                        split_store(r.rd[k][0], sd, dst, NCO * 2);
                        split_store(r.rd[k][1], sd, dst + DST, NCO * 2);
                    }
                }
                return;
            }
        };
        Set R0, R1, R2;
        TP_DECL;
        G(0, R0); G(1, R1); G(2, R2);
        wait_set(integral_constant<int, 2 * SET_LOADS>{}, R0);
        MAXPUB(0, 0, R0);
        __builtin_amdgcn_s_waitcnt(0xc07f);                                 // lgkmcnt(0): own LDS writes retired
        __builtin_amdgcn_s_barrier();                                       // P1: max(0) visible
        WIN(0, 0, R0);
        wait_set(integral_constant<int, SET_LOADS>{}, R1);
        MAXPUB(1, 1, R1);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();                                       // P2: tile 0 staged, max(1) visible
        // iteration q: request tile q+3, stage tile q+1, publish max(q+2)
        auto iteration = [&](int q, int sl, Set& Rnext, Set& Rmax, Set& Rload) {
            TP_STAMP(7);
            G(q + 3, Rload);
            TP_STAMP(2);                                                    // [2] producer: issue of the tile loads
            wait_set(integral_constant<int, 2 * SET_LOADS>{}, Rnext);        // (tile q+1 arrived during the previous step)
            WIN(q + 1, (sl + 1) % 3, Rnext);
            TP_STAMP(3);                                                    // [3] producer: split + transposed LDS writes
            wait_set(integral_constant<int, SET_LOADS>{}, Rmax);             // tile q+2: requested two steps ago
            MAXPUB(q + 2, (sl + 2) % 3, Rmax);
            __builtin_amdgcn_s_waitcnt(0xc07f);
            TP_STAMP(4);                                                    // [4] producer: wait for tile q+2, max
            __builtin_amdgcn_s_barrier();
            TP_STAMP(5);                                                    // [5] producer: barrier wait
        };
        for (int q = 0; q < nq; q += 3) {
            iteration(q, 0, R1, R2, R0);
            if (q + 1 < nq) iteration(q + 1, 1, R2, R0, R1);
            if (q + 2 < nq) iteration(q + 2, 2, R0, R1, R2);
        }
#ifdef IODINE_TILE_PROF
        if (ptid == 0 && blockIdx.x < TP_MAXBLK) for (int i_ = 2; i_ < 8; ++i_) g_wgrad_prof[blockIdx.x * 8 + i_] = tp_acc[i_];
#endif
        VM_WAIT(0);
#undef VM_WAIT
#undef BLOAD4
        __builtin_amdgcn_s_barrier();                                       // F1: consumers are done with the planes
        reinterpret_cast<float4*>(smem_ws)[ptid] = bsum;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();                                       // F2
        return;
    }

    // ---------------------------------------------------------------------- CONSUMERS ----
    const int mi = wv % MT, ni = (wv / MT) % NTT, ks = wv / (MT * NTT);
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float acc_prod = 1.f;
    __builtin_amdgcn_s_barrier();                                           // P1
    __builtin_amdgcn_s_barrier();                                           // P2
    TP_DECL;
    for (int q = 0; q < nq; ++q) {
        const float prod = s_scale[q & 1];
        if (prod != acc_prod) {                                             // block-uniform; exact (powers of two)
            const float r = prod / acc_prod;
#pragma unroll
            for (int tp = 0; tp < 9; ++tp)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[tp][e] *= r;
            acc_prod = prod;
        }
        if constexpr (TR) {
            // lane -> (16-lane group g: K half kh = g >> 1, channel half g & 1; i = lane & 15: pixel i >> 2, channel quad i & 3)
            typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
            const int g = lane >> 4, i16 = lane & 15;
            const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)smem_ws + (q & 1) * BUF_DW * 4;
            const int row0 = RW == 1 ? ks : 0;                          // RW == 1: this wave's single row through the base address
            const unsigned a_addr = lds0 + (row0 * 20 + 8 * (g >> 1) + (i16 >> 2)) * AST + (mi * 32 + 16 * (g & 1) + 4 * (i16 & 3)) * 2;
            const unsigned d_addr = lds0 + A_BYTES + (row0 * 16 + 8 * (g >> 1) + (i16 >> 2)) * DST + (ni * 32 + 16 * (g & 1) + 4 * (i16 & 3)) * 2;
            struct FragA { u32x2_ v[2][3][2]; };                         // [term][dx][pixel half]
            struct FragB { u32x2_ v[2][2]; };                            // [term][pixel half]
#define IOD_TRR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
            auto loadA = [&, a_addr](auto rc, auto dyc, FragA& f) {
                constexpr int rrow = decltype(rc)::value + decltype(dyc)::value;
                const unsigned aa = a_addr;
#pragma unroll
                for (int term = 0; term < 2; ++term)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            // (constant-folded after unrolling: the offset must be an immediate)
                            switch (term * 6 + dx * 2 + h) {
#define IOD_CASE(T_, DX_, H_) case T_ * 6 + DX_ * 2 + H_: IOD_TRR(f.v[T_][DX_][H_], aa, (rrow * 20 + DX_ + 1 + 4 * H_) * AST + T_ * CI * 2); break;
                                IOD_CASE(0, 0, 0) IOD_CASE(0, 0, 1) IOD_CASE(0, 1, 0) IOD_CASE(0, 1, 1) IOD_CASE(0, 2, 0) IOD_CASE(0, 2, 1)
                                IOD_CASE(1, 0, 0) IOD_CASE(1, 0, 1) IOD_CASE(1, 1, 0) IOD_CASE(1, 1, 1) IOD_CASE(1, 2, 0) IOD_CASE(1, 2, 1)
#undef IOD_CASE
                            }
                        }
            };
            auto loadB = [&, d_addr](auto rc, FragB& f) {
                constexpr int rrow = decltype(rc)::value;
                const unsigned da = d_addr;
                IOD_TRR(f.v[0][0], da, (rrow * 16) * DST);
                IOD_TRR(f.v[0][1], da, (rrow * 16 + 4) * DST);
                IOD_TRR(f.v[1][0], da, (rrow * 16) * DST + NCO * 2);
                IOD_TRR(f.v[1][1], da, (rrow * 16 + 4) * DST + NCO * 2);
            };
#undef IOD_TRR
            auto mma = [&](auto dyc, FragA& fa, FragB& fb) {
                constexpr int dy = decltype(dyc)::value;
                f16x8 B[2], A[2][3];
#pragma unroll
                for (int term = 0; term < 2; ++term) {
                    const uint4 vb = make_uint4(fb.v[term][0].x, fb.v[term][0].y, fb.v[term][1].x, fb.v[term][1].y);
                    __builtin_memcpy(&B[term], &vb, 16);
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const uint4 va = make_uint4(fa.v[term][dx][0].x, fa.v[term][dx][0].y, fa.v[term][dx][1].x, fa.v[term][dx][1].y);
                        __builtin_memcpy(&A[term][dx], &va, 16);
                    }
                }
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int tap = dy * 3 + dx;
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[1][dx], B[0], acc[tap], 0, 0, 0);
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0][dx], B[1], acc[tap], 0, 0, 0);
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0][dx], B[0], acc[tap], 0, 0, 0);
                }
            };
            using std::integral_constant;
            // fragments are double-buffered: the reads of step s+1 are issued before the MFMAs of step s; LDS returns in
            // order, so waiting until only the newer step's reads are outstanding retires the older step's
            FragA fa0, fa1;
            FragB fb0, fb1;
            auto wait_frags = [&](auto nc, FragA& fa, FragB& fb) {
                constexpr int nleft = decltype(nc)::value;
                asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(nleft) : "memory");
#pragma unroll
                for (int term = 0; term < 2; ++term) {
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) { asm volatile("" : "+v"(fa.v[term][dx][0])); asm volatile("" : "+v"(fa.v[term][dx][1])); }
                    asm volatile("" : "+v"(fb.v[term][0])); asm volatile("" : "+v"(fb.v[term][1]));
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            // rows of this wave: RW == 4: rows 0..3 (compile-time offsets); RW == 1: row ks through the base addresses
            static_assert(RW == 4 || RW == 1, "rows per consumer wave");
            // step list (row, dy): even steps use (fa0), odd steps (fa1); B fragments alternate per row
            auto run = [&]() {
                constexpr int NROW = RW;
                loadB(integral_constant<int, 0>{}, fb0);
                loadA(integral_constant<int, 0>{}, integral_constant<int, 0>{}, fa0);
                static_for<NROW>([&](auto rc) {
                    constexpr int r = decltype(rc)::value;
                    FragB& fbc = (r & 1) ? fb1 : fb0;
                    FragB& fbn = (r & 1) ? fb0 : fb1;
                    // dy = 0 (fa of parity (3r) & 1)
                    auto& f_0 = ((3 * r) & 1) ? fa1 : fa0;
                    auto& f_1 = ((3 * r + 1) & 1) ? fa1 : fa0;
                    auto& f_2 = ((3 * r + 2) & 1) ? fa1 : fa0;
                    loadA(rc, integral_constant<int, 1>{}, f_1);
                    wait_frags(integral_constant<int, 12>{}, f_0, fbc);
                    mma(integral_constant<int, 0>{}, f_0, fbc);
                    loadA(rc, integral_constant<int, 2>{}, f_2);
                    wait_frags(integral_constant<int, 12>{}, f_1, fbc);
                    mma(integral_constant<int, 1>{}, f_1, fbc);
                    if constexpr (r + 1 < NROW) {
                        loadB(integral_constant<int, (r + 1 < NROW ? r + 1 : 0)>{}, fbn);
                        loadA(integral_constant<int, (r + 1 < NROW ? r + 1 : 0)>{}, integral_constant<int, 0>{}, f_1);   // step 3r+3 has the parity of 3r+1
                        wait_frags(integral_constant<int, 15>{}, f_2, fbc);   // (16 newer reads; lgkmcnt is a 4-bit counter)
                    } else {
                        wait_frags(integral_constant<int, 0>{}, f_2, fbc);
                    }
                    mma(integral_constant<int, 2>{}, f_2, fbc);
                });
            };
            run();
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        TP_STAMP(0);                                                        // [0] consumer: fragment reads + MFMAs of a tile
        __builtin_amdgcn_s_barrier();
        TP_STAMP(1);                                                        // [1] consumer: barrier wait
    }
#ifdef IODINE_TILE_PROF
    if (tid == 0 && blockIdx.x < TP_MAXBLK) for (int i_ = 0; i_ < 2; ++i_) g_wgrad_prof[blockIdx.x * 8 + i_] = tp_acc[i_];
#endif
    constexpr int NCOP = NTT * 32;
    // Round 5: the partial tile of THIS block can be kept across the T + 1 decoder passes of a training step (accum: add alpha x this
    // launch to what the block left there in the previous pass; alpha = the pass's loss weight -w_i / B), so that the fixed-order
    // reduction over the blocks runs once per layer and step instead of once per launch (18 -> 3 reduce launches per cfg3 step).
    const float inv = alpha / acc_prod;
    if constexpr (KS > 1) {
        // Round 6 (C = 32: the four consumer waves each own one ROW of the tile and a full set of the nine 32 x 32 tap accumulators): the four
        // K-split accumulator sets are summed through LDS - fixed order wave 0 .. 3 - before ONE partial tile per block is written, instead of
        // four (37.7 -> 9.4 MB of partial tiles per cfg2 launch, and the fixed-order reduction behind it reads a quarter).  Three rounds of three
        // taps (4 waves x 3 x 16 x 64 floats = 48 KB per round, behind the 4 KB the producers' bias sums use); the producer waves have left after F2,
        // terminated waves do not take part in s_barrier.
        __builtin_amdgcn_s_barrier();                                       // F1
        __builtin_amdgcn_s_barrier();                                       // F2: producers' bias sums are in LDS
        if (tid < D4) {
            const float4* s_red = reinterpret_cast<const float4*>(smem_ws);
            float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = tid; j < 256; j += D4) { const float4 v = s_red[j]; t4.x += v.x; t4.y += v.y; t4.z += v.z; t4.w += v.w; }
            float4* pb = reinterpret_cast<float4*>(part_b + (size_t)blockIdx.x * NCO + tid * 4);
            float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (accum) o4 = *pb;
            *pb = make_float4(o4.x + alpha * t4.x, o4.y + alpha * t4.y, o4.z + alpha * t4.z, o4.w + alpha * t4.w);
        }
        static_assert(KS == 4 && MT == 1 && NTT == 1, "K-split reduction is written for the 32 x 32 instance");
        float* s_sum = reinterpret_cast<float*>(smem_ws) + 1024;            // [wave][3 taps x 16 regs][64 lanes]
        float* pwb = part + ((size_t)blockIdx.x * 9) * CI * NCOP;
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) {
#pragma unroll
            for (int tl = 0; tl < 3; ++tl)
#pragma unroll
                for (int r = 0; r < 16; ++r) s_sum[(ks * 48 + tl * 16 + r) * 64 + lane] = nq > 0 ? acc[rd * 3 + tl][r] * inv : 0.f;
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int ent = ks * 12 + e, tl = ent >> 4, r = ent & 15;
                const float v = ((s_sum[(0 * 48 + ent) * 64 + lane] + s_sum[(1 * 48 + ent) * 64 + lane]) + s_sum[(2 * 48 + ent) * 64 + lane]) + s_sum[(3 * 48 + ent) * 64 + lane];
                const int cr = (r & 3) + 8 * (r >> 2) + 4 * kh;
                float* dst = pwb + ((size_t)(rd * 3 + tl) * CI + cr) * NCOP + li;
                *dst = accum ? *dst + v : v;
            }
            __builtin_amdgcn_s_barrier();
        }
        return;
    }
    float* pw = part + ((size_t)(blockIdx.x * KS + ks) * 9) * CI * NCOP;
    if (accum) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            float old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) old[r] = pw[((size_t)tap * CI + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * NCOP + ni * 32 + li];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                pw[((size_t)tap * CI + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * NCOP + ni * 32 + li] = old[r] + (nq > 0 ? acc[tap][r] * inv : 0.f);
        }
    } else {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cr = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            pw[((size_t)tap * CI + cr) * NCOP + ni * 32 + li] = nq > 0 ? acc[tap][r] * inv : 0.f;
        }
    }
    __builtin_amdgcn_s_barrier();                                           // F1
    __builtin_amdgcn_s_barrier();                                           // F2: producers' bias sums are in LDS
    if (tid < D4) {
        const float4* s_red = reinterpret_cast<const float4*>(smem_ws);
        float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = tid; j < 256; j += D4) { const float4 v = s_red[j]; t4.x += v.x; t4.y += v.y; t4.z += v.z; t4.w += v.w; }
        float4* pb = reinterpret_cast<float4*>(part_b + (size_t)blockIdx.x * NCO + tid * 4);
        float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (accum) o4 = *pb;
        *pb = make_float4(o4.x + alpha * t4.x, o4.y + alpha * t4.y, o4.z + alpha * t4.z, o4.w + alpha * t4.w);
    }
}

template <int CI, int NCO, bool TR>
static hipError_t launch_wgrad_f16_ws_inst(hipStream_t st, const float* a, const float* d, float* part, float* part_b,
                                           int N, int S, int* nparts, int* ncop, int* nbias, float alpha, int accum)
{
    constexpr int MT = CI / 32, NTT = NCO / 32, KS = 4 / (MT * NTT);
    constexpr size_t buf = true ? (size_t)6 * 20 * (2 * CI * 2 + 64) + (size_t)4 * 16 * (2 * NCO * 2 + 64)
                              : (size_t)(2 * CI * 76 + 2 * NCO * 36) * 4;
    constexpr size_t lds = 2 * buf + 26 * 4 + 32;
    const int tiles_x = S / 16, tiles_y = S / 4, ntiles = N * tiles_x * tiles_y;
    const int blocks = ntiles < 256 ? ntiles : 256;
    const hipError_t e = iod_launch<conv3x3_wgrad_f16x3_ws_kernel<CI, NCO, TR>>(st, dim3(blocks), dim3(512), lds, (int)lds, a, d, part, part_b, S,
                                                                                ntiles, tiles_x, tiles_y, alpha, accum);
#ifdef IODINE_TILE_PROF
    static const char* names[8] = {"C:mfma-phase", "C:barrier", "P:load-issue", "P:split+lds-write", "P:load-wait+max", "P:barrier", "-", "P:loop-edge"};
    tp_report(st, HIP_SYMBOL(g_wgrad_prof), blocks, tp_title("[wgrad ws prof <%d,%d>] memtime ticks per TILE", CI, NCO).c_str(), names, 8, 0, ntiles);
#endif
    *nparts = blocks;                                                       // (round 6: the KS K-split sets of a block are summed before the write)
    *ncop = NTT * 32;
    *nbias = blocks;
    return e;
}

// variant 1: transposing stagers + v_alignbit shifts; variant 2: natural-order staging + ds_read_b64_tr_b16
hipError_t launch_conv3x3_wgrad_f16x3_ws(hipStream_t st, const float* a, const float* d, float* part, float* part_b, int N,
                                         int S, int ci, int nco, int* nparts, int* ncop, int* nbias_parts, float alpha, int accum)
{
    if (S % 16 != 0) return hipErrorInvalidValue;
    if (ci == 64 && nco == 64) return launch_wgrad_f16_ws_inst<64, 64, true>(st, a, d, part, part_b, N, S, nparts, ncop, nbias_parts, alpha, accum);
    if (ci == 32 && nco == 32) return launch_wgrad_f16_ws_inst<32, 32, true>(st, a, d, part, part_b, N, S, nparts, ncop, nbias_parts, alpha, accum);
    return hipErrorInvalidValue;
}
