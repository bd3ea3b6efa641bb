// The persistent, XCD-aware tile schedule, both halves in one place: the grid a launcher asks for (iod_xcd_grid) and the tiles a
// block of that grid takes (xcd_span).  Block b runs on XCD b % 8 (observed; speed only), so every XCD gets one contiguous eighth
// of the tile list and the blocks that share an L2 work on neighbouring tiles.
// PRECONDITION: the grid is a multiple of 8, or xcd_order is false.  Then every tile of [0, ntiles) is taken by exactly one block
// (tests/test_launch_cpu.py); with another grid the XCD order would leave tiles out.
// xcd_span is the statement of the device half: the five persistent kernels (conv3x3_ws_f16x3, refine_bwd01, conv3x3_wgrad_f32_ws,
// dec_out_wgrad_f32, conv3x3_wgrad_f16x3_ws) spell the same arithmetic out in their prologues, because through the function the
// compiler orders their scalar instructions differently (profiles/launch_helpers_equivalence.md); a new kernel calls it.
// Nothing from HIP is included: a plain C++ compiler can build this header.
#pragma once

#ifdef __HIPCC__
#define IOD_HD __host__ __device__
#else
#define IOD_HD
#endif

// the tiles of one block: first, first + stride, ... < end
struct XcdSpan { int first, end, stride; };

// block b of nblk; xcd_order false: the plain order b, b + nblk, ... (any grid)
IOD_HD inline XcdSpan xcd_span(int ntiles, int nblk, int b, bool xcd_order = true)
{
    if (!xcd_order) return XcdSpan{b, ntiles, nblk};
    const int xcd = b & 7, bix = (int)((unsigned)b >> 3), bpx = (nblk + 7) >> 3;
    const int per_xcd = (ntiles + 7) >> 3;
    const int t_begin = xcd * per_xcd, t_stop = t_begin + per_xcd;
    return XcdSpan{t_begin + bix, ntiles < t_stop ? ntiles : t_stop, bpx};
}

// grid of a persistent kernel on n_cu compute units with blocks_per_cu resident blocks each: a multiple of 8, at most one block per tile
// of an XCD's eighth.  (A caller that caps the result caps it to a multiple of 8.)
inline int iod_xcd_grid(int ntiles, int blocks_per_cu, int n_cu)
{
    const int per_xcd = (ntiles + 7) / 8, fill = blocks_per_cu * n_cu / 8;
    const int bpx = fill < 1 ? 1 : fill;
    return 8 * (per_xcd < bpx ? per_xcd : bpx);
}
