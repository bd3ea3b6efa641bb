// The extent of every weight pack, once.  A pack is a device buffer in the order a kernel fetches its MFMA operands; iodine_create and the
// operator-level entries allocate it, a pack kernel fills it (pack_bodies.h, the pack_* kernels), a conv kernel stages it.  All three take
// the size from here: the *_vecs functions count the vectors the kernels index by (16 bytes unless noted), *_bytes is what is allocated.
// A split-fp16 pack travels with a `meta` block holding its power-of-two scale.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// meta block of a split-fp16 pack: {scale, 1 / scale} of the forward pack, then the same pair of the data-gradient pack of the same tensor
// (a pack without a sibling uses the first pair; allocated as one block of four either way)
constexpr size_t WPK_META_FLOATS = 4;

// weight-stationary 3x3 conv C -> C (kernels_convws.hip, kernels_refws.hip, kernels_refbwd.hip):
// [cout group of 16][chunk of 32 cin][tap][hi/lo][lane][8 fp16] = the A operand of v_mfma_f32_16x16x32_f16 (lane l: row = cout 16 cg + l % 16,
// k = cin 32 c + 8 (l / 16) .. + 7).  Its exact-fp32 form has the same byte count: [cout group][chunk][tap][half][lane][4 fp32]
__host__ __device__ constexpr size_t wpk_ws_vecs(int C) { return (size_t)(C / 16) * (C / 32) * 9 * 2 * 64; }
__host__ __device__ constexpr size_t wpk_ws_bytes(int C) { return wpk_ws_vecs(C) * 16; }

// LDS-tile 3x3 conv, split fp16 (kernels_conv.hip; cin padded to 16): [chunk of 16 cin][tap][hi/lo][k half][cout][8 fp16]
__host__ __device__ constexpr size_t wpk_tile_f16_vecs(int cin, int cout) { return (size_t)(cin / 16) * 9 * 2 * 2 * cout; }
__host__ __device__ constexpr size_t wpk_tile_f16_bytes(int cin, int cout) { return wpk_tile_f16_vecs(cin, cout) * 16; }
// stride-2 tile (kernels_refine.hip): the LDS-tile f16 layout; its exact-fp32 form keeps the byte count, [chunk of 16 cin][tap][term][k half]
// [cout][4 fp32] with element e of slot (term, kh, co) = input channel 16 chunk + 8 kh + 4 term + e
__host__ __device__ constexpr size_t wpk_s2_tile_bytes(int cin, int cout) { return wpk_tile_f16_bytes(cin, cout); }

// LDS-tile 3x3 conv, fp32 (kernels_conv.hip: tile and gather kernels).  A conv with CIN (padded) input channels is cut into chunks of CC
// channels.  Inside a chunk the reduction index is organised in "quads" q = tap * (CC/4) + cig: 4 consecutive input channels (cig*4 .. +3)
// at filter tap `tap` (= dy*3+dx).  Quads are consumed in pairs by v_mfma_f32_32x32x2_f32: lanes 0-31 feed quad 2g, lanes 32-63 quad 2g+1,
// element s of the quad at MFMA step s.  wpk[chunk][q][co] is a float4 over the quad's 4 channels.
__host__ __device__ constexpr int conv_cc(int cin) { return cin == 20 ? 20 : (cin >= 16 ? 16 : cin); }
__host__ __device__ constexpr int conv_nq(int cin) { return 9 * (conv_cc(cin) / 4); }
__host__ __device__ constexpr int conv_nqp(int cin) { return (conv_nq(cin) + 1) & ~1; }
__host__ __device__ constexpr int conv_nchunk(int cin) { return cin / conv_cc(cin); }
// float4 elements in a packed weight tensor
__host__ __device__ constexpr size_t conv_wpk_elems(int cin, int cout) { return (size_t)conv_nchunk(cin) * conv_nqp(cin) * cout; }
__host__ __device__ constexpr size_t wpk_tile_f32_bytes(int cin, int cout) { return conv_wpk_elems(cin, cout) * 16; }

// fused first refinement layer (kernels_refl0.hip), one operand per input part: [O / 16][9 taps][hi/lo][64 lanes][4 fp16]; vectors of 8 bytes
__host__ __device__ constexpr size_t wpk_l0_vecs(int O) { return (size_t)(O / 16) * 9 * 2 * 64; }
__host__ __device__ constexpr size_t wpk_l0_bytes(int O) { return wpk_l0_vecs(O) * 8; }

// output conv C -> 4, GEMM form (kernels_out.hip forward, stream and rows): [chunk of 16 ci][term hi/lo][kh][n 0..63][8 fp16],
// n = tap * 4 + co (n >= 36 zero)
__host__ __device__ constexpr size_t wpk_out_gemm_vecs(int C) { return (size_t)(C / 16) * 2 * 2 * 64; }
__host__ __device__ constexpr size_t wpk_out_gemm_bytes(int C) { return wpk_out_gemm_vecs(C) * 16; }

// output conv, data-gradient form (kernels_out.hip, kernels_outbwd.hip): [chunk 3][term hi/lo][kh 2][C][8 fp16], k = chunk * 16 + kh * 8 + e
// = tap * 4 + o (zero for k >= 36)
__host__ __device__ constexpr size_t wpk_out_dgrad_vecs(int C) { return (size_t)3 * 2 * 2 * C; }
__host__ __device__ constexpr size_t wpk_out_dgrad_bytes(int C) { return wpk_out_dgrad_vecs(C) * 16; }

// output conv, `rows32`: the fp32 operand of the row-streaming kernel's exact form, dst[(nt * (C / 2) + ks) * 64 + lane] = W[column nt * 32 +
// lane % 32 (= tap * 4 + co, zero from 36)][channel of (k-step ks, half wave lane / 32) = 16 (ks / 8) + 8 (lane / 32) + ks % 8]
__host__ __device__ constexpr size_t wpk_out_rows32_floats(int C) { return (size_t)2 * (C / 2) * 64; }
__host__ __device__ constexpr size_t wpk_out_rows32_bytes(int C) { return wpk_out_rows32_floats(C) * 4; }

// output conv, fp32 tap form of the round-1 kernel (launch_pack_dec_out): [tap][ci][4 co] fp32
__host__ __device__ constexpr size_t wpk_out_taps_bytes(int C) { return (size_t)9 * C * 4 * 4; }

// generic path (kernels_generic.hip, kernels_gens2.hip, kernels_genl0.hip): [tap][ci][co] fp32, k x k taps
__host__ __device__ constexpr size_t wpk_gen_floats(int k, int ci, int co) { return (size_t)k * k * ci * co; }
__host__ __device__ constexpr size_t wpk_gen_bytes(int k, int ci, int co) { return wpk_gen_floats(k, ci, co) * 4; }

// generic split slices (kernels_gensplit.hip), one direction of a conv k x k, C -> C staged in chunks of cch = 32 or 16 channels
// (gen_split_cch): per group of 16 output channels one slice image, blocks of 1 KB [k-group kq][16 output channels][8 halves], hi image then
// lo image of every MFMA group (32 / cch taps per MFMA); meta: one inverse scale per slice
__host__ __device__ constexpr size_t wpk_gen_split_slice_bytes(int k, int C, int cch) {
    return (size_t)(C / cch) * ((k * k + 32 / cch - 1) / (32 / cch)) * 2048;
}
__host__ __device__ constexpr size_t wpk_gen_split_bytes(int k, int C, int cch) { return (size_t)(C / 16) * wpk_gen_split_slice_bytes(k, C, cch); }
__host__ __device__ constexpr size_t wpk_gen_split_meta_floats(int C) { return (size_t)(C / 16); }

// the values every layout had before it was written down here
static_assert(wpk_ws_bytes(64) == 147456 && wpk_ws_bytes(32) == 36864, "weight-stationary pack");
static_assert(wpk_tile_f16_bytes(64, 64) == 147456 && wpk_tile_f16_bytes(32, 64) == 73728, "LDS-tile f16 pack");
static_assert(wpk_tile_f16_bytes(16, 32) == 576 * 32 && wpk_tile_f16_bytes(16, 64) == 576 * 64 && wpk_s2_tile_bytes(16, 4) == 576 * 4,
              "split first layer: 576 bytes per output channel");
static_assert(wpk_tile_f32_bytes(64, 64) == 4 * 36 * 64 * 16 && wpk_tile_f32_bytes(20, 32) == 46 * 32 * 16, "LDS-tile f32 pack");
static_assert(wpk_out_gemm_bytes(64) == 16384 && wpk_out_gemm_bytes(32) == 8192, "output conv, GEMM form");
static_assert(wpk_out_dgrad_bytes(64) == 192 * 64 && wpk_out_dgrad_bytes(32) == 192 * 32 && wpk_out_dgrad_bytes(8) == 192 * 8,
              "output conv, data-gradient form: 192 bytes per channel");
static_assert(wpk_l0_bytes(64) == 36864, "fused first refinement layer");
static_assert(wpk_out_rows32_bytes(64) == 16384 && wpk_out_rows32_bytes(32) == 8192, "output conv, rows32");
// the operator-level entry of the output conv keeps rows32 where it allocated the GEMM-form pack (iodine_op_dec_out_f16x3, variant 3)
static_assert(wpk_out_rows32_bytes(64) <= wpk_out_gemm_bytes(64) && wpk_out_rows32_bytes(32) <= wpk_out_gemm_bytes(32), "rows32 fits the GEMM-form pack");
static_assert(wpk_gen_split_bytes(5, 64, 32) == 4 * 2 * 25 * 2048 && wpk_gen_split_bytes(3, 48, 16) == 3 * 3 * 5 * 2048, "generic split slices");
