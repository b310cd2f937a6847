// Pieces shared by the persistent kernels of the encoder's Dense layers (gemm_dxdw.hip, ffn_bwd.hip, ffn_fwd.hip, attn_out_bwd.hip):
// the sizes of their ring of [32][128] bf16 token-tile images in LDS and the LDS-DMA request that fills one.  The image's XOR
// swizzle and its fragment offsets are VTile<128>'s (mfma.h), the transposed fragment read is frag_tr2.
#pragma once
#include "mfma.h"

#define DD_TOK 32                    // tokens per tile
#define DD_SUB (DD_TOK * 256)        // one [32][128] bf16 sub-tile: 8 KB
#define DD_RING 4                    // LDS stages: the tile in work + three on their way (one tile of cover leaves the memory
                                     // system idle while the workgroup computes and waits in turn: 2.7 TB/s measured)
#define DD_OSTR 272                  // bytes per staged dX row (256 + 16)

// rows [tok0, tok0 + 32) x columns [c0, c0 + 128) of P (row pitch ld) -> LDS sub-tile at byte address lds_dst, this wave's share
// (one of the 8 wave instructions of 1 KiB: 4 rows); rows >= M arrive as zeros.
// Inline assembly, not __builtin_amdgcn_raw_ptr_buffer_load_lds: the compiler cannot tell the DMA's destination from the stages the
// loop's ds_reads address and drains the vector-memory counter right behind every request (s_waitcnt vmcnt(0): the four-stage ring
// ran as one stage).  The kernel orders a tile's arrival against its first read itself (counted s_waitcnt + barrier).
// `width_bytes` < 256: a tensor narrower than 128 columns (row pitch ld < 128): the image's columns past the width hold the next
// row's first entries, and zeros in the tile's last row -- the descriptor ends with the tile's last valid byte.
__device__ __forceinline__ void dd_dma(const bf16_t *__restrict__ P, int ld, int c0, int64_t tok0, int64_t M, unsigned lds_dst, int wave, int lane,
                                       int width_bytes = 256) {
    const int64_t left = M - tok0;
    const int64_t rows = left < 0 ? 0 : (left < DD_TOK ? left : DD_TOK);
    const int64_t bytes = rows > 0 ? (rows - 1) * (int64_t)ld * 2 + width_bytes : 0;
    const uint64_t base = (uint64_t)(P + tok0 * ld + c0);
    u32x4 rs;
    rs[0] = __builtin_amdgcn_readfirstlane((unsigned)base);
    rs[1] = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32) & 0xFFFFu);
    rs[2] = __builtin_amdgcn_readfirstlane((unsigned)bytes);
    rs[3] = 0x00020000u;
    const int row = wave * 4 + (lane >> 4), slot = lane & 15;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst + (unsigned)(wave * 1024));
    const unsigned voff = (unsigned)((row * ld + ((slot ^ VTile<128>::swz(row)) << 3)) * 2);
    // (s_nop 0: a SALU write of M0 needs one wait state before an LDS-DMA reads it -- the compiler pads its own requests, it cannot
    // see into this one.  A write of M0 right BEHIND a 16-B-per-lane request does not reach it: scratch/m0_hazard.hip, 0 misplaced
    // pieces in 39 M with and without a backlog of loads in front.)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(dst), "v"(voff), "s"(rs) : "m0");
}

