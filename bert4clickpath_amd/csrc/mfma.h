// Matrix-core fragment helpers shared by every kernel file that uses v_mfma_f32_32x32x16_bf16 (gfx950; wave = 64).
//
// Operand maps (lane l: r = l & 31, hf = l >> 5):
//   A[row r][k = 8 hf + j], B[k = 8 hf + j][col r], j = 0..7;  D reg t: row (t&3) + 8 (t>>2) + 4 hf, col r  (rowmap).
//   An accumulator tile X used as the B operand of the next MFMA (summing over X's rows): k-step s takes
//   regs 8s..8s+7 (pack8), whose rows are 16 s + 8 (j>>2) + 4 hf + (j&3) -- the A operand must use the same k order:
//   two 8-byte pieces 8 rows apart, read transposed from a row-major image (frag_tr) or plainly from a transposed one
//   (frag_from_2x8B).
#pragma once
#include "common.h"

__device__ __forceinline__ int rowmap(int t, int hf) { return (t & 3) + 8 * (t >> 2) + 4 * hf; }
__device__ __forceinline__ bf16x8 pack8(const float *p) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16_t)p[j];
    return v;
}
__device__ __forceinline__ bf16x8 frag_from_2x8B(const char *p0, const char *p1) {
    const u32x2 lo = *reinterpret_cast<const u32x2 *>(p0);
    const u32x2 hi = *reinterpret_cast<const u32x2 *>(p1);
    u32x4 w = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_bit_cast(bf16x8, w);
}

// 4 rows x 16 columns of bf16 read transposed (ds_read_b64_tr_b16): lane i of each 16-lane group gets
// column (col0 + i) of rows row0..row0+3; the lane supplies the address of row (i>>2), columns 4(i&3)...
// Checked on MI355X with integer data (scratch/trtest.hip).  EXEC must be full.
__device__ __forceinline__ s16x4 tr_read(const char *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)(p));
}
// one A / B fragment from two such pieces (rows +0..3 and, 8 rows on, +8..11 of the lane's column)
__device__ __forceinline__ bf16x8 frag_tr2(const char *p0, const char *p1) {
    const s16x4 a = tr_read(p0), b = tr_read(p1);
    const s16x8 w = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, w);
}
__device__ __forceinline__ bf16x8 frag_tr(const char *p, int second_off) { return frag_tr2(p, p + second_off); }

// ---- attention-probability dropout in the BACKWARD matrix-core attention kernels ----
// Keep bits of one 32 x 32 score tile, with the KEY on the lane (r) and the QUERY on the accumulator rows (rowmap): bit t =
// register t.  The keep rule (common.h) hashes four consecutive keys of one query at once, and the four lanes of a quad hold
// exactly such four keys: each lane hashes the queries of the registers (r & 3) + 4 tq, tq = 0..3, and the quad exchanges the
// bits (DPP quad broadcast) -- four hashes per lane per tile, as in the forward, where the four keys are four registers of one
// lane.  The hash counter b4c_attn_ctr(row, k0, S_arg) is split into the workgroup-uniform base = attn_ctr_base(b*H + h, S_arg)
// and a 32-bit lane part q * (S4 / 4) + k0 / 4 (q < 2048, S4 / 4 <= 512 with the key-block walk of attn_long.hip: below 2^21).  qpos(i) = position of the query of tile row i inside its
// sequence, k_tile = first key of the tile.  EXEC must be full.
template <typename QPos>
__device__ __forceinline__ uint32_t keep_tile_bwd(uint64_t seed, uint64_t base, int S_arg, QPos qpos, int k_tile, uint32_t thr, int r, int hf) {
    const int c = r & 3;
    const uint32_t s4q = b4c_attn_s4(S_arg) >> 2, kq = (uint32_t)(k_tile + (r & ~3)) >> 2;
    uint32_t mk = 0;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq)
        mk |= b4c_attn_keep4(seed, base + ((uint32_t)qpos(c + 8 * tq + 4 * hf) * s4q + kq), thr) << (4 * tq);
    uint32_t km = ((quad_bcast<0>(mk) >> c) & 0x1111u);
    km |= ((quad_bcast<1>(mk) >> c) & 0x1111u) << 1;
    km |= ((quad_bcast<2>(mk) >> c) & 0x1111u) << 2;
    km |= ((quad_bcast<3>(mk) >> c) & 0x1111u) << 3;
    return km;
}

// ---- XOR-swizzled LDS image of a row tile ----
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vtile_rsrc(const void *base, int64_t rows, int64_t row_bytes) {
    int64_t bytes = (rows < 0 ? 0 : rows) * row_bytes;
    if (bytes > 0x3FFFFFF0ll) bytes = 0x3FFFFFF0ll;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (unsigned)bytes, 0x00020000);
}

// A [128 rows][KD] bf16 tile in LDS, filled by LDS-DMA (buffer_load ... lds: no staging registers, no ds_write).
// Rows are unpadded (KD * 2 bytes); the 16-B chunk c of row j sits at chunk c ^ f(j):
//   KD = 128 (a row = one 256-B bank row):   f(j) = ((j & 3) << 2) | ((j >> 2) & 3)
//   KD =  64 (two rows per bank row):        f(j) = (((j >> 1) & 1) << 2) | ((j >> 2) & 3)
// so that a transposed read (32-lane group: 4 consecutive rows x the same 64 B) and a direct fragment read
// (ds_read_b128 16-lane groups: rows {0-3,12-15,20-27} / {4-11,16-19,28-31}, same chunk) both land on distinct
// 16-B slots of the 64 banks (MI355X_MICROARCH.md, LDS).  An LDS-DMA wave instruction writes 64 x 16 B
// contiguously (lane l -> base + 16 l), so the swizzle is applied to the SOURCE address of each lane.
template <int KD> struct VTile {
    static constexpr int CH = KD / 8;            // 16-B chunks per row
    static constexpr int NIT = 128 * CH / 512;   // DMA instructions per thread: 4 (KD = 128) or 2 (KD = 64)
    static constexpr int STR = KD * 2;
    static constexpr int BYTES = 128 * STR;
    static __device__ __forceinline__ int swz(int row) {
        return KD == 128 ? (((row & 3) << 2) | ((row >> 2) & 3)) : ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
    }
    static __device__ __forceinline__ int chunk_off(int row, int chunk) { return row * STR + ((chunk ^ swz(row)) << 4); }
    // rows [row0, row0 + 128) of P (row pitch ld elements) -> LDS tile at `dst`; rows >= nrows arrive as zeros.
    // Completion is on the VM counter: s_waitcnt vmcnt(0) + a barrier before any wave reads the tile.
    template <int NT = 512>
    static __device__ __forceinline__ void dma(const bf16_t *__restrict__ P, int ld, int64_t row0, int64_t nrows, char *dst, int tid) {
        const int64_t left = nrows - row0;
        const __amdgpu_buffer_rsrc_t rs = vtile_rsrc(P + row0 * ld, left < 128 ? left : 128, (int64_t)ld * 2);
#pragma unroll
        for (int i = 0; i < NIT * 512 / NT; ++i) {
            const int c = tid + i * NT, row = c / CH, slot = c % CH;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(dst + ((c & ~63) << 4)), 16,
                                                     (row * ld + ((slot ^ swz(row)) << 3)) * 2, 0, 0, 0);
        }
    }
    // one DMA instruction of the same transfer (piece i of NIT * 512 / NT; a 256-thread workgroup spreads them over its loop)
    template <int NT>
    static __device__ __forceinline__ void dma_piece(const bf16_t *__restrict__ P, int ld, int64_t row0, int64_t nrows, char *dst, int tid, int i) {
        const int64_t left = nrows - row0;
        const __amdgpu_buffer_rsrc_t rs = vtile_rsrc(P + row0 * ld, left < 128 ? left : 128, (int64_t)ld * 2);
        const int c = tid + i * NT, row = c / CH, slot = c % CH;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(dst + ((c & ~63) << 4)), 16,
                                                 (row * ld + ((slot ^ swz(row)) << 3)) * 2, 0, 0, 0);
    }
    // The same piece as inline assembly, for a loop whose LDS slots are run-time values: through the builtin the compiler
    // cannot tell the DMA's destination from the slots the loop's ds_reads address and parks every wave on vmcnt(0) after
    // each piece (400 cycles per piece measured).  Here it sees no LDS write at all: the caller orders the tile's arrival
    // against its first read itself (s_waitcnt vmcnt(0) + barrier), as every sweep of vocab_ce.hip does anyway.
    // lds_base: LDS byte address of the slot (wave-uniform); wave: the wave's index (wave-uniform).
    template <int NT>
    static __device__ __forceinline__ void dma_piece_asm(const bf16_t *__restrict__ P, int ld, int64_t row0, int64_t nrows, unsigned lds_base,
                                                         int wave, int lane, int i) {
        const int64_t left = nrows - row0;
        int64_t bytes = (left < 0 ? 0 : (left < 128 ? left : 128)) * (int64_t)ld * 2;
        if (bytes > 0x3FFFFFF0ll) bytes = 0x3FFFFFF0ll;
        const uint64_t base = (uint64_t)(P + row0 * ld);
        u32x4 rs;
        rs[0] = __builtin_amdgcn_readfirstlane((unsigned)base);
        rs[1] = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32) & 0xFFFFu);
        rs[2] = __builtin_amdgcn_readfirstlane((unsigned)bytes);
        rs[3] = 0x00020000u;
        const int c = wave * 64 + lane + i * NT, row = c / CH, slot = c % CH;
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)((wave * 64 + i * NT) << 4));
        const unsigned voff = (unsigned)((row * ld + ((slot ^ swz(row)) << 3)) * 2);
        // (s_nop 0: one wait state between a SALU write of M0 and an LDS-DMA that reads it -- csrc/dxdw_common.h dd_dma)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(dst), "v"(voff), "s"(rs) : "m0");
    }
    // per-lane offsets, relative to a row base that is a multiple of 16 rows:
    //   direct fragment (row r, k-step ks, half hf): 16 B
    static __device__ __forceinline__ int frag_off(int r, int ks, int hf) { return chunk_off(r, 2 * ks + hf); }
    //   transposed fragment piece of MFMA 32x32x16 (A or B operand: column `32 dt + r`, rows 8 hf + 0..7 of a 16-row step): the
    //   lane's address is row 4 hf + (li >> 2) (+ 8 for the second piece), columns 32 dt + 16 (g & 1) + 4 (li & 3)
    static __device__ __forceinline__ int tr_off(int hf, int li, int g, int dt, int second) {
        const int row = 4 * hf + (li >> 2) + 8 * second;
        const int e = dt * 32 + 16 * (g & 1) + 4 * (li & 3);
        return chunk_off(row, e >> 3) + (e & 7) * 2;
    }
};
