// bf16 MFMA attention for sequences past the resident kernels of attn_mfma.hip (include/b4c.h): S <= 2048.
//
// forward : a 512-thread workgroup owns 256 queries of one (sequence, head) -- wave w the 32-query tile w of the block -- and
//           streams the keys in blocks of 128 through a double-buffered K | V | mask image (2 x (2 x 128 x (2 dh + 16) + 512) B and
//           2.3 KB of padding bytes and tile flags: 77,056 B at dh = 64, two workgroups per CU; 94 .. 128 VGPRs, no spill).  The next block's rows are loaded into registers before the current
//           block's tiles are computed and written to the other stage behind them: one LDS barrier per key block.  The tile body
//           is attn_fwd_mfma_kernel's: S^T = K Q^T with the KEY on the accumulator rows, lane-local online softmax in log2 units
//           with the lazy raise of m by 2^12, P^T from the accumulator registers into O^T = V^T P^T, V^T fragments through
//           ds_read_b64_tr_b16.  The workgroups of one (sequence, head) are adjacent in the 1-D grid: its K / V come from L2.
//           CAUSAL: a query block streams the key blocks up to its own last query; the element mask runs in the diagonal tile only.
// backward: attn_bwd_mfma_kernel (attn_mfma.hip) over ceil(S / 256) <= 8 key blocks in one launch, the fp32 dQ accumulator in the
//           caller's workspace (b4c_attn_bwd_blocks, beside the kernel).
#include <math.h>

#include "mfma.h"

#define ATL_KB 128     // keys per stage
#define ATL_QB 256     // queries per workgroup
#define ATL_MAX_TILES (B4C_ATTN_LONG_MAX_S / 32)      // 64: one bit per key tile in a 64-bit mask

int b4c_attn_bwd_blocks(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o, const void *d_o, int ld_do,
                        const float *lse, void *dqkv, int ld_dqkv, int B, int S, int H, int dh, float *dq_acc, const int32_t *cu,
                        float rate, uint64_t seed, bool causal, hipStream_t st);      // attn_mfma.hip

template <int DH> struct AtlLds {
    static constexpr int KSTR = DH * 2 + 16;
    static constexpr int STAGE = 2 * ATL_KB * KSTR + ATL_KB * 4;      // K | V | mask (fp32, log2 units)
    static constexpr int BYTES = 2 * STAGE + ATL_MAX_TILES * 4 + B4C_ATTN_LONG_MAX_S;      // two stages | per key tile: any unmasked key? | the sequence's padding bytes
};

template <int DH, bool DROP, bool CAUSAL>
__global__ void __launch_bounds__(512, 4) attn_long_fwd_kernel(const bf16_t *__restrict__ qkv, int ld, const uint8_t *__restrict__ key_pad,
                                                               bf16_t *__restrict__ o, int ld_o, float *__restrict__ lse, int S_arg, int H,
                                                               int nqb, float scale, const int32_t *__restrict__ cu, float rate, uint64_t seed) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KSTR = AtlLds<DH>::KSTR, STAGE = AtlLds<DH>::STAGE;
    constexpr int NKS = DH / 16, NDT = DH / 32, CH = DH / 8;
    constexpr int NIT = ATL_KB * CH / 512;                // 16-B chunks of K (and of V) per thread and stage: 2 (dh 64) or 1
    // the query blocks of one (sequence, head) are neighbours in the grid
    const int item = blockIdx.x / nqb, qb = blockIdx.x % nqb;
    const int b = item / H, hh = item % H, dm = H * DH;
    const int S = cu ? cu[b + 1] - cu[b] : S_arg;          // packed layout: this sequence's own length
    // a query block past its sequence's end (packed layout, S_arg = the longest sequence): uniform over the workgroup, and
    // in front of the first barrier
    if (qb * ATL_QB >= S) return;
    const int64_t tok0 = cu ? (int64_t)cu[b] : (int64_t)b * S_arg;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const float scale2 = scale * 1.4426950408889634f;
    const uint32_t thr = DROP ? b4c_keep_threshold(rate) : 0u;
    int *sLive = reinterpret_cast<int *>(smem + 2 * STAGE);
    uint8_t *sPad = reinterpret_cast<uint8_t *>(sLive + ATL_MAX_TILES);
    const bf16_t *kbase = qkv + tok0 * ld + dm + hh * DH;
    const bf16_t *vbase = kbase + dm;
    const int nqt = (S + 31) >> 5;                         // 32-row tiles of the sequence (queries and keys alike)
    const int qt = qb * (ATL_QB / 32) + wave;              // this wave's query tile, counted inside the sequence
    const bool active = qt < nqt;                          // wave-uniform
    const int q_end = (qb + 1) * ATL_QB < S ? (qb + 1) * ATL_QB : S;
    const int nkb = ((CAUSAL ? q_end : S) + ATL_KB - 1) / ATL_KB;      // key blocks this workgroup streams
    const int nkt_vis = CAUSAL ? qt + 1 : nqt;             // key tiles this wave's queries see: kt < nkt_vis

    // which key tiles hold an unmasked key: the whole sequence's padding bytes, four per thread (unconditional loads on a
    // clamped index), one ballot per load -- lanes 0..31 are one tile, 32..63 the next
#pragma unroll
    for (int i = 0; i < B4C_ATTN_LONG_MAX_S / 512; ++i) {
        const int k = i * 512 + tid;
        const uint8_t pd = key_pad[tok0 + (k < S ? k : S - 1)];
        sPad[k] = pd;
        const unsigned long long bl = __ballot(k < S && !pd);
        if (lane == 0) {
            sLive[i * 16 + 2 * wave] = (unsigned)bl != 0u;
            sLive[i * 16 + 2 * wave + 1] = (unsigned)(bl >> 32) != 0u;
        }
    }
    bf16x8 qf[NKS];
    {
        const int qrow = qt * 32 + r;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (active && qrow < S) v = *reinterpret_cast<const u32x4 *>(qkv + (tok0 + qrow) * ld + hh * DH + ks * 16 + hf * 8);
            qf[ks] = __builtin_bit_cast(bf16x8, v);
        }
    }
    // one stage = 128 keys: loaded into registers early, written to LDS behind the compute of the stage before
    u32x4 rk[NIT], rv[NIT];
    auto prefetch = [&](int kb) {
        const int key0 = kb * ATL_KB;
        // (a workgroup-uniform 64-bit base and a 32-bit lane offset inside the block: row < 128)
        const bf16_t *kblk = kbase + (int64_t)key0 * ld, *vblk = vbase + (int64_t)key0 * ld;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int c = tid + it * 512, row = c / CH, part = c % CH;
            rk[it] = rv[it] = (u32x4){0u, 0u, 0u, 0u};
            if (key0 + row < S) {
                rk[it] = *reinterpret_cast<const u32x4 *>(kblk + (unsigned)(row * ld + part * 8));
                rv[it] = *reinterpret_cast<const u32x4 *>(vblk + (unsigned)(row * ld + part * 8));
            }
        }
    };
    auto commit = [&](int kb) {
        char *st = smem + (kb & 1) * STAGE;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int c = tid + it * 512, row = c / CH, part = c % CH;
            *reinterpret_cast<u32x4 *>(st + row * KSTR + part * 16) = rk[it];
            *reinterpret_cast<u32x4 *>(st + (ATL_KB + row) * KSTR + part * 16) = rv[it];
        }
        if (tid < ATL_KB) {
            const int k = kb * ATL_KB + tid;
            reinterpret_cast<float *>(st + 2 * ATL_KB * KSTR)[tid] = (k >= S) ? -INFINITY : (sPad[k] ? -1e9f * 1.4426950408889634f : 0.f);
        }
    };
    prefetch(0);
    B4C_LDS_BARRIER();                 // the padding bytes: a stage's mask is written from them
    commit(0);
    B4C_LDS_BARRIER();
    // Fully padded key tiles contribute exp(-1e9 - m) == 0 and are skipped -- unless the queries see no unmasked key at all, where
    // the softmax degenerates to uniform weights over what they see: then every visible tile is processed.  Bidirectional: the
    // whole sequence without a live key.  CAUSAL: per query tile over its visible tiles 0 .. qt (leading pads).
    const unsigned long long live_bits = __ballot(sLive[lane] != 0);
    const bool force = CAUSAL ? !(live_bits & ((2ull << qt) - 1ull)) : live_bits == 0ull;

    float m = -INFINITY, l = 0.f;
    f32x16 oacc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int t = 0; t < 16; ++t) oacc[dt][t] = 0.f;
    const uint32_t s4q = b4c_attn_s4(S_arg) >> 2, dq = (uint32_t)(qt * 32 + r) * s4q;      // dropout counter, the query's part: < 2^20

    for (int kb = 0; kb < nkb; ++kb) {
        const bool more = kb + 1 < nkb;
        if (more) prefetch(kb + 1);
        const char *sK = smem + (kb & 1) * STAGE, *sV = sK + ATL_KB * KSTR;
        const float *sMask = reinterpret_cast<const float *>(sK + 2 * ATL_KB * KSTR);
        for (int j = 0; j < ATL_KB / 32; ++j) {
            const int kt = kb * (ATL_KB / 32) + j;             // key tile inside the sequence; j inside the stage
            if (!active || kt >= nkt_vis) break;               // wave-uniform
            if (!(((live_bits >> kt) & 1ull) || force)) continue;
            f32x16 acc;
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[t] = 0.f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8 *>(sK + (j * 32 + r) * KSTR + ks * 32 + hf * 16);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
            float tm = -INFINITY;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                acc[t] = __builtin_fmaf(acc[t], scale2, sMask[j * 32 + rowmap(t, hf)]);
                if (!CAUSAL) tm = fmaxf(tm, acc[t]);
            }
            if (CAUSAL) {
                if (kt == qt) {                                // the diagonal tile (wave-uniform): keys behind the lane's query are out
#pragma unroll
                    for (int t = 0; t < 16; ++t) acc[t] = rowmap(t, hf) > r ? -INFINITY : acc[t];
                }
#pragma unroll
                for (int t = 0; t < 16; ++t) tm = fmaxf(tm, acc[t]);
            }
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const bool raise = tm > m + 12.0f;
            if (__any(raise)) {
                if (raise) {
                    const float al = __builtin_amdgcn_exp2f(m - tm);          // 0 at the first live tile (m = -inf)
                    m = tm;
                    l *= al;
#pragma unroll
                    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                        for (int t = 0; t < 16; ++t) oacc[dt][t] *= al;
                }
            }
            const float mref = (m == -INFINITY) ? 0.f : m;                    // a tile of -inf scores only: p = 0
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                acc[t] = __builtin_amdgcn_exp2f(acc[t] - mref);
                l += acc[t];
            }
            if (DROP) {
                // l keeps the undropped sum.  Registers 4 tq .. 4 tq + 3 are the keys kt*32 + 8 tq + 4 hf + {0..3} of this lane's
                // query: one hash.
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) {
                    const uint32_t kbits = b4c_attn_keep4(seed, attn_ctr_base(item, S_arg) + (dq + (uint32_t)(kt * 8 + 2 * tq + hf)), thr);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[4 * tq + jj] = ((kbits >> jj) & 1u) ? acc[4 * tq + jj] : 0.f;
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float pv[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) pv[jj] = acc[8 * s2 + jj];
                const bf16x8 pf = pack8(pv);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    // V^T[dh = dt*32 + r][keys j*32 + 16 s2 + 4 hf + {0..3, 8..11}] from row-major V
                    const char *vb = sV + (j * 32 + 16 * s2 + 4 * hf + (li >> 2)) * KSTR + (dt * 32 + 16 * (g & 1) + 4 * (li & 3)) * 2;
                    const bf16x8 vf = frag_tr(vb, 8 * KSTR);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[dt], 0, 0, 0);
                }
            }
        }
        if (more) commit(kb + 1);      // the other stage: every wave left it at the barrier that ended the block before
        B4C_LDS_BARRIER();
    }
    l += __shfl_xor(l, 32);
    // O^T (dh on the registers, query on the lane) -> row-major bf16 through this wave's slice of the stages (dead behind the
    // last barrier), then whole 16-B chunks: full rows per store instruction.
    if (active) {
        const float inv = DROP ? (1.0f / (1.0f - rate)) / l : 1.0f / l;
        char *st = smem + wave * (32 * KSTR);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                bf16x4 w;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) w[jj] = (bf16_t)(oacc[dt][4 * tq + jj] * inv);
                *reinterpret_cast<bf16x4 *>(st + r * KSTR + (dt * 32 + 8 * tq + 4 * hf) * 2) = w;
            }
#pragma unroll
        for (int i = 0; i < 32 * CH / 64; ++i) {
            const int c = lane + 64 * i, row = c / CH, part = c % CH;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(st + row * KSTR + part * 16);
            if (qt * 32 + row < S) {
                bf16_t *dst = o + (tok0 + qt * 32 + row) * ld_o + hh * DH + part * 8;
                if (B4C_NT(B4C_NT_ATTN_O)) __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(dst));
                else *reinterpret_cast<u32x4 *>(dst) = v;
            }
        }
        const int qrow = qt * 32 + r;
        if (qrow < S && hf == 0 && lse) lse[((int64_t)b * H + hh) * S_arg + qrow] = (m + __log2f(l)) * 0.6931471805599453f;
    }
}

// ------------------------------------------------------------------------------------------
// the argument checks of both directions, in the header's order; no pointer is looked at
static int atl_check(const char *who, int ld_qkv, int ld_o, int B, int S, int H, int dh, float rate, uint32_t flags) {
    B4C_REQUIRE((flags & ~B4C_ATTN_CAUSAL) == 0, "%s: unknown flag bits 0x%x in flags", who, flags & ~B4C_ATTN_CAUSAL);
    B4C_REQUIRE(rate >= 0.f && rate < 1.f, "%s: dropout_rate %g outside [0, 1)", who, (double)rate);
    B4C_REQUIRE(dh == 32 || dh == 64, "%s: head depth dh = %d not in {32, 64}", who, dh);
    B4C_REQUIRE(S >= 1 && S <= B4C_ATTN_LONG_MAX_S, "%s: S = %d outside [1, %d]", who, S, B4C_ATTN_LONG_MAX_S);
    B4C_REQUIRE(B > 0 && H > 0, "%s: bad shape (B = %d, H = %d)", who, B, H);
    B4C_REQUIRE((int64_t)B * H * ((S + ATL_QB - 1) / ATL_QB) <= 2147483647ll, "%s: B * H * ceil(S / 256) exceeds the grid limit 2^31 - 1", who);
    // (ld_qkv < 2^22: the forward addresses the 128 rows of a key block with a 32-bit offset)
    B4C_REQUIRE((int64_t)ld_qkv >= 3ll * H * dh && ld_qkv % 8 == 0 && ld_qkv < (1 << 22) && (int64_t)ld_o >= (int64_t)H * dh && ld_o % 8 == 0,
                "%s: bad pitch (ld_qkv = %d, ld_o = %d)", who, ld_qkv, ld_o);
    return B4C_OK;
}

extern "C" int b4c_attn_long_fwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o, int ld_o,
                                 float *lse, int B, int S, int H, int dh, void *stream, float dropout_rate, uint64_t seed,
                                 uint32_t flags) {
    if (int rc = atl_check("attn_long_fwd", ld_qkv, ld_o, B, S, H, dh, dropout_rate, flags)) return rc;
    B4C_REQUIRE(qkv && key_pad && o, "attn_long_fwd: null pointer");
    const bool causal = (flags & B4C_ATTN_CAUSAL) != 0;
    const int nqb = (S + ATL_QB - 1) / ATL_QB;
    const float scale = 1.0f / sqrtf((float)dh);
    hipStream_t st = (hipStream_t)stream;
    b4c_by_int<32, 64>(dh, [&](auto DH) { b4c_by_bool(dropout_rate != 0.f, [&](auto DR) { b4c_by_bool(causal, [&](auto CA) {
        constexpr size_t shm = AtlLds<DH()>::BYTES;
        b4c_allow_lds(attn_long_fwd_kernel<DH(), DR(), CA()>, shm);
        attn_long_fwd_kernel<DH(), DR(), CA()><<<B * H * nqb, 512, shm, st>>>((const bf16_t *)qkv, ld_qkv, key_pad, (bf16_t *)o, ld_o, lse, S, H, nqb, scale, cu_seqlens, dropout_rate, seed);
    }); }); });
    return b4c_check_launch("attn_long_fwd");
}

extern "C" int64_t b4c_attn_long_bwd_workspace_bytes(int64_t rows, int H, int dh) {
    if (rows < 0 || H <= 0 || (dh != 32 && dh != 64)) return -1;
    return rows * H * dh * (int64_t)sizeof(float);       // fp32 dQ accumulator across the key blocks
}

extern "C" int b4c_attn_long_bwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o, int ld_o,
                                 const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B, int S,
                                 int H, int dh, void *workspace, int64_t workspace_bytes, void *stream, float dropout_rate,
                                 uint64_t seed, uint32_t flags) {
    if (int rc = atl_check("attn_long_bwd", ld_qkv, ld_o, B, S, H, dh, dropout_rate, flags)) return rc;
    B4C_REQUIRE(ld_do >= H * dh && ld_do % 8 == 0 && ld_dqkv >= 3 * H * dh && ld_dqkv % 8 == 0, "attn_long_bwd: bad pitch (ld_do = %d, ld_dqkv = %d)", ld_do, ld_dqkv);
    // (the packed layout's row count cu_seqlens[B] lives on the device: B * S bounds it, and is what a dense launch has)
    const int64_t need = cu_seqlens ? 0 : b4c_attn_long_bwd_workspace_bytes((int64_t)B * S, H, dh);
    B4C_REQUIRE(workspace_bytes >= need && workspace_bytes >= (int64_t)H * dh * (int64_t)sizeof(float),
                "attn_long_bwd: workspace_bytes = %lld, needs %lld (b4c_attn_long_bwd_workspace_bytes)", (long long)workspace_bytes, (long long)need);
    B4C_REQUIRE(qkv && key_pad && o && d_o && lse && delta && dqkv && workspace, "attn_long_bwd: null pointer");
    return b4c_attn_bwd_blocks(qkv, ld_qkv, key_pad, o, ld_o, d_o, ld_do, lse, dqkv, ld_dqkv, B, S, H, dh, (float *)workspace, cu_seqlens,
                               dropout_rate, seed, (flags & B4C_ATTN_CAUSAL) != 0, (hipStream_t)stream);
}
