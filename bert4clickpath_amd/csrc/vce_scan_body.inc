// Body of vce_scan_kernel / vce_scan_excl_kernel (vocab_ce.hip): included inside each kernel, with `a` its argument block and
// EX whether it takes exclusion lists.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NKS = KD / 16, STR = VTile<KD>::STR;
    constexpr int TILE_B = VTile<KD>::BYTES;
    float *sBias = reinterpret_cast<float *>(smem + 2 * TILE_B);     // [3][128]: a ring -- the scores of a tile's second half are
                                                                     // formed one tile later, while the next bias arrives
    const int unit = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hf = lane >> 5;
    const int tg = NH == 2 ? wave : (wave & 3), vh = NH == 2 ? 0 : (wave >> 2);
    const int64_t tok0 = (int64_t)(unit % a.ntt) * (128 * NH);
    const int64_t tok = tok0 + tg * 32 + r;
    const int part = unit / a.ntt;
    const int nvt = (a.V + 127) >> 7;
    const int vt0 = (int)((int64_t)nvt * part / a.parts), vt1 = (int)((int64_t)nvt * (part + 1) / a.parts);
    const bool live = tok < a.R;

    bf16x8 hfr[NKS];
    vce_load_hfrag<KD>(a.h, a.ld_h, tok, a.R, hf, hfr);
    int foff[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) foff[ks] = VTile<KD>::frag_off(r, ks, hf) + vh * 64 * STR;

    // per-lane state
    float ref = INFINITY;          // RANK: x_y;  COLLECT: tau  (+inf: nothing counts / nothing is collected)
    int y = -1;
    if (OP == SCAN_RANK && live) { ref = a.xy[tok]; y = a.labels[tok]; }
    if (OP == SCAN_COLLECT && live) ref = a.tau[tok];
    unsigned n_before = 0;         // RANK
    float cm[16];                  // CLASSMAX
#pragma unroll
    for (int t = 0; t < 16; ++t) cm[t] = -INFINITY;

    int xn = 0x7fffffff, xq = 0x7fffffff, xp = 0;     // EX: cursor (next excluded id, the one after it, index of the latter)
    const int32_t *xl = nullptr;
    if constexpr (EX) {
        if (live) {
            // first list entry at or past this part's first row (entries after the last id are -1)
            xl = vce_ex(a).excl + tok * vce_ex(a).ld_e;
            const int lo = vt0 * 128;
            int p = 0, n = vce_ex(a).E;
            while (n > 0) {
                const int half = n >> 1, v = xl[p + half];
                if (v >= 0 && v < lo) { p += half + 1; n -= half + 1; } else n = half;
            }
            const int v0 = p < vce_ex(a).E ? xl[p] : -1, v1 = p + 1 < vce_ex(a).E ? xl[p + 1] : -1;
            xn = v0 < 0 ? 0x7fffffff : v0;
            xq = v1 < 0 ? 0x7fffffff : v1;
            xp = p + 1;
        }
    }
    // EX: NaN into the lane's excluded entries of the half-tile (vt, vhe) whose MFMA chain has just completed in acc
    auto excl = [&](f32x16 (&acc)[2], int vt, int vhe) __attribute__((always_inline)) {
        if constexpr (EX) {
            const int base = vt * 128 + vhe * 64, hi = base + 64;
            if (__any(xn < hi)) {
                unsigned m = 0;
                while (xn < hi) {
                    const int o = xn - base;          // negative: an id of the half-tile this wave does not score (NH = 1)
                    if (o >= 0 && ((o >> 2) & 1) == hf) m |= 1u << ((o >> 5) * 16 + (o & 3) + 4 * ((o >> 3) & 3));
                    xn = xq;
                    ++xp;
                    const int v = xp < vce_ex(a).E ? xl[xp] : -1;
                    xq = v < 0 ? 0x7fffffff : v;
                }
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int t = 0; t < 16; ++t)
                        if ((m >> (rt * 16 + t)) & 1u) acc[rt][t] = __builtin_nanf("");
            }
        }
    };

    float breg = 0.f;
    auto fetch = [&](int vt, int buf) {
        VTile<KD>::template dma<512>(a.wt, a.ld_w, (int64_t)vt * 128, vt < vt1 ? a.V : 0, smem + buf * TILE_B, tid);
        if (tid < 128) {
            const int v = vt * 128 + tid;
            breg = (vt < vt1 && v < a.V) ? (a.bias ? a.bias[v] : 0.f) : -INFINITY;   // rows past V: score = -inf
        }
    };
    fetch(vt0, 0);
    if (tid < 128) sBias[tid] = breg;
    VCE_DMA_WAIT();
    __syncthreads();

    // One half-tile (64 vocabulary rows x the wave's 32 tokens) = 16 MFMAs into acc, then ~4 VALU instructions per entry
    // on the result.  A VALU wave-instruction holds the SIMD's issue port for 4 cycles, an MFMA for 8 of its 32: run one
    // after the other the two phases add up (measured: matrix pipe 36 % busy, VALU issue 43 %, sum 79 % of the kernel's
    // cycles); interleaved -- the MFMA chain of one half-tile issued between the VALU instructions of the previous one --
    // they overlap.  So the loop is software-pipelined by half a tile: `scores` of half-tile i runs inside the instruction
    // stream of `chain` of half-tile i + 1 (sched_group_barrier pins the interleave), on two accumulator sets.
    // one entry of a half-tile's scores: x = accumulator + bias (the bias last, as the materialising GEMM adds it; rows past
    // V: -inf); RANK: count it if it beats x_y, note an equal one; CLASSMAX: the running maximum of its accumulator slot;
    // COLLECT: note one that reaches tau
    bool hot = false;
    auto entry = [&](f32x16 (&acc)[2], int rt, int t, float bj) __attribute__((always_inline)) {
        const float x = acc[rt][t] + bj;
        acc[rt][t] = x;
        if (OP == SCAN_RANK) {
            n_before += x > ref ? 1u : 0u;
            hot |= x == ref;
        } else if (OP == SCAN_CLASSMAX) {
            cm[t] = fmaxf(cm[t], x);
        } else {
            hot |= x >= ref;
        }
    };
    // The 16 MFMAs of a half-tile's chain into accN, and -- WITH = true -- between them the scores of the half-tile before
    // it (accP: 32 entries per lane, two per MFMA).  sched_barrier(0) after every MFMA's group pins the interleave (left to
    // itself, or to sched_group_barrier, the compiler issues the sixteen MFMAs first and the VALU after them).
    auto chain = [&](auto WITH, f32x16 (&accN)[2], const char *w, f32x16 (&accP)[2], const float *bs, int vhe) __attribute__((always_inline)) {
        constexpr bool with = decltype(WITH)::value;
        bf16x8 wfq[NKS];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int t = 0; t < 16; ++t) accN[rt][t] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) wfq[ks] = *reinterpret_cast<const bf16x8 *>(w + foff[ks]);
        hot = false;
        // the eight bias quads of the previous half-tile are requested up front, with the first fragments: a quad requested
        // where it is used parks the wave for a full LDS round trip (~130 cycles) sixteen times per tile
        f32x4 bq[8];
        if (with) {
#pragma unroll
            for (int q = 0; q < 8; ++q) bq[q] = *reinterpret_cast<const f32x4 *>(bs + vhe * 64 + (q >> 2) * 32 + 8 * (q & 3) + 4 * hf);
        }
#pragma unroll
        for (int i = 0; i < 2 * NKS; ++i) {
            const int rt = i / NKS, ks = i % NKS;
            __builtin_amdgcn_sched_barrier(0);
            accN[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfq[ks], hfr[ks], accN[rt], 0, 0, 0);
            if (rt == 0) wfq[ks] = *reinterpret_cast<const bf16x8 *>(w + 32 * STR + foff[ks]);
            if (with) {
                // entries 2 i, 2 i + 1 of the previous half-tile (NKS = 8: all 32; NKS = 4: the rest follows the chain)
#pragma unroll
                for (int e = 2 * i; e < 2 * i + 2; ++e) entry(accP, e >> 4, e & 15, bq[e >> 2][e & 3]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (with && NKS < 8) {
#pragma unroll
            for (int e = 4 * NKS; e < 32; ++e) entry(accP, e >> 4, e & 15, bq[e >> 2][e & 3]);
        }
    };
    // the scores of a half-tile on their own (NH = 1; the last half-tile of NH = 2)
    auto scores = [&](f32x16 (&acc)[2], const float *bs, int vhe) __attribute__((always_inline)) {
        hot = false;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bs + vhe * 64 + rt * 32 + 8 * tq + 4 * hf);
#pragma unroll
                for (int k = 0; k < 4; ++k) entry(acc, rt, 4 * tq + k, b4[k]);
            }
    };
    auto rare = [&](f32x16 (&acc)[2], int vt, int vhe) __attribute__((always_inline)) {       // the half-tile that holds the label / a candidate
        const int row0 = vt * 128 + vhe * 64 + 4 * hf;
        int slot = 0;
        if (OP == SCAN_COLLECT) {          // the lane's candidates of this half-tile take consecutive slots: one atomic
            int n = 0;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int t = 0; t < 16; ++t)
                    n += (acc[rt][t] >= ref && row0 + rt * 32 + (t & 3) + 8 * (t >> 2) < a.V) ? 1 : 0;
            if (n) slot = atomicAdd(a.cnt + tok, n);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int j = row0 + rt * 32 + (t & 3) + 8 * (t >> 2);
                const float x = acc[rt][t];
                if (OP == SCAN_RANK) {
                    n_before += (x == ref && j < y) ? 1u : 0u;        // ties: the lower index ranks first
                } else if (x >= ref && j < a.V) {
                    if (slot < VCE_CAND) {
                        a.cand_v[tok * VCE_CAND + slot] = x;
                        a.cand_i[tok * VCE_CAND + slot] = j;
                    }
                    ++slot;
                }
            }
    };
    f32x16 accA[2], accB[2];
    int vt_prev = vt0;
    bool have_prev = false;
    int bcur = 0, bprev = 2;           // bias ring slots of this tile and of the previous one; the next one's goes to the third
#ifdef VCE_SCAN_STAMPS
    unsigned long long st_[6] = {0, 0, 0, 0, 0, 0}, t0_ = __builtin_amdgcn_s_memtime();
#endif
    constexpr std::integral_constant<bool, true> YES{};
    constexpr std::integral_constant<bool, false> NO{};
    auto tile = [&](auto BUF, int vt) __attribute__((always_inline)) {
        constexpr int buf = decltype(BUF)::value;
        VCE_STAMP(5);
        fetch(vt + 1, buf ^ 1);
        VCE_STAMP(0);
        const char *w = smem + buf * TILE_B;
        const int bnext = 3 - bcur - bprev;
        if (NH == 2) {
            // accA <- half 0 of this tile, beside the scores of the previous tile's half 1 (accB)
            if (have_prev) {
                chain(YES, accA, w, accB, sBias + bprev * 128, 1);
                if (OP != SCAN_CLASSMAX && __any(hot)) rare(accB, vt_prev, 1);
            } else {
                chain(NO, accA, w, accB, sBias, 0);
            }
            excl(accA, vt, 0);
            VCE_STAMP(1);
            // accB <- half 1, beside the scores of half 0
            chain(YES, accB, w + 64 * STR, accA, sBias + bcur * 128, 0);
            if (OP != SCAN_CLASSMAX && __any(hot)) rare(accA, vt, 0);
            excl(accB, vt, 1);
            VCE_STAMP(2);
            have_prev = true;
            vt_prev = vt;
        } else {
            chain(NO, accA, w, accB, sBias, 0);
            excl(accA, vt, vh);
            scores(accA, sBias + bcur * 128, vh);
            if (OP != SCAN_CLASSMAX && __any(hot)) rare(accA, vt, vh);
        }
        if (tid < 128) sBias[bnext * 128 + tid] = breg;
        bprev = bcur;
        bcur = bnext;
        VCE_DMA_WAIT();
        VCE_STAMP(3);
        B4C_LDS_BARRIER();
        VCE_STAMP(4);
    };
    for (int vt = vt0; vt < vt1; vt += 2) {
        tile(std::integral_constant<int, 0>{}, vt);
        if (vt + 1 < vt1) tile(std::integral_constant<int, 1>{}, vt + 1);
    }
    if (NH == 2 && have_prev) {          // the last half-tile's scores
        scores(accB, sBias + bprev * 128, 1);
        if (OP != SCAN_CLASSMAX && __any(hot)) rare(accB, vt_prev, 1);
    }
#ifdef VCE_SCAN_STAMPS
    if (lane == 0 && blockIdx.x < 2048)
        for (int k = 0; k < 6; ++k) g_vce_stamps[(blockIdx.x * 8 + wave) * 6 + k] = st_[k];
#endif
    if (!live) return;
    if (OP == SCAN_RANK) {
        if (n_before) atomicAdd(a.rank + tok, (int)n_before);          // integer adds: any order gives the same count
    } else if (OP == SCAN_CLASSMAX) {
        // sub-list index: (part, half of the tile, lane half) for NH = 1; (part, lane half) for NH = 2 (a.nsub_per_part of them)
        const int sub = NH == 2 ? part * 2 + hf : part * 4 + vh * 2 + hf;
        float *o = a.cm + ((int64_t)sub * a.R + tok) * 16;
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) *reinterpret_cast<f32x4 *>(o + 4 * tq) = (f32x4){cm[4 * tq], cm[4 * tq + 1], cm[4 * tq + 2], cm[4 * tq + 3]};
    }
