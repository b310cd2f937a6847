// Body of cand_score_kernel / cand_rank_rows_kernel (candidates.hip), included inside each kernel after the row's list is in
// LDS: sv[p] / si[p] (p < C) the score and id of list position p (si -1: absent), sy the label's score, y the label (-1: none).
// One wave per row (the workgroup); rank, then the k selection rounds, which take the ids they hand out out of si.
// A duplicated id counts once in the rank, at its first position: hk / hp (2^hb slots each, rank != NULL only) hold every
// listed id and the smallest position it sits at (atomicCAS for the key, atomicMin for the position).
    if (rank) {
        int cnt = 0;
        if (y >= 0) {
            const int hm = (1 << hb) - 1;
            for (int i = lane; i <= hm; i += 64) { hk[i] = -1; hp[i] = 0x7fffffff; }
            __syncthreads();
            for (int p = lane; p < C; p += 64) {
                const int c = si[p];
                if (c < 0) continue;
                int s = sampler_hash_slot(c, hb);
                for (;;) {
                    const int old = atomicCAS(&hk[s], -1, c);
                    if (old == -1 || old == c) break;
                    s = (s + 1) & hm;
                }
                atomicMin(&hp[s], p);
            }
            __syncthreads();
            for (int p = lane; p < C; p += 64) {
                const int c = si[p];
                if (c < 0 || c == y) continue;
                const float s = sv[p];
                if (s > sy || (s == sy && c < y)) {
                    int t = sampler_hash_slot(c, hb);
                    while (hk[t] != c) t = (t + 1) & hm;
                    cnt += hp[t] == p ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) rank[row] = y >= 0 ? cnt : -1;
    }
    if (idx) {
        for (int kk = 0; kk < k; ++kk) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int p = lane; p < C; p += 64) {
                const int c = si[p];
                if (c >= 0 && cand_better(sv[p], c, bv, bi)) { bv = sv[p]; bi = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) idx[row * k + kk] = bi == 0x7fffffff ? -1 : bi;
            if (bi != 0x7fffffff)
                for (int p = lane; p < C; p += 64)
                    if (si[p] == bi) si[p] = -1;        // every copy of the id handed out leaves the list
            __syncthreads();
        }
    }
