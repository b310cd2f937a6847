// Body of topk_rows_kernel / topk_rows_excl_kernel (head.hip), included inside each kernel; EX: exclusion lists.
    __shared__ int sx[EX ? B4C_MAX_EXCL : 1];
    __shared__ int s_nx;
    __shared__ float cv[TOPK_CAP];
    __shared__ int ci[TOPK_CAP];
    __shared__ float mv[TOPK_THREADS];
    __shared__ int s_cnt;
    __shared__ float s_tv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = (V + 7) >> 3;
    for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
        const T *xr = x + row * ld;
        const int nx = topk_excl_stage<EX, TOPK_THREADS>(excl, ld_e, E, row, sx, &s_nx, tid);
        // pass 1: per-thread maximum (values only; fmaxf drops NaNs).  Four loads in flight per thread.
        float m = -INFINITY;
        for (int c0 = tid; c0 < nch; c0 += 4 * TOPK_THREADS) {
            float v[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * TOPK_THREADS;
                Vec8<T>::load(xr + (c < nch ? c : c0) * 8, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * TOPK_THREADS;
                if (EX && c < nch) {
                    const unsigned xm = topk_excl_bits(sx, nx, c);
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c * 8 + e < V && !((xm >> e) & 1u)) m = fmaxf(m, v[u][e]);
                } else if (c + 1 < nch) {           // whole chunk inside the row (the last chunk may hold pad columns)
#pragma unroll
                    for (int e = 0; e < 8; ++e) m = fmaxf(m, v[u][e]);
                } else if (c < nch) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c * 8 + e < V) m = fmaxf(m, v[u][e]);
                }
            }
        }
        mv[tid] = m;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        if (wave == 0) {
            // 64 maxima of disjoint element sets (lane l: threads l, l + 64, ...); the k-th largest of them is a lower
            // bound of the row's k-th largest value: at least k elements are >= it
            float g = mv[lane];
#pragma unroll
            for (int w = 1; w < TOPK_THREADS / 64; ++w) g = fmaxf(g, mv[lane + 64 * w]);
            const int rank = wave_rank(g, lane, 64);
            if (rank == k - 1) s_tv = g;      // ranks are a permutation of 0..63 (ties broken by lane)
        }
        __syncthreads();
        const float tv = s_tv;
        // Candidates = the elements >= tv.  A thread whose own maximum is below tv holds none, so only the few threads
        // with m >= tv (about k of the 512) read their chunks again: the row is NOT read a second time.
        if (m >= tv)
        for (int c0 = tid; c0 < nch; c0 += 4 * TOPK_THREADS) {
            float v[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * TOPK_THREADS;
                Vec8<T>::load(xr + (c < nch ? c : c0) * 8, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * TOPK_THREADS;
                const unsigned xm = (EX && c < nch) ? topk_excl_bits(sx, nx, c) : 0u;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int j = c * 8 + e;
                    if (c < nch && j < V && !((xm >> e) & 1u) && v[u][e] >= tv) {
                        const int pos = atomicAdd(&s_cnt, 1);
                        if (pos < TOPK_CAP) { cv[pos] = v[u][e]; ci[pos] = j; }
                    }
                }
            }
        }
        __syncthreads();
        topk_select(cv, ci, s_cnt, k, row, tid, lane, wave, topk_idx, labels, hit, ndcg, redo);
        __syncthreads();
    }
