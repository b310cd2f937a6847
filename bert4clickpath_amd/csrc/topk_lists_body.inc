// Body of topk_rows_lists_kernel / topk_rows_lists_excl_kernel (head.hip), included inside each kernel; EX: exclusion lists.
    __shared__ int sx[EX ? B4C_MAX_EXCL : 1];
    __shared__ int s_nx;
    __shared__ float lv[256][KM + 1];
    __shared__ int li[256][KM + 1];
    __shared__ float wv[4];
    __shared__ int wi[4], wo[4];
    __shared__ int s_owner;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = (V + 7) >> 3;
    for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
        if (redo && !redo[row]) continue;       // block-uniform: the threshold kernel has done this row
        const T *xr = x + row * ld;
        const int nx = topk_excl_stage<EX, 256>(excl, ld_e, E, row, sx, &s_nx, tid);
        float tv[KM];
        int ti[KM];
#pragma unroll
        for (int q = 0; q < KM; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
        for (int c = tid; c < nch; c += 256) {
            float v[8];
            Vec8<T>::load(xr + c * 8, v);
            const unsigned xm = EX ? topk_excl_bits(sx, nx, c) : 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = c * 8 + e;
                if (j < V && !((xm >> e) & 1u) && better(v[e], j, tv[KM - 1], ti[KM - 1])) {
                    tv[KM - 1] = v[e];
                    ti[KM - 1] = j;
#pragma unroll
                    for (int q = KM - 1; q > 0; --q) {
                        if (better(tv[q], ti[q], tv[q - 1], ti[q - 1])) {
                            const float fv = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = fv;
                            const int fi = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = fi;
                        }
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KM; ++q) { lv[tid][q] = tv[q]; li[tid][q] = ti[q]; }
        lv[tid][KM] = -INFINITY; li[tid][KM] = 0x7fffffff;
        int hp = 0;
        const int lab = labels ? labels[row] : -1;
        float h_acc = 0.f, n_acc = 0.f;
        for (int kk = 0; kk < k; ++kk) {
            float bv = lv[tid][hp];
            int bi = li[tid][hp], bo = tid;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o), oo = __shfl_xor(bo, o);
                if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; bo = oo; }
            }
            __syncthreads();
            if (lane == 0) { wv[wave] = bv; wi[wave] = bi; wo[wave] = bo; }
            __syncthreads();
            if (tid == 0) {
                float fv = wv[0]; int fi = wi[0], fo = wo[0];
                for (int w = 1; w < 4; ++w)
                    if (better(wv[w], wi[w], fv, fi)) { fv = wv[w]; fi = wi[w]; fo = wo[w]; }
                s_owner = fo;
                topk_idx[row * k + kk] = fi == 0x7fffffff ? -1 : fi;
                if (labels && fi == lab) {
                    h_acc += 1.f;
                    n_acc += 1.0f / (logf((float)(kk + 2)) / logf(2.0f));
                }
            }
            __syncthreads();
            if (tid == s_owner && hp < KM) ++hp;
        }
        if (tid == 0) {
            if (hit) hit[row] = h_acc;
            if (ndcg) ndcg[row] = n_acc;
        }
        __syncthreads();
    }
