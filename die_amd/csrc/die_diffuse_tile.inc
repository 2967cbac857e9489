// The body of an LDS-tiled separable gaussian kernel on the torus (die_diffuse.h): the (TX+2R)×(TY+2R) input tile is staged once,
// filtered along x (axis 0, as scipy does first) into a second LDS plane, then along y.  Included inside a kernel of DIE_BLOCK
// threads that has in scope: the type T of a cell, the radius R (constant expressions), `DiffuseArgs a`, and the macro
// DIF_LOAD(src, i) — cell i of the plane `src` (a.src as const T*) as the filter is to see it.  A kernel that does something
// else with a finished cell than store it defines DIF_STORE(dst, i, v) — a statement given the output plane, the cell and its value —
// ahead of the include; left undefined it is the plain store, token for token the statement that stood here before the hook.
#ifndef DIF_STORE
#define DIF_STORE(dst, i, v) die_st(dst, i, v);
#define DIF_STORE_IS_DEFAULT
#endif
    constexpr int LW = DIF_TY + 2 * R + 1;    // odd pitch: bank-conflict-free column walks
    constexpr int LH = DIF_TX + 2 * R;
    __shared__ float s_in[LH * LW];
    __shared__ float s_mid[DIF_TX * LW];
    const T* src = (const T*)a.src;
    T* dst = (T*)a.dst;
    const int x0 = blockIdx.y * DIF_TX, y0 = blockIdx.x * DIF_TY;
    const int H = a.H, W = a.W;
    constexpr int LWV = DIF_TY + 2 * R;       // valid columns
    for (int idx = threadIdx.x; idx < LH * LWV; idx += DIE_BLOCK) {
        const int li = idx / LWV, lj = idx - li * LWV;
        const int gx = edge_idx(x0 - R + li, W, a.mode), gy = edge_idx(y0 - R + lj, H, a.mode);
        s_in[li * LW + lj] = (gx < 0 || gy < 0) ? 0.f : DIF_LOAD(src, (int64_t)gx * H + gy);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < DIF_TX * LWV; idx += DIE_BLOCK) {
        const int i = idx / LWV, j = idx - i * LWV;
        float t = a.w[R] * s_in[(i + R) * LW + j];            // scipy's correlate1d on a symmetric kernel: the centre, then
#pragma unroll
        for (int k = 0; k < R; ++k) t += (s_in[(i + k) * LW + j] + s_in[(i + 2 * R - k) * LW + j]) * a.w[k];   // pairs, outermost first
        s_mid[i * LW + j] = t;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < DIF_TX * DIF_TY; idx += DIE_BLOCK) {
        const int i = idx / DIF_TY, j = idx - i * DIF_TY;
        const int gx = x0 + i, gy = y0 + j;
        if (gx < W && gy < H) {
            float o = a.w[R] * s_mid[i * LW + j + R];
#pragma unroll
            for (int k = 0; k < R; ++k) o += (s_mid[i * LW + j + k] + s_mid[i * LW + j + 2 * R - k]) * a.w[k];
            DIF_STORE(dst, (int64_t)gx * H + gy, o * a.keep)
        }
    }
#ifdef DIF_STORE_IS_DEFAULT
#undef DIF_STORE
#undef DIF_STORE_IS_DEFAULT
#endif
