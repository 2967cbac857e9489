// The sweep of a row-marching diffusion kernel (die_diffuse.h: one wave per strip of 248 columns, no LDS, no barrier).  Included inside
// a kernel of DIF_BLOCK threads that has in scope: T, R, FUSED, WRAP (constant expressions), `RowsArgs a` with src / dst / food
// already at this workgroup's plane, `row0` (the grid rows ahead of the field's), and the macro DIF_EMIT(off, v) — a statement that
// adds to the 4 cells v[] just read at plane offset `off` (a multiple of 4) what the filter is to see beside them, ahead of the
// deposits; empty for the plane as it is.  A kernel that does something else with a finished group of 4 outputs than store it defines
// DIF_STORE(dst, off, o) — a statement given the output plane, the group's plane offset and its 4 values — ahead of the include; left
// undefined it is the plain 16-byte store, token for token the statement that stood here before the hook.
#ifndef DIF_STORE
#define DIF_STORE(dst, off, o) Vec4<T>::st(dst + off, o);
#define DIF_STORE_IS_DEFAULT
#endif
    const T* src = (const T*)a.src;
    T* dst = (T*)a.dst;
    T* food = (T*)a.food;
    const int W = a.W, H = a.H;
    const int lane = threadIdx.x & (DIE_WAVE - 1);
    const int strip = blockIdx.x * (DIF_BLOCK / DIE_WAVE) + (threadIdx.x >> 6);
    const int yb = strip * DIF_WCOLS;                       // first output column of this wave
    if (yb >= H) return;                                    // whole wave idle (nothing below synchronises)
    const int nout = min(DIF_WCOLS, H - yb) / 4;            // output lanes are 1..nout (H % 4 == 0)
    const bool need = lane <= nout + 1;                     // + the two halo lanes
    const bool outl = lane >= 1 && lane <= nout;
    const bool wx = WRAP || a.wrapx, wy = WRAP || a.wrapy;
    const int hx = wx ? 0 : a.halo, hy = wy ? 0 : a.halo;
    const int col = wy ? wrap_idx(yb + 4 * (lane - 1), H)    // 16-byte aligned since H % 4 == 0
                       : min(max(yb + 4 * (lane - 1), 0), H - 4);     // tile: clamp, border ring is don't-care
    const int x0 = ((int)blockIdx.y - row0) * a.rpw;
    const int rows = min(a.rpw, W - x0);

    float win[2 * R + 1][4];
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) { win[k][0] = win[k][1] = win[k][2] = win[k][3] = 0.f; }

    auto load_row = [&](int i, float v[4]) {
        v[0] = v[1] = v[2] = v[3] = 0.f;
        if (!need) return;
        const int r = wx ? wrap_idx(x0 + i, W) : min(max(x0 + i, 0), W - 1);
        const int64_t off = (int64_t)r * H + col;
        Vec4<T>::ld(src + off, v);
        DIF_EMIT(off, v)
        if (FUSED) {
            bool occ[4];
            bool any = false;
            if (FUSED == 1) {
                const ulonglong2 c01 = *(const ulonglong2*)(a.claim + off), c23 = *(const ulonglong2*)(a.claim + off + 2);
                const unsigned long long c[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    occ[j] = die_claim_occupied(c[j], a.epoch);
                    if (occ[j]) v[j] = die_as_stored<T>(v[j] + die_claim_deposit(c[j]));     // chem[cell] + deposit of the last writer
                    any |= occ[j];
                }
            } else {
                const uint4 d4 = *(const uint4*)(a.dep + off);
                const uint32_t d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    occ[j] = d[j] != DIE_DEP_EMPTY;
                    if (occ[j]) v[j] = die_as_stored<T>(v[j] + __uint_as_float(d[j]));
                    any |= occ[j];
                }
            }
            // feeding: this wave owns rows [x0, x0+rows) × its output lanes (tile mode: interior cells only)
            const bool own_row = i >= 0 && i < rows && r >= hx && r < W - hx;
            if (any && outl && own_row && !a.food_infinite) {
                float f[4];
                Vec4<T>::ld(food + off, f);
                bool changed = false;                           // (an occupied cell without food stays as it is: a group in which nothing changes is not written)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool mine = col + j >= hy && col + j < H - hy;
                    if (occ[j] && mine && f[j] != 0.f) { f[j] = f[j] - a.rate_feed * f[j]; changed = true; }
                }
                if (changed) Vec4<T>::st(food + off, f);
            }
        }
    };

    float nxt[4];
    load_row(-R, nxt);
    for (int i = -R; i < rows + R; ++i) {
        float cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
        if (i + 1 < rows + R) load_row(i + 1, nxt);            // prefetch one row ahead
#pragma unroll
        for (int k = 0; k < 2 * R; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) win[k][j] = win[k + 1][j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) win[2 * R][j] = cur[j];
        const int orow = i - R;                                // the window is centred on this row
        if (orow < 0) continue;
        float xf[4 + 2 * 4];                                   // [4 − R .. 4 + 4 + R): own 4 at [4..8)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = a.w[R] * win[R][j];                      // centre, then symmetric pairs from the outermost inwards: mirror
#pragma unroll
            for (int k = 0; k < R; ++k) t += (win[k][j] + win[2 * R - k][j]) * a.w[k];      // cells get identical sums, as in scipy
            xf[4 + j] = t;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            xf[4 - R + j] = __shfl_up(xf[4 + 4 - R + j], 1, DIE_WAVE);      // left lane's last R cells
            xf[8 + j] = __shfl_down(xf[4 + j], 1, DIE_WAVE);                 // right lane's first R cells
        }
        if (outl) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = a.w[R] * xf[4 + j];
#pragma unroll
                for (int k = 0; k < R; ++k) t += (xf[4 + j - R + k] + xf[4 + j + R - k]) * a.w[k];
                o[j] = t * a.keep;
            }
            DIF_STORE(dst, (int64_t)(x0 + orow) * H + col, o)
        }
    }
#ifdef DIF_STORE_IS_DEFAULT
#undef DIF_STORE
#undef DIF_STORE_IS_DEFAULT
#endif
