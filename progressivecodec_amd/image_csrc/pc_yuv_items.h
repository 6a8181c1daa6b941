// pc_yuv_items.h -- the work items the YUV 4:2:0 libraries share, as __device__ templates; what differs per caller is a compile-time
// policy or an argument, never a branch on the caller.  The __global__ kernels, their launch bounds, grids and parameter lists stay
// in each library's own .hip file.
//   cut_item       eight luma columns of one row -> float32 R, G, B (the ingest of DESIGN.md section 13): frames, frame_tiles, clips
//   compare_tile   a tile's footprint in two frames, row pair by eight columns, and its halo ring: clips (count), clip_tol (count,
//                  sse, maxabs); the policy Acc says what one sample pair adds
//   sse_tile       a decoded float tile against a frame in the frame's codes, band-weighted (section 15): frame_rate, clip_rate
// An item whose samples all lie inside the frame and whose accesses are all wide is compiled on its own (FULL, or the WIDE branch of
// cut_item); every other item goes element by element.  The access path only changes the load and store instructions, never which
// thread holds which sample or in which order it adds.  Include after pc_yuv_device.h, pc_tile_grid.h and pc_reduce.h.
#ifndef PC_YUV_ITEMS_H
#define PC_YUV_ITEMS_H

namespace {

// The item space of a tile taken row pair by eight columns: T * T / 16 items, NT to a block (a multiple of NT for every T that is a
// multiple of 64: no block straddles two tiles and none has a tail), and `extra` more blocks per tile (the halo ring's).  Blocks per
// tile without the extra ones and blocks in all; false for what the calls refuse.
bool pair_blocks_of(int T, int n_tiles, int t_max, int extra, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > t_max || n_tiles < 1) return false;
    bpt = (int)((int64_t)T * T / (2 * COLS * NT));
    blocks = (int64_t)n_tiles * (bpt + extra);
    return blocks <= INT32_MAX;
}

// eight floats to d: two 128-bit words, or the first n one by one
template <bool WIDE>
__device__ __forceinline__ void store8(float* d, const float (&o)[COLS], int n)
{
    if (WIDE) {
        *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
        for (int i = 0; i < COLS; ++i)
            if (i < n) d[i] = o[i];
    }
}

// -- cut -----------------------------------------------------------------------------------------------------------------------------

// Luma row y (0 <= y < H) and columns x0 .. x0+7 of one picture -> o[R, G, B][column]; a column outside [0, W) is left as it is.
// SH: the bits below the code in an element (P010: 6).  The chroma taps are clamped at the picture's edges Hc - 1, Wc - 1.  PAD: x0
// may be negative (the padded planes of the ingest); else 0 <= x0 < W.  WIDE needs x0 a multiple of 8: x0 / 2 is then one of 4.
template <class T, bool IL, bool WIDE, bool PAD>
__device__ __forceinline__ void cut_item(const Planes<const T>& s, int W, int Hc, int Wc, int y, int x0, int linear, const Levels& lv,
                                         const IngestCoef& k, float (&o)[3][COLS])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    const int i0 = y >> 1;
    const int i1 = clampi(i0 + ((y & 1) ? 1 : -1), 0, Hc - 1);
    const T* yrow = s.y + (int64_t)y * s.yr;
    const T* u0 = s.u + (int64_t)i0 * s.ur;                       // Cb of chroma row i0, i1; Cr: one element on, or the V plane
    const T* u1 = s.u + (int64_t)i1 * s.ur;
    const T* v0 = IL ? u0 + 1 : s.v + (int64_t)i0 * s.vr;
    const T* v1 = IL ? u1 + 1 : s.v + (int64_t)i1 * s.vr;
    if (WIDE && (!PAD || x0 >= 0) && x0 + COLS - 1 < W) {
        unsigned Yc[COLS];
        load4(yrow + x0, Yc);
        load4(yrow + x0 + 4, Yc + 4);
        const int jc = x0 >> 1;                                    // chroma columns jc .. jc+3 exist; a multiple of 4
        const int jl = max(jc - 1, 0), jr = min(jc + 4, Wc - 1);
        unsigned cw[2][2][6];                                      // [row i0, i1][Cb, Cr][columns jl, jc .. jc+3, jr]
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const T* pu = rr ? u1 : u0;
            const T* pv = rr ? v1 : v0;
            if (rr == 1 && !linear) {
#pragma unroll
                for (int j = 0; j < 6; ++j) { cw[1][0][j] = cw[0][0][j]; cw[1][1][j] = cw[0][1][j]; }
                break;
            }
            if (IL) {
                unsigned e[8];
                load4(pu + 2 * (int64_t)jc, e);
                load4(pu + 2 * (int64_t)jc + 4, e + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { cw[rr][0][1 + j] = e[2 * j]; cw[rr][1][1 + j] = e[2 * j + 1]; }
            } else {
                load4(pu + jc, &cw[rr][0][1]);
                load4(pv + jc, &cw[rr][1][1]);
            }
            cw[rr][0][0] = pu[CS * (int64_t)jl]; cw[rr][1][0] = pv[CS * (int64_t)jl];
            cw[rr][0][5] = pu[CS * (int64_t)jr]; cw[rr][1][5] = pv[CS * (int64_t)jr];
        }
#pragma unroll
        for (int i = 0; i < COLS; ++i) {
            const int j0 = 1 + (i >> 1), j1 = (i & 1) ? j0 + 1 : j0 - 1;
            int c16[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int c00 = (int)(cw[0][p][j0] >> SH), c01 = (int)(cw[0][p][j1] >> SH);
                const int c10 = (int)(cw[1][p][j0] >> SH), c11 = (int)(cw[1][p][j1] >> SH);
                c16[p] = linear ? 9 * c00 + 3 * c01 + 3 * c10 + c11 : 16 * c00;
            }
            to_rgb((int)(Yc[i] >> SH), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
        }
    } else {                                                      // element by element; also the items that straddle an edge
#pragma unroll
        for (int i = 0; i < COLS; ++i) {
            const int x = x0 + i;
            if ((!PAD || x >= 0) && x < W) {
                const int64_t j0 = x >> 1;
                const int64_t j1 = clampi((int)j0 + ((x & 1) ? 1 : -1), 0, Wc - 1);
                int c16[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const T* r0 = p ? v0 : u0;
                    const T* r1 = p ? v1 : u1;
                    const int c00 = (int)(r0[CS * j0] >> SH);
                    if (linear) {
                        const int c01 = (int)(r0[CS * j1] >> SH), c10 = (int)(r1[CS * j0] >> SH), c11 = (int)(r1[CS * j1] >> SH);
                        c16[p] = 9 * c00 + 3 * c01 + 3 * c10 + c11;
                    } else {
                        c16[p] = 16 * c00;
                    }
                }
                to_rgb((int)(yrow[x] >> SH), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
            }
        }
    }
}

// -- compare -------------------------------------------------------------------------------------------------------------------------

// One item: luma rows Y, Y + 1 and columns X .. X+7 of the frame (both even), of which `rows` rows and the lanes 0 .. hi-1 lie
// inside the tile's part of the frame (rows is 1 or 2, 1 <= hi <= 8), and the chroma samples (Y / 2, X / 2 + m), 2m < hi.
// FULL: rows == 2, hi == 8 and every access is wide; else element by element.  A lane outside is 0 in both frames: it adds nothing.
// Acc::take<SH>(a, b, p, ac): one sample pair of plane p (elements, the code is element >> SH) into the thread's Acc::N numbers.
template <class T, bool IL, bool FULL, class Acc>
__device__ __forceinline__ void compare_item(const Planes<const T>& a, const Planes<const T>& b, int64_t Y, int64_t X, int rows, int hi,
                                             unsigned (&ac)[Acc::N])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (FULL || r < rows) {
            const T* pa = a.y + (Y + r) * a.yr + X;
            const T* pb = b.y + (Y + r) * b.yr + X;
            unsigned wa[COLS], wb[COLS];
            if (FULL) {
                load4(pa, wa);
                load4(pa + 4, wa + 4);
                load4(pb, wb);
                load4(pb + 4, wb + 4);
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) {
                    wa[q] = q < hi ? (unsigned)pa[q] : 0u;
                    wb[q] = q < hi ? (unsigned)pb[q] : 0u;
                }
            }
#pragma unroll
            for (int q = 0; q < COLS; ++q) Acc::template take<SH>(wa[q], wb[q], 0, ac);
        }
    }
    const int64_t ci = Y >> 1, cx0 = X >> 1;
    const T* ua = a.u + ci * a.ur + CS * cx0;
    const T* va = IL ? ua + 1 : a.v + ci * a.vr + cx0;
    const T* ub = b.u + ci * b.ur + CS * cx0;
    const T* vb = IL ? ub + 1 : b.v + ci * b.vr + cx0;
    unsigned ca[2][4], cb[2][4];                                  // [Cb, Cr][sample]
    if (FULL) {
        if (IL) {
            unsigned ea[8], eb[8];
            load4(ua, ea);
            load4(ua + 4, ea + 4);
            load4(ub, eb);
            load4(ub + 4, eb + 4);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                ca[0][m] = ea[2 * m]; ca[1][m] = ea[2 * m + 1];
                cb[0][m] = eb[2 * m]; cb[1][m] = eb[2 * m + 1];
            }
        } else {
            load4(ua, ca[0]);
            load4(va, ca[1]);
            load4(ub, cb[0]);
            load4(vb, cb[1]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bool in = 2 * m < hi;
            ca[0][m] = in ? (unsigned)ua[CS * m] : 0u;
            ca[1][m] = in ? (unsigned)va[CS * m] : 0u;
            cb[0][m] = in ? (unsigned)ub[CS * m] : 0u;
            cb[1][m] = in ? (unsigned)vb[CS * m] : 0u;
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        Acc::template take<SH>(ca[0][m], cb[0][m], 1, ac);
        Acc::template take<SH>(ca[1][m], cb[1][m], 2, ac);
    }
}

// A block's share of tile `tile` of the grid, frames a against b.  Blocks bl = 0 .. bpt - 1 of a tile hold its items: item ->
// (row pair kp, group g), tile rows 2 kp and 2 kp + 1, tile columns 8g .. 8g+7 (G8 = T / 8); S and T are even, so a tile's cells are
// the frame's, and the items cover the tile's luma and the chroma rectangle WITHOUT the halo exactly once.  Block bl = bpt holds the
// halo ring -- the chroma row above and below and the column left and right of that rectangle, where the frame has them and `halo`
// is set -- element by element (2 T + 4 samples at most).
template <class T, bool IL, bool WIDE, class Acc>
__device__ __forceinline__ void compare_tile(const Planes<const T>& a, const Planes<const T>& b, const Grid& gr, int tile, int bl, int bpt,
                                             int G8, int halo, unsigned (&ac)[Acc::N])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;
    const int i = tile / gr.nx, j = tile - i * gr.nx;
    const int Yt = i * gr.S, Xt = j * gr.S;                       // the tile's first row and column in the frame: < H, < W
    const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
    if (bl < bpt) {
        const int rem = bl * NT + (int)threadIdx.x;               // < T * T / 16 <= 2^18
        const int kp = rem / G8, r0 = 2 * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            const int rows = r0 + 1 < hh ? 2 : 1, hi = min(COLS, ww - q0);
            if (WIDE && rows == 2 && hi == COLS)
                compare_item<T, IL, true, Acc>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ac);
            else
                compare_item<T, IL, false, Acc>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ac);
        }
    } else if (halo) {
        // the chroma rectangle the items covered: rows r0c .. r1c, columns c0c .. c1c; the ring around it where the frame has it
        const int Hc = (gr.H + 1) >> 1, Wc = (gr.W + 1) >> 1;
        const int r0c = Yt >> 1, r1c = r0c + ((hh + 1) >> 1) - 1, c0c = Xt >> 1, c1c = c0c + ((ww + 1) >> 1) - 1;
        const bool top = r0c > 0, bottom = r1c < Hc - 1, left = c0c > 0, right = c1c < Wc - 1;
        const int cf = c0c - (left ? 1 : 0), nw = c1c + (right ? 1 : 0) - cf + 1, nh = r1c - r0c + 1;
        for (int idx = (int)threadIdx.x; idx < 2 * nw + 2 * nh; idx += NT) {
            int row, col;
            bool on;
            if (idx < nw) { row = r0c - 1; col = cf + idx; on = top; }
            else if (idx < 2 * nw) { row = r1c + 1; col = cf + idx - nw; on = bottom; }
            else if (idx < 2 * nw + nh) { row = r0c + idx - 2 * nw; col = c0c - 1; on = left; }
            else { row = r0c + idx - 2 * nw - nh; col = c1c + 1; on = right; }
            if (on) {                                              // 0 <= row < Hc and 0 <= col < Wc
                const int64_t oa = (int64_t)row * a.ur + CS * (int64_t)col, ob = (int64_t)row * b.ur + CS * (int64_t)col;
                const T* va = IL ? a.u + oa + 1 : a.v + (int64_t)row * a.vr + col;
                const T* vb = IL ? b.u + ob + 1 : b.v + (int64_t)row * b.vr + col;
                Acc::template take<SH>((unsigned)a.u[oa], (unsigned)b.u[ob], 1, ac);
                Acc::template take<SH>((unsigned)*va, (unsigned)*vb, 2, ac);
            }
        }
    }
}

// -- sse -----------------------------------------------------------------------------------------------------------------------------

// One item: rows r0, r0 + 1 and columns q0 .. q0+7 of the tile at xt, of which `rows` rows and the lanes 0 .. hi-1 lie inside the
// frame (rows is 1 or 2, 1 <= hi <= 8); Y, X: the frame position of (r0, q0), both even.  FULL: rows == 2, hi == 8 and every access
// is wide; else element by element, a row or column beyond the frame standing in as the last one inside it (section 13's edge cells).
// ay[2], ax[8]: the band numerators of the item's rows and columns, whether inside the frame or not.
template <class T, bool IL, bool FULL>
__device__ __forceinline__ void sse_item(const float* xt, int64_t sc, int64_t sh, int r0, int q0, int rows, int hi,
                                         const Planes<const T>& ref, int64_t Y, int64_t X, const Levels& lv, const EmitCoef& k,
                                         const unsigned ay[2], const unsigned ax[COLS], u64 su[3])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    unsigned yq[2][COLS];
    float ub[2][COLS], ur[2][COLS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        float v[3][COLS];
        const int rr = FULL ? r : min(r, rows - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            // r0 + 1 < T <= sh and q0 + 7 < T: the row pair and the eight floats lie inside the tile whatever the frame's edge
            const float* s = xt + ch * sc + (int64_t)(r0 + rr) * sh + q0;
            if (FULL) {
                const float4 f0 = *reinterpret_cast<const float4*>(s), f1 = *reinterpret_cast<const float4*>(s + 4);
                v[ch][0] = f0.x; v[ch][1] = f0.y; v[ch][2] = f0.z; v[ch][3] = f0.w;
                v[ch][4] = f1.x; v[ch][5] = f1.y; v[ch][6] = f1.z; v[ch][7] = f1.w;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) v[ch][q] = s[min(q, hi - 1)];
            }
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(v[0][q], v[1][q], v[2][q], lv, k, yq[r][q], ub[r][q], ur[r][q]);
    }
    // luma
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (FULL || r < rows) {
            const T* p = ref.y + (Y + r) * ref.yr + X;
            unsigned w[COLS];
            if (FULL) {
                load4(p, w);
                load4(p + 4, w + 4);
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) w[q] = q < hi ? (unsigned)p[q] : 0u;
            }
            u64 row = 0ull;                                        // each term < 2^11 * 2^20
#pragma unroll
            for (int q = 0; q < COLS; ++q) {
                if (FULL || q < hi) {
                    const int e = (int)yq[r][q] - (int)(w[q] >> SH);
                    row += (u64)(ax[q] * (unsigned)(e * e));
                }
            }
            su[0] += (u64)ay[r] * row;
        }
    }
    // chroma: the frame's sample (Y / 2, X / 2 + m) is the mean of the tile's cell (r0 / 2, q0 / 2 + m)
    const int64_t ci = Y >> 1, cx0 = X >> 1;
    const T* pu = ref.u + ci * ref.ur + CS * cx0;
    const T* pv = IL ? pu + 1 : ref.v + ci * ref.vr + cx0;
    unsigned w[2][4];
    if (FULL) {
        if (IL) {
            unsigned e[8];
            load4(pu, e);
            load4(pu + 4, e + 4);
#pragma unroll
            for (int m = 0; m < 4; ++m) { w[0][m] = e[2 * m]; w[1][m] = e[2 * m + 1]; }
        } else {
            load4(pu, w[0]);
            load4(pv, w[1]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bool in = 2 * m < hi;
            w[0][m] = in ? (unsigned)pu[CS * m] : 0u;
            w[1][m] = in ? (unsigned)pv[CS * m] : 0u;
        }
    }
    const u64 cy = (u64)((ay[0] + ay[1]) >> 1);
    u64 sb = 0ull, sr = 0ull;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (FULL || 2 * m < hi) {
            const int eb = emit_chroma(ub[0][2 * m], ub[0][2 * m + 1], ub[1][2 * m], ub[1][2 * m + 1], lv) - (int)(w[0][m] >> SH);
            const int er = emit_chroma(ur[0][2 * m], ur[0][2 * m + 1], ur[1][2 * m], ur[1][2 * m + 1], lv) - (int)(w[1][m] >> SH);
            const unsigned cx = (ax[2 * m] + ax[2 * m + 1]) >> 1;
            sb += (u64)(cx * (unsigned)(eb * eb));
            sr += (u64)(cx * (unsigned)(er * er));
        }
    }
    su[1] += cy * sb;
    su[2] += cy * sr;
}

// Block b's share of tile `tile` of the grid, the float tile at xt against the frame ref: the items b * NT .. of the tile, item ->
// (row pair kp, group g), tile rows 2 kp and 2 kp + 1, tile columns 8g .. 8g+7 (G8 = T / 8).
template <class T, bool IL, bool WIDE>
__device__ __forceinline__ void sse_tile(const float* xt, int64_t sc, int64_t sh, const Planes<const T>& ref, const Grid& gr, int tile,
                                         int b, int G8, const Levels& lv, const EmitCoef& k, u64 su[3])
{
    const int i = tile / gr.nx, j = tile - i * gr.nx;
    const int S = gr.S, O = gr.O, den = O > 0 ? 2 * O : 1;
    const int Yt = i * S, Xt = j * S;                             // the tile's first row and column in the frame: < H, < W
    const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
    const int rem = b * NT + (int)threadIdx.x;                    // < T * T / 16 <= 2^18
    const int kp = rem / G8, r0 = 2 * kp, q0 = COLS * (rem - kp * G8);
    if (r0 < hh && q0 < ww) {
        const int rows = r0 + 1 < hh ? 2 : 1, hi = min(COLS, ww - q0);
        unsigned ay[2], ax[COLS];
#pragma unroll
        for (int r = 0; r < 2; ++r) ay[r] = axis_weight(i, gr.ny, r0 + r, S, O, den);
#pragma unroll
        for (int q = 0; q < COLS; ++q) ax[q] = axis_weight(j, gr.nx, q0 + q, S, O, den);
        if (WIDE && rows == 2 && hi == COLS)
            sse_item<T, IL, true>(xt, sc, sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, lv, k, ay, ax, su);
        else
            sse_item<T, IL, false>(xt, sc, sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, lv, k, ay, ax, su);
    }
}

}  // namespace

#endif  // PC_YUV_ITEMS_H
