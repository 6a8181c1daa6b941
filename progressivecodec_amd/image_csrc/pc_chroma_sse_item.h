// pc_chroma_sse_item.h -- the measuring item of the twelve YUV formats and three chroma sitings (DESIGN.md sections 24 and 28): SY
// rows of one decoded float tile by eight tile-aligned columns, rendered by section 21's emit with the tile's in-frame part as the
// picture and compared with the original frame's codes under the integer band weights.  pc_chroma_clip_rate.hip (a list of (frame,
// tile) jobs over a clip) includes it; pc_chroma_rate.hip (a linear range of tiles of one frame) still holds the text it was taken
// from, word for word, until the refactoring that deletes that copy (tests/test_chroma_clip_rate_host.py holds the two equal).  The
// __global__ kernels, their grids and every decision about the access path stay in each library's own .hip file.
//   Measure        what the measurement takes of the siting and the depth
//   weighted_row   one row of an item -> its horizontally filtered chroma differences and its weighted luma error
//   sse_item       one item -> su[Y, Cb, Cr]
// Include after pc_yuv_device.h and pc_chroma_items.h (emit_px, load4, clampi, code_of).
#ifndef PC_CHROMA_SSE_ITEM_H
#define PC_CHROMA_SSE_ITEM_H

namespace {

// What the measurement takes of the siting and the depth: co-sited along x (0 where the axis is not subsampled), s = 1 / (scale_h *
// scale_v), and the depth shift.  The vertical siting chooses the kernel (its template parameter VCO) on the host.
struct Measure {
    int hco;
    float s;
    int sh;
};

// One row of an item: the floats of tile columns q0 .. q0+7 at xr (channel stride sc; xr is column 0 of the tile's row), of which
// the lanes 0 .. hi-1 lie inside the frame -> the row's horizontally filtered chroma differences h[Cb, Cr][8 / SX] and, where the
// item owns the row (ry: lane 0 of the original's luma row), its weighted luma error ay * sum ax(q) e^2 into su.  A column right of
// hi - 1 is column hi - 1 (p[min(2m+1, N-1)]); the co-sited filter's column q0 - 1 is the halo pixel, column 0 at the tile's left
// edge (p[max(2m-1, 0)]).
template <class T, int SX, bool FULL>
__device__ __forceinline__ void weighted_row(const float* xr, int64_t sc, int q0, int hi, const T* ry, unsigned ay, const unsigned (&ax)[COLS],
                                             const Measure& ms, const Levels& lv, const EmitCoef& k, float (&h)[2][COLS / SX], u64& su)
{
    unsigned yq[COLS];
    float ub[COLS], ur[COLS];
    {
        float c[3][COLS];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = xr + ch * sc + q0;                   // q0 + 7 < T <= the row stride: inside the tile's row
            if (FULL) {
                const float4 f0 = *reinterpret_cast<const float4*>(s), f1 = *reinterpret_cast<const float4*>(s + 4);
                c[ch][0] = f0.x; c[ch][1] = f0.y; c[ch][2] = f0.z; c[ch][3] = f0.w;
                c[ch][4] = f1.x; c[ch][5] = f1.y; c[ch][6] = f1.z; c[ch][7] = f1.w;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) c[ch][q] = s[min(q, hi - 1)];
            }
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(c[0][q], c[1][q], c[2][q], lv, k, yq[q], ub[q], ur[q]);
    }
    if (SX == 1) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) { h[0][q] = ub[q]; h[1][q] = ur[q]; }
    } else if (ms.hco) {
        const int ql = max(q0 - 1, 0);
        unsigned yl;
        float bl, rl;
        emit_px(xr[ql], xr[sc + ql], xr[2 * sc + ql], lv, k, yl, bl, rl);
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j) {
            h[0][j] = ((j ? ub[2 * j - 1] : bl) + ub[2 * j + 1]) + (ub[2 * j] + ub[2 * j]);
            h[1][j] = ((j ? ur[2 * j - 1] : rl) + ur[2 * j + 1]) + (ur[2 * j] + ur[2 * j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j) {
            h[0][j] = ub[2 * j] + ub[2 * j + 1];
            h[1][j] = ur[2 * j] + ur[2 * j + 1];
        }
    }
    if (!ry) return;
    unsigned w[COLS];
    if (FULL) {
        load4(ry, w);
        load4(ry + 4, w + 4);
    } else {
#pragma unroll
        for (int q = 0; q < COLS; ++q) w[q] = q < hi ? (unsigned)ry[q] : 0u;
    }
    u64 row = 0ull;                                               // each term < 2^11 * 2^16 (8 bits), 2^10 * 2^20 (10 bits)
#pragma unroll
    for (int q = 0; q < COLS; ++q) {
        if (FULL || q < hi) {
            const int e = (int)yq[q] - (int)code_of<T>(w[q], ms.sh, (unsigned)lv.maxv);
            row += (u64)(ax[q] * (unsigned)(e * e));
        }
    }
    su += (u64)ay * row;
}

// One item: tile rows r0 .. r0 + SY - 1 and tile columns q0 .. q0+7 of the tile at xt, of which `rows` rows and the lanes 0 .. hi-1
// lie inside the frame (1 <= rows <= SY, 1 <= hi <= 8); Y, X: the frame position of (r0, q0), multiples of SY and of 8 / 4.  FULL:
// rows == SY, hi == 8 and every access is wide; else element by element.  ay[SY], ax[8]: the band numerators of the item's rows and
// columns, whether inside the frame or not.  The whole item is compiled twice, so that the two kinds of access never meet in one
// basic block.
template <class T, bool IL, int SX, int SY, bool VCO, bool FULL>
__device__ __forceinline__ void sse_item(const float* xt, int64_t sc, int64_t sh, int r0, int q0, int rows, int hi, const Planes<const T>& ref,
                                         int64_t Y, int64_t X, const Measure& ms, const Levels& lv, const EmitCoef& k,
                                         const unsigned (&ay)[SY], const unsigned (&ax)[COLS], u64 su[3])
{
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
    const int nc = SX == 2 ? (hi + 1) >> 1 : hi;
    const T* ry = ref.y + Y * ref.yr + X;
    float v[2][NC];
    if (SY == 1) {
        weighted_row<T, SX, FULL>(xt + (int64_t)r0 * sh, sc, q0, hi, ry, ay[0], ax, ms, lv, k, v, su[0]);
    } else {
        // In the order the vertical rule adds them: the row above (a, co-sited only; row 0 itself at the tile's top edge), the row
        // below (c; the last row inside the frame stands in for a missing one), then the item's first row (b): (a + c) + (b + b), or
        // b + c.
        const bool second = FULL || rows == 2;
        float acc[2][NC], t[2][NC];
        if (VCO) {
            weighted_row<T, SX, FULL>(xt + (int64_t)max(r0 - 1, 0) * sh, sc, q0, hi, nullptr, 0u, ax, ms, lv, k, acc, su[0]);
            weighted_row<T, SX, FULL>(xt + (int64_t)(second ? r0 + 1 : r0) * sh, sc, q0, hi, second ? ry + ref.yr : nullptr, ay[SY - 1], ax, ms,
                                      lv, k, t, su[0]);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[p][j] = acc[p][j] + t[p][j];
        } else {
            weighted_row<T, SX, FULL>(xt + (int64_t)(second ? r0 + 1 : r0) * sh, sc, q0, hi, second ? ry + ref.yr : nullptr, ay[SY - 1], ax, ms,
                                      lv, k, acc, su[0]);
        }
        weighted_row<T, SX, FULL>(xt + (int64_t)r0 * sh, sc, q0, hi, ry, ay[0], ax, ms, lv, k, t, su[0]);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < NC; ++j) v[p][j] = VCO ? acc[p][j] + (t[p][j] + t[p][j]) : t[p][j] + acc[p][j];
    }
    // chroma: the frame's sample (Y / SY, X / SX + m) is the tile's sample (r0 / SY, q0 / SX + m)
    const int64_t ci = SY == 2 ? Y >> 1 : Y, cx0 = SX == 2 ? X >> 1 : X;
    const T* ru = ref.u + ci * ref.ur + CS * cx0;
    const T* rv = IL ? ru + 1 : ref.v + ci * ref.vr + cx0;
    unsigned w[2][NC];
    if (FULL) {
        if (IL) {
            unsigned e[2 * NC];
#pragma unroll
            for (int m = 0; m < 2 * NC; m += 4) load4(ru + m, e + m);
#pragma unroll
            for (int j = 0; j < NC; ++j) { w[0][j] = e[2 * j]; w[1][j] = e[2 * j + 1]; }
        } else {
#pragma unroll
            for (int m = 0; m < NC; m += 4) { load4(ru + m, w[0] + m); load4(rv + m, w[1] + m); }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            w[0][j] = j < nc ? (unsigned)ru[CS * j] : 0u;
            w[1][j] = j < nc ? (unsigned)rv[CS * j] : 0u;
        }
    }
    const u64 cy = (u64)(SY == 2 ? (ay[0] + ay[SY - 1]) >> 1 : ay[0]);
    u64 sb = 0ull, sr = 0ull;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (FULL || j < nc) {
            const int eb = clampi((int)rintf(v[0][j] * ms.s + (float)lv.co), 0, lv.maxv) - (int)code_of<T>(w[0][j], ms.sh, (unsigned)lv.maxv);
            const int er = clampi((int)rintf(v[1][j] * ms.s + (float)lv.co), 0, lv.maxv) - (int)code_of<T>(w[1][j], ms.sh, (unsigned)lv.maxv);
            const unsigned cx = SX == 2 ? (ax[SX * j] + ax[SX * j + SX - 1]) >> 1 : ax[j];
            sb += (u64)(cx * (unsigned)(eb * eb));
            sr += (u64)(cx * (unsigned)(er * er));
        }
    }
    su[1] += cy * sb;
    su[2] += cy * sr;
}

}  // namespace

#endif  // PC_CHROMA_SSE_ITEM_H
