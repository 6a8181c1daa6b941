// pc_chroma_compare.h -- a tile's footprint in two frames of any of the twelve YUV formats and three chroma sitings (DESIGN.md section
// 25's footprint), as __device__ templates: what compare_tile of pc_yuv_items.h is for centre-sited 4:2:0.  What differs per caller
// is a compile-time policy or an argument, never a branch on the caller.  The __global__ kernels, their launch bounds, grids and
// parameter lists stay in each library's own .hip file.
//   compare_chroma_tile   a tile's footprint in two frames, SY luma rows by eight columns, and its halo ring: chroma_clip_tol (count,
//                         sse, maxabs); the policy Acc says what one sample pair adds.  pc_chroma_clips.hip's changes_item is this
//                         item under a count policy, still written out there (out of scope).
// An item whose samples all lie inside the frame and whose accesses are all wide is compiled on its own (FULL); every other item goes
// element by element.  The access path only changes the load instructions, never which thread holds which sample.  Include after
// pc_yuv_device.h, pc_tile_grid.h, pc_reduce.h and pc_chroma_items.h (code_of).
#ifndef PC_CHROMA_COMPARE_H
#define PC_CHROMA_COMPARE_H

namespace {

// The footprint's halo: whether the rule reaches one chroma sample below the items' rectangle (lo) and above it (hi) along y and
// along x -- four wave-uniform flags, computed on the host from the format, the siting and the upsampling --, the depth shift and
// the code mask.
struct Halo {
    int ylo, yhi, xlo, xhi, sh;
    unsigned mask;
};

// hi = 1 on a subsampled axis under linear upsampling; lo = 1 there under centre siting on that axis as well
inline Halo halo_of(int sx, int sy, bool centre_x, bool centre_y, bool linear, int shift, int bits)
{
    return Halo{sy == 2 && linear && centre_y, sy == 2 && linear, sx == 2 && linear && centre_x, sx == 2 && linear, shift,
                (1u << bits) - 1u};
}

// One item: luma rows Y .. Y + SY - 1 and columns X .. X+7 of the frame (multiples of SY and SX), of which `rows` rows and the lanes
// 0 .. hi-1 lie inside the tile's part of the frame (1 <= rows <= SY, 1 <= hi <= 8), and the chroma samples (Y / SY, X / SX + m),
// SX m < hi.  FULL: rows == SY, hi == 8 and every access is wide; else element by element.  A lane outside is 0 in both frames: it
// adds nothing.  Acc::take<T>(a, b, p, ha, ac): one sample pair of plane p (elements; the code is code_of<T>) into the thread's
// Acc::N numbers.  SY * 8 luma samples and 8 / SX of Cb and of Cr: at most 16 of a plane.
template <class T, bool IL, int SX, int SY, bool FULL, class Acc>
__device__ __forceinline__ void compare_chroma_item(const Planes<const T>& a, const Planes<const T>& b, int64_t Y, int64_t X, int rows, int hi,
                                                    const Halo& ha, unsigned (&ac)[Acc::N])
{
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
#pragma unroll
    for (int r = 0; r < SY; ++r) {
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
            for (int q = 0; q < COLS; ++q) Acc::template take<T>(wa[q], wb[q], 0, ha, ac);
        }
    }
    const int64_t ci = SY == 2 ? Y >> 1 : Y, cx0 = SX == 2 ? X >> 1 : X;
    const T* ua = a.u + ci * a.ur + CS * cx0;
    const T* va = IL ? ua + 1 : a.v + ci * a.vr + cx0;
    const T* ub = b.u + ci * b.ur + CS * cx0;
    const T* vb = IL ? ub + 1 : b.v + ci * b.vr + cx0;
    unsigned ca[2][NC], cb[2][NC];                                // [Cb, Cr][sample]
    if (FULL) {
        if (IL) {
            unsigned ea[2 * NC], eb[2 * NC];
#pragma unroll
            for (int m = 0; m < 2 * NC; m += 4) {
                load4(ua + m, ea + m);
                load4(ub + m, eb + m);
            }
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                ca[0][m] = ea[2 * m]; ca[1][m] = ea[2 * m + 1];
                cb[0][m] = eb[2 * m]; cb[1][m] = eb[2 * m + 1];
            }
        } else {
#pragma unroll
            for (int m = 0; m < NC; m += 4) {
                load4(ua + m, ca[0] + m);
                load4(va + m, ca[1] + m);
                load4(ub + m, cb[0] + m);
                load4(vb + m, cb[1] + m);
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const bool in = SX * m < hi;
            ca[0][m] = in ? (unsigned)ua[CS * m] : 0u;
            ca[1][m] = in ? (unsigned)va[CS * m] : 0u;
            cb[0][m] = in ? (unsigned)ub[CS * m] : 0u;
            cb[1][m] = in ? (unsigned)vb[CS * m] : 0u;
        }
    }
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        Acc::template take<T>(ca[0][m], cb[0][m], 1, ha, ac);
        Acc::template take<T>(ca[1][m], cb[1][m], 2, ha, ac);
    }
}

// A block's share of tile `tile` of the grid, frames a against b.  Blocks bl = 0 .. bpt - 1 of a tile hold its items: item ->
// (chroma row kp, group g), tile rows SY kp .. SY kp + SY - 1, tile columns 8g .. 8g+7 (G8 = T / 8); S and T are multiples of 4, so
// a tile's cells are the frame's, and the items cover the tile's luma and the chroma rectangle WITHOUT the halo exactly once.  Block
// bl = bpt holds the halo ring -- the chroma row above and below and the column left and right of that rectangle, where the rule has
// a halo on that side (ha) and the frame has the samples -- element by element: 2 * (T / SX + 2) + 2 * (T / SY) indices over NT
// threads, of which the ones that are on number at most 2 * 1026 + 2 * 1024 (4:2:0) or 2 * 2048 in one run (4:2:2): a thread takes
// at most 17 of a plane.
template <class T, bool IL, int SX, int SY, bool WIDE, class Acc>
__device__ __forceinline__ void compare_chroma_tile(const Planes<const T>& a, const Planes<const T>& b, const Grid& gr, int tile, int bl,
                                                    int bpt, int G8, const Halo& ha, unsigned (&ac)[Acc::N])
{
    constexpr int CS = IL ? 2 : 1;
    const int i = tile / gr.nx, j = tile - i * gr.nx;
    const int Yt = i * gr.S, Xt = j * gr.S;                       // the tile's first row and column in the frame: < H, < W
    const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
    if (bl < bpt) {
        const int rem = bl * NT + (int)threadIdx.x;               // < T * T / 8 <= 2^19
        const int kp = rem / G8, r0 = SY * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            const int rows = min(SY, hh - r0), hi = min(COLS, ww - q0);
            if (WIDE && rows == SY && hi == COLS)
                compare_chroma_item<T, IL, SX, SY, true, Acc>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ha, ac);
            else
                compare_chroma_item<T, IL, SX, SY, false, Acc>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ha, ac);
        }
    } else {
        // the chroma rectangle the items covered: rows r0c .. r1c, columns c0c .. c1c; the ring around it where the rule and the frame
        // have it
        const int Hc = (gr.H + SY - 1) / SY, Wc = (gr.W + SX - 1) / SX;
        const int r0c = Yt / SY, r1c = r0c + (hh + SY - 1) / SY - 1, c0c = Xt / SX, c1c = c0c + (ww + SX - 1) / SX - 1;
        const bool top = ha.ylo && r0c > 0, bottom = ha.yhi && r1c < Hc - 1, left = ha.xlo && c0c > 0, right = ha.xhi && c1c < Wc - 1;
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
                Acc::template take<T>((unsigned)a.u[oa], (unsigned)b.u[ob], 1, ha, ac);
                Acc::template take<T>((unsigned)*va, (unsigned)*vb, 2, ha, ac);
            }
        }
    }
}

}  // namespace

#endif  // PC_CHROMA_COMPARE_H
