// pc_chroma.hip -- YUV 4:2:0 / 4:2:2 / 4:4:4 frames, planar or semi-planar, 8-bit or 10-bit in 16-bit words, chroma sited at the
// centre of its luma samples or on the even ones, <-> the codec's float32 RGB planes on gfx950 (pc_chroma.h).  Definition: DESIGN.md
// section 21.  pc_frames.hip generalised: at 4:2:0 with centre siting every sample goes through the same operations in the same order.
//
// A work item is eight consecutive luma columns: of ONE padded row for the ingest, of SY rows of the window for the emit (a row pair
// at 4:2:0, one row at 4:2:2 and 4:4:4) with the 8 / SX chroma samples of those columns.  A thread takes one item, a block NT
// consecutive items of ONE picture.  The access path (WIDE: four elements of a plane and four floats per access; else one by one)
// only changes the load and store instructions, never which thread handles which sample or in which order it adds.
//
// The co-sited emit filter [1, 2, 1] reaches one luma column left of the item and, vertically, one luma row above it.  The item
// computes emit_px of those halo pixels itself, from the same three floats by the same single IEEE operations as the item that owns
// them, so both hold the same bits and no item waits for another: no LDS, no cross-lane traffic, no dependence on where a wave or a
// block begins.  The price is three scalar loads per row (of a cache line the neighbouring lane reads anyway) and, for a vertical
// halo, a third row of emit_px per row pair.
//
// Template parameters are what changes the shape of an item (element type, interleave, SX, SY, the access path, whether sums are
// taken and, at SY = 2, whether the row above is read); the depth shift, the tap weights of the ingest, the horizontal siting of
// the emit and its scale are wave-uniform kernel arguments.  24 ingest kernels, 64 emit kernels and the final.
// No LDS on the data path; the sums go thread, wave tree, waves in order (12 words of LDS), then emit_final over the block partials,
// no atomics (image_csrc/pc_reduce.h).
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"
#include "pc_chroma_items.h"

#include "pc_chroma.h"

namespace {

static_assert(PC_CH_PLANAR == LAYOUT_PLANAR && PC_CH_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma.h's");
static_assert(PC_CH_CENTRE == SITE_CENTRE && PC_CH_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma.h's");

template <class T>
struct Batch {                           // pc_ch_frame with typed pointers; strides in elements
    T* y;
    int64_t yb, yr;
    T* u;
    int64_t ub, ur;
    T* v;
    int64_t vb, vr;
};

// The emit's siting: co-sited along x / y (0 on an axis that is not subsampled), s = 1 / (scale_h * scale_v), and the depth shift.
// The kernels read hco, s and sh; vco chooses the kernel (its template parameter VCO) on the host.
struct Site {
    int hco, vco;
    float s;
    int sh;
};

// -- ingest --------------------------------------------------------------------------------------------------------------------------

// Items are the eight-column groups of the PADDED rows: item -> (yp, g), columns 8g .. 8g+7 of row yp of dst.  G = ceil(Wp / 8),
// items = Hp * G per picture, blocks = ceil(items / NT) per picture.
template <class T, bool IL, int SX, int SY, bool WIDE>
__global__ __launch_bounds__(NT) void ingest_kernel(Batch<const T> s, int H, int W, int Hc, int Wc, float* __restrict__ dst, int Hp, int Wp,
                                                    int top, int left, int G, int items, int blocks, Taps t, Levels lv, IngestCoef k)
{
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    const int item = blk * NT + threadIdx.x;
    if (item >= items) return;
    const int yp = item / G, g = item - yp * G;
    const int xp0 = COLS * g, n = min(COLS, Wp - xp0);            // n columns of dst exist
    const int y = yp - top, x0 = xp0 - left;                      // picture coordinates of the first column
    float o[3][COLS];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < COLS; ++i) o[c][i] = 0.f;
    if (y >= 0 && y < H && x0 + COLS - 1 >= 0 && x0 < W) {       // x0 is a multiple of 8 on the wide path (left is)
        const Planes<const T> pic{s.y + b * s.yb, s.yr, s.u + b * s.ub, s.ur, IL ? nullptr : s.v + b * s.vb, s.vr};
        ingest_item<T, IL, SX, SY, WIDE>(pic, W, Hc, Wc, y, x0, t, lv, k, o);
    }
    const int64_t plane = (int64_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) store8<WIDE>(dst + (b * (int64_t)3 + c) * plane + (int64_t)yp * Wp + xp0, o[c], n);   // WIDE: Wp is a multiple of 8, n == 8
}

// -- emit ----------------------------------------------------------------------------------------------------------------------------

// One luma row of an item: the floats of columns x0 .. x0+n-1 at xr (channel stride sc; xr is column 0 of the window's row) ->
// their luma codes (written to dy and compared with ry where the item owns the row and the pointers are set) and the row's
// horizontally filtered chroma differences h[Cb, Cr][8 / SX].  A column right of the last one is the last one (p[min(2j+1, N-1)]);
// the co-sited filter's column x0 - 1 is the halo pixel, column 0 at the picture's left edge (p[max(2j-1, 0)]).
template <class T, int SX, bool FULL, bool HAS_REF>
__device__ __forceinline__ void emit_row(const float* xr, int64_t sc, bool own, T* dy, const T* ry, int x0, int n, const Site& st,
                                         const Levels& lv, const EmitCoef& k, float (&h)[2][COLS / SX], u64& su)
{
    unsigned yq[COLS];
    float ub[COLS], ur[COLS];
    {
        float c[3][COLS];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = xr + ch * sc + x0;
            if (FULL) {
                const float4 f0 = *reinterpret_cast<const float4*>(s), f1 = *reinterpret_cast<const float4*>(s + 4);
                c[ch][0] = f0.x; c[ch][1] = f0.y; c[ch][2] = f0.z; c[ch][3] = f0.w;
                c[ch][4] = f1.x; c[ch][5] = f1.y; c[ch][6] = f1.z; c[ch][7] = f1.w;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) c[ch][q] = s[min(q, n - 1)];   // the last column stands in for those right of it
            }
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(c[0][q], c[1][q], c[2][q], lv, k, yq[q], ub[q], ur[q]);
    }
    if (SX == 1) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) { h[0][q] = ub[q]; h[1][q] = ur[q]; }
    } else if (st.hco) {
        const int xl = max(x0 - 1, 0);
        unsigned yl;
        float bl, rl;
        emit_px(xr[xl], xr[sc + xl], xr[2 * sc + xl], lv, k, yl, bl, rl);
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
    if (!own) return;
    if (dy) {
        if (FULL) {
            unsigned w[COLS];
#pragma unroll
            for (int q = 0; q < COLS; ++q) w[q] = word_of<T>(yq[q], st.sh);
            store4(dy + x0, w);
            store4(dy + x0 + 4, w + 4);
        } else {
#pragma unroll
            for (int q = 0; q < COLS; ++q)
                if (q < n) dy[x0 + q] = (T)word_of<T>(yq[q], st.sh);
        }
    }
    if (HAS_REF) {
        unsigned w[COLS];
        if (FULL) {
            load4(ry + x0, w);
            load4(ry + x0 + 4, w + 4);
        } else {
#pragma unroll
            for (int q = 0; q < COLS; ++q) w[q] = q < n ? (unsigned)ry[x0 + q] : 0u;
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) {
            if (q < n) {
                const int e = (int)yq[q] - (int)code_of<T>(w[q], st.sh, (unsigned)lv.maxv);
                su += (u64)(e * e);
            }
        }
    }
}

// One item of the emit: chroma row i, luma rows SY i .. SY i + SY - 1 (the last may be missing at the odd last row), luma columns
// x0 .. x0+n-1, chroma columns x0 / SX ...  FULL: n == 8 and every access is wide; else element by element.  The whole item is
// compiled twice, not only its loads and stores, so that the two kinds of access never meet in one basic block.
template <class T, bool IL, int SX, int SY, bool VCO, bool FULL, bool HAS_REF>
__device__ __forceinline__ void emit_item(const float* xw, int64_t sc, int64_t sh, int H, const Planes<T>& dst, const Planes<const T>& ref, int i,
                                          int x0, int n, const Site& st, const Levels& lv, const EmitCoef& k, u64 su[3])
{
    constexpr int CS = IL ? 2 : 1;
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
    const int nc = SX == 2 ? (n + 1) >> 1 : n;
    float v[2][NC];
    if (SY == 1) {
        emit_row<T, SX, FULL, HAS_REF>(xw + (int64_t)i * sh, sc, true, dst.y ? dst.y + (int64_t)i * dst.yr : nullptr,
                                       HAS_REF ? ref.y + (int64_t)i * ref.yr : nullptr, x0, n, st, lv, k, v, su[0]);
    } else {
        const int r0 = 2 * i, r1 = min(r0 + 1, H - 1);            // the last row stands in for the one below it
        float hb[2][NC], hc[2][NC];
        emit_row<T, SX, FULL, HAS_REF>(xw + (int64_t)r0 * sh, sc, true, dst.y ? dst.y + (int64_t)r0 * dst.yr : nullptr,
                                       HAS_REF ? ref.y + (int64_t)r0 * ref.yr : nullptr, x0, n, st, lv, k, hb, su[0]);
        emit_row<T, SX, FULL, HAS_REF>(xw + (int64_t)r1 * sh, sc, r0 + 1 < H, dst.y ? dst.y + (int64_t)r1 * dst.yr : nullptr,
                                       HAS_REF ? ref.y + (int64_t)r1 * ref.yr : nullptr, x0, n, st, lv, k, hc, su[0]);
        if (VCO) {
            const int ra = max(r0 - 1, 0);                        // the halo row; row 0 at the picture's top edge
            float ha[2][NC];
            emit_row<T, SX, FULL, false>(xw + (int64_t)ra * sh, sc, false, nullptr, nullptr, x0, n, st, lv, k, ha, su[0]);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NC; ++j) v[p][j] = (ha[p][j] + hc[p][j]) + (hb[p][j] + hb[p][j]);
        } else {
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NC; ++j) v[p][j] = hb[p][j] + hc[p][j];
        }
    }
    unsigned cq[2][NC];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < NC; ++j) cq[p][j] = (unsigned)clampi((int)rintf(v[p][j] * st.s + (float)lv.co), 0, lv.maxv);
    const int64_t cx0 = x0 / SX;
    if (dst.y) {
        T* du = dst.u + (int64_t)i * dst.ur + CS * cx0;
        T* dv = IL ? du + 1 : dst.v + (int64_t)i * dst.vr + cx0;
        if (FULL) {
            if (IL) {
                unsigned w[2 * NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) { w[2 * j] = word_of<T>(cq[0][j], st.sh); w[2 * j + 1] = word_of<T>(cq[1][j], st.sh); }
#pragma unroll
                for (int m = 0; m < 2 * NC; m += 4) store4(du + m, w + m);
            } else {
                unsigned w[2][NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) { w[0][j] = word_of<T>(cq[0][j], st.sh); w[1][j] = word_of<T>(cq[1][j], st.sh); }
#pragma unroll
                for (int m = 0; m < NC; m += 4) { store4(du + m, w[0] + m); store4(dv + m, w[1] + m); }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j < nc) { du[CS * j] = (T)word_of<T>(cq[0][j], st.sh); dv[CS * j] = (T)word_of<T>(cq[1][j], st.sh); }
        }
    }
    if (HAS_REF) {
        const T* ru = ref.u + (int64_t)i * ref.ur + CS * cx0;
        const T* rv = IL ? ru + 1 : ref.v + (int64_t)i * ref.vr + cx0;
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
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (j < nc) {
                const int eb = (int)cq[0][j] - (int)code_of<T>(w[0][j], st.sh, (unsigned)lv.maxv);
                const int er = (int)cq[1][j] - (int)code_of<T>(w[1][j], st.sh, (unsigned)lv.maxv);
                su[1] += (u64)(eb * eb);
                su[2] += (u64)(er * er);
            }
        }
    }
}

// Items are the eight-column groups of the WINDOW's chroma rows: item -> (i, g), luma rows SY i .., columns 8g .. 8g+7 of the
// picture.  G = ceil(W / 8), items = Hc * G per picture.  x.p is the window's first pixel.  partials: [gridDim.x][3].
template <class T, bool IL, int SX, int SY, bool VCO, bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void emit_kernel(F32 x, int H, int W, Batch<T> dst, Batch<const T> ref, int G, int items, int blocks, Site st,
                                                  Levels lv, EmitCoef k, u64* __restrict__ partials)
{
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    const int item = blk * NT + threadIdx.x;
    u64 su[3] = {0ull, 0ull, 0ull};
    if (item < items) {
        const int i = item / G, g = item - i * G;
        const int x0 = COLS * g, n = min(COLS, W - x0);           // n luma columns exist
        const Planes<T> d{dst.y ? dst.y + b * dst.yb : nullptr, dst.yr, dst.u + b * dst.ub, dst.ur, IL ? nullptr : dst.v + b * dst.vb, dst.vr};
        const Planes<const T> r{ref.y + b * ref.yb, ref.yr, ref.u + b * ref.ub, ref.ur, IL ? nullptr : ref.v + b * ref.vb, ref.vr};
        const float* xw = x.p + b * x.st;
        if (WIDE && n == COLS) emit_item<T, IL, SX, SY, VCO, true, HAS_REF>(xw, x.sc, x.sh, H, d, r, i, x0, n, st, lv, k, su);
        else emit_item<T, IL, SX, SY, VCO, false, HAS_REF>(xw, x.sc, x.sh, H, d, r, i, x0, n, st, lv, k, su);
    }
    if (HAS_REF) block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One block per picture: its block partials (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void emit_final_kernel(const u64* __restrict__ partials, int blocks, u64* __restrict__ sse)
{
    const int b = blockIdx.x;
    u64 su[3] = {0ull, 0ull, 0ull};
    gather_partials<Sum>(partials + (int64_t)b * blocks * 3, 0, blocks, (int)threadIdx.x, NT, su);
    block_reduce<Sum>(su, sse + b * 3);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

// One plane of B pictures of `rows` rows of `len` elements: pointer aligned to its element, strides in range; `disjoint`
// (destinations): rows inside pictures, which is sufficient (not necessary) for no element of the plane to be written twice.
bool batch_plane_ok(const void* p, int64_t sb, int64_t sr, int es, int B, int rows, int64_t len, bool disjoint)
{
    if (!p || reinterpret_cast<uintptr_t>(p) % es || sr < len || sb < 1) return false;
    if (disjoint && B > 1 && sb < (int64_t)(rows - 1) * sr + len) return false;
    return true;
}

// The frame check for Hc = ceil(H / sy), Wc = ceil(W / sx).
bool batch_frame_ok(const Fmt& f, const pc_ch_frame* fr, int B, int H, int W, bool disjoint)
{
    if (!fr) return false;
    const int es = f.bits == 10 ? 2 : 1, Hc = (int)cdiv(H, f.sy);
    const int64_t Wc = cdiv(W, f.sx);
    if (!batch_plane_ok(fr->y, fr->y_batch, fr->y_row, es, B, H, W, disjoint)) return false;
    if (f.il) return batch_plane_ok(fr->u, fr->u_batch, fr->u_row, es, B, Hc, 2 * Wc, disjoint);
    return batch_plane_ok(fr->u, fr->u_batch, fr->u_row, es, B, Hc, Wc, disjoint) && batch_plane_ok(fr->v, fr->v_batch, fr->v_row, es, B, Hc, Wc, disjoint);
}

// Sizes every call shares: B, rows, cols >= 1 and the block count of an item space of rows x ceil(cols / 8) per picture in 32 bits.
struct Items {
    int G, items, blocks;
};

bool items_of(int B, int rows, int cols, Items& g)
{
    if (B < 1 || rows < 1 || cols < 1) return false;
    const int64_t G = cdiv(cols, COLS), items = (int64_t)rows * G;
    if (items > INT32_MAX - NT) return false;
    const int64_t blocks = cdiv(items, NT);
    if ((int64_t)B * blocks > INT32_MAX) return false;
    g.G = (int)G;
    g.items = (int)items;
    g.blocks = (int)blocks;
    return true;
}

// The alignment of a frame as the wide path needs it: every plane pointer on four elements, every stride a multiple of 4.
bool batch_frame_wide(bool il, int es, const pc_ch_frame* f)
{
    if (!plane_wide(f->y, f->y_row, es) || !mult4(f->y_batch)) return false;
    if (!plane_wide(f->u, f->u_row, es) || !mult4(f->u_batch)) return false;
    return il || (plane_wide(f->v, f->v_row, es) && mult4(f->v_batch));
}

// The one place that decides the access path: the calls launch from it, pc_chroma_plan reports it.
bool wide_path(int op, bool il, int es, const pc_ch_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh, int left,
               const pc_ch_frame* ref)
{
    if (!f32_wide(f32, fb, fc, fh)) return false;
    if (op == PC_CH_INGEST) return fh % 8 == 0 && left % 8 == 0 && batch_frame_wide(il, es, frame);       // fh = Wp: no partial last item
    return left % 4 == 0 && (!frame || batch_frame_wide(il, es, frame)) && (!ref || batch_frame_wide(il, es, ref));
}

bool window_ok(int B, int H, int W, int Hp, int Wp, int top, int left)
{
    if (B < 1 || H < 1 || W < 1 || top < 0 || left < 0 || Hp < 1 || Wp < 1) return false;
    return (int64_t)top + H <= Hp && (int64_t)left + W <= Wp;
}

template <class T>
Batch<T> batch_of(const pc_ch_frame* f)
{
    if (!f) return Batch<T>{nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0};
    return Batch<T>{static_cast<T*>(f->y), f->y_batch, f->y_row, static_cast<T*>(f->u), f->u_batch, f->u_row, static_cast<T*>(f->v), f->v_batch,
                    f->v_row};
}

}  // namespace

extern "C" int pc_chroma_plan(int op, int layout, int bits, const pc_ch_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh,
                              int left, const pc_ch_frame* ref, int* wide)
{
    Fmt fm;
    if ((op != PC_CH_INGEST && op != PC_CH_EMIT) || !format_of(layout, bits, 0, 1, 1, fm) || !f32 || !wide || left < 0) return PC_ERR_ARG;
    if (op == PC_CH_INGEST) ref = nullptr;
    if (!frame && (op != PC_CH_EMIT || !ref)) return PC_ERR_ARG;
    for (const pc_ch_frame* f : {frame, ref})
        if (f && !(f->y && f->u && (fm.il || f->v))) return PC_ERR_ARG;
    *wide = wide_path(op, fm.il, bits == 10 ? 2 : 1, frame, f32, fb, fc, fh, left, ref) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_chroma_ingest(const pc_ch_frame* src, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                                int upsample, float a, float b, float c, float d, int B, int H, int W, float* dst, int Hp, int Wp, int top,
                                int left, void* stream)
{
    Items g;
    Levels lv;
    Fmt fm;
    if (!dst || !aligned(dst, 4) || !window_ok(B, H, W, Hp, Wp, top, left)) return PC_ERR_ARG;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!batch_frame_ok(fm, src, B, H, W, false) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (!items_of(B, Hp, Wp, g)) return PC_ERR_ARG;
    const int64_t plane = (int64_t)Hp * Wp;
    const bool wide = wide_path(PC_CH_INGEST, fm.il, bits == 10 ? 2 : 1, src, dst, 3 * plane, plane, Wp, left, nullptr);
    const IngestCoef k{a, b, c, d};
    const Taps t = taps_of(sx, sy, hsite, vsite, upsample == PC_CH_LINEAR, shift);
    const int Hc = (int)cdiv(H, sy), Wc = (int)cdiv(W, sx);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks));
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T = decltype(el);
        const Batch<const T> s = batch_of<const T>(src);
        if (wide)
            hipLaunchKernelGGL((ingest_kernel<T, il.value, SX.value, SY.value, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, dst, Hp, Wp, top,
                               left, g.G, g.items, g.blocks, t, lv, k);
        else
            hipLaunchKernelGGL((ingest_kernel<T, il.value, SX.value, SY.value, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, dst, Hp, Wp, top,
                               left, g.G, g.items, g.blocks, t, lv, k);
    });
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_chroma_emit_workspace_size(int B, int H, int W, int sy)
{
    Items g;
    if (H < 1 || (sy != 1 && sy != 2)) return 0;
    return items_of(B, (int)cdiv(H, sy), W, g) ? (size_t)B * g.blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_chroma_emit(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H, int W,
                              int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range, float kr, float kg,
                              float kb, float ib, float ir, const pc_ch_frame* dst, const pc_ch_frame* ref, void* workspace,
                              size_t workspace_bytes, uint64_t* sse, void* stream)
{
    Items g;
    Levels lv;
    Fmt fm;
    if (!x || !aligned(x, 4) || !window_ok(B, H, W, Hp, Wp, top, left)) return PC_ERR_ARG;
    if (sxh < Wp || sxc < 1 || sxb < 1 || !format_of(layout, bits, shift, sx, sy, fm) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (!site_ok(hsite) || !site_ok(vsite) || (!dst && !ref)) return PC_ERR_ARG;
    if (dst && !batch_frame_ok(fm, dst, B, H, W, true)) return PC_ERR_ARG;
    if (ref && !batch_frame_ok(fm, ref, B, H, W, false)) return PC_ERR_ARG;
    if (!items_of(B, (int)cdiv(H, sy), W, g)) return PC_ERR_ARG;
    if (ref) {
        if (!workspace || !aligned(workspace, 8) || !sse || !aligned(sse, 8)) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)B * g.blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_CH_EMIT, fm.il, bits == 10 ? 2 : 1, dst, x, sxb, sxc, sxh, left, ref);
    const F32 xv{x + (int64_t)top * sxh + left, sxb, sxc, sxh};                // the window's first pixel
    const EmitCoef k{kr, kg, kb, ib, ir};
    Site site;
    site.hco = sx == 2 && hsite == PC_CH_COSITED;
    site.vco = sy == 2 && vsite == PC_CH_COSITED;
    site.s = 1.f / (float)((sx == 2 ? (site.hco ? 4 : 2) : 1) * (sy == 2 ? (site.vco ? 4 : 2) : 1));
    site.sh = shift;
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks));
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T = decltype(el);
        const Batch<T> d = batch_of<T>(dst);
        const Batch<const T> r = batch_of<const T>(ref);
#define PC_EMIT(VCO, WIDE, REF)                                                                                                             \
    hipLaunchKernelGGL((emit_kernel<T, il.value, SX.value, SY.value, VCO, WIDE, REF>), grid, dim3(NT), 0, st, xv, H, W, d, r, g.G, g.items, g.blocks, \
                       site, lv, k, part)
    // VCO is instantiated for SY = 2 alone: at SY = 1 both branches below name the same kernel
#define PC_EMIT_V(WIDE, REF)                                                                                                                \
    do {                                                                                                                                    \
        if (SY.value == 2 && site.vco) PC_EMIT((SY.value == 2), WIDE, REF); else PC_EMIT(false, WIDE, REF);                                 \
    } while (0)
        if (ref) {
            if (wide) PC_EMIT_V(true, true); else PC_EMIT_V(false, true);
        } else {
            if (wide) PC_EMIT_V(true, false); else PC_EMIT_V(false, false);
        }
#undef PC_EMIT_V
#undef PC_EMIT
    });
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(emit_final_kernel, dim3((unsigned)B), dim3(NT), 0, st, part, g.blocks, reinterpret_cast<u64*>(sse));
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_chroma_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting, range or upsampler, unsupported shape or workspace too "
               "small (pc_chroma_emit_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_last_hip_error(void) { return g_last_hip.load(); }
