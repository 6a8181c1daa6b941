// pc_chroma_items.h -- what the libraries of the twelve YUV formats and three chroma sitings (chroma, chroma_tiles, chroma_rate,
// chroma_clips; DESIGN.md sections 21 and 23 to 25) share: the ingest item with its taps, the code of an element, and the host's
// checks of a format, a siting and a picture.  The __global__ kernels, their launch bounds, grids and parameter lists, the emit-side
// rows and every decision about the access path stay in each library's own .hip file.
//   ingest_item    eight luma columns of one row -> float32 R, G, B (section 21's ingest): chroma, chroma_tiles, chroma_clips
//   code_of        the code of an element, word_of the element of a code: all four
//   format_of ...  layout, depth, shift and subsampling -> Fmt; site_ok, depth_levels, picture_ok, with_format: all four
//   taps_of        the ingest's weights from the subsampling, the siting and the upsampler
// The layout and siting values are this header's own; each library asserts that its public enumerators equal them.  Include after
// pc_yuv_device.h.
#ifndef PC_CHROMA_ITEMS_H
#define PC_CHROMA_ITEMS_H

#include <type_traits>

namespace {

constexpr int LAYOUT_PLANAR = 0, LAYOUT_SEMIPLANAR = 1;
constexpr int SITE_CENTRE = 0, SITE_COSITED = 1;

// The ingest's weights of the (near, far) chroma sample along x and y for an even and an odd luma index, and the depth shift.
struct Taps {
    int xe0, xe1, xo0, xo1, ye0, ye1, yo0, yo1, sh;
};

// The code of an element and the element of a code.  An 8-bit element is its code (shift 0, nothing above it), which the 8-bit
// instantiations know at compile time; a 16-bit word carries a wave-uniform shift and may hold other bits.
template <class T>
__device__ __forceinline__ unsigned code_of(unsigned w, int sh, unsigned mask) { return sizeof(T) == 1 ? w : (w >> sh) & mask; }

template <class T>
__device__ __forceinline__ unsigned word_of(unsigned code, int sh) { return sizeof(T) == 1 ? code : code << sh; }

// -- ingest --------------------------------------------------------------------------------------------------------------------------

// Luma row y (0 <= y < H) and columns x0 .. x0+7 of one picture -> o[R, G, B][column]; a column outside [0, W) is left as it is.
// The far tap of an axis is the chroma sample after the near one for an odd luma index, before it for an even one, clamped to the
// plane; what it weighs (0 where the rule has no second tap) is in t.  WIDE needs x0 a multiple of 8 at SX = 2 and of 4 at SX = 1.
template <class T, bool IL, int SX, int SY, bool WIDE>
__device__ __forceinline__ void ingest_item(const Planes<const T>& s, int W, int Hc, int Wc, int y, int x0, const Taps& t, const Levels& lv,
                                            const IngestCoef& k, float (&o)[3][COLS])
{
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    const int sh = t.sh;
    const unsigned mask = (unsigned)lv.maxv;
    const int i0 = SY == 2 ? y >> 1 : y;
    const int i1 = SY == 2 ? clampi(i0 + ((y & 1) ? 1 : -1), 0, Hc - 1) : i0;
    const int wy0 = SY == 2 ? ((y & 1) ? t.yo0 : t.ye0) : 4, wy1 = SY == 2 ? ((y & 1) ? t.yo1 : t.ye1) : 0;
    const T* yrow = s.y + (int64_t)y * s.yr;
    const T* u0 = s.u + (int64_t)i0 * s.ur;                       // Cb of chroma row i0, i1; Cr: one element on, or the V plane
    const T* u1 = s.u + (int64_t)i1 * s.ur;
    const T* v0 = IL ? u0 + 1 : s.v + (int64_t)i0 * s.vr;
    const T* v1 = IL ? u1 + 1 : s.v + (int64_t)i1 * s.vr;
    if (WIDE && x0 >= 0 && x0 + COLS - 1 < W) {
        constexpr int NW = SX == 2 ? 6 : COLS;                     // SX == 2: columns jl, jc .. jc+3, jr; else jc .. jc+7
        unsigned Yc[COLS];
        load4(yrow + x0, Yc);
        load4(yrow + x0 + 4, Yc + 4);
        const int jc = x0 / SX;                                    // the item's first chroma column; jc * CS is a multiple of 4
        unsigned cw[2][2][NW];                                     // [row i0, i1][Cb, Cr][column]
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const T* pu = rr ? u1 : u0;
            const T* pv = rr ? v1 : v0;
            if (rr == 1 && (SY == 1 || wy1 == 0)) {
#pragma unroll
                for (int j = 0; j < NW; ++j) { cw[1][0][j] = cw[0][0][j]; cw[1][1][j] = cw[0][1][j]; }
                break;
            }
            constexpr int F = SX == 2 ? 1 : 0;                     // where column jc stands in cw
            constexpr int NI = COLS / SX;                          // chroma columns of the item
            if (IL) {
                unsigned e[2 * NI];
#pragma unroll
                for (int m = 0; m < 2 * NI; m += 4) load4(pu + 2 * (int64_t)jc + m, e + m);
#pragma unroll
                for (int j = 0; j < NI; ++j) { cw[rr][0][F + j] = e[2 * j]; cw[rr][1][F + j] = e[2 * j + 1]; }
            } else {
#pragma unroll
                for (int m = 0; m < NI; m += 4) {
                    load4(pu + jc + m, &cw[rr][0][F + m]);
                    load4(pv + jc + m, &cw[rr][1][F + m]);
                }
            }
            if (SX == 2) {
                const int jl = max(jc - 1, 0), jr = min(jc + 4, Wc - 1);
                cw[rr][0][0] = pu[CS * (int64_t)jl]; cw[rr][1][0] = pv[CS * (int64_t)jl];
                cw[rr][0][NW - 1] = pu[CS * (int64_t)jr]; cw[rr][1][NW - 1] = pv[CS * (int64_t)jr];
            }
        }
#pragma unroll
        for (int i = 0; i < COLS; ++i) {
            const int j0 = SX == 2 ? 1 + (i >> 1) : i, j1 = SX == 2 ? ((i & 1) ? j0 + 1 : j0 - 1) : j0;
            const int wx0 = SX == 2 ? ((i & 1) ? t.xo0 : t.xe0) : 4, wx1 = SX == 2 ? ((i & 1) ? t.xo1 : t.xe1) : 0;
            int c16[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int c00 = (int)code_of<T>(cw[0][p][j0], sh, mask), c01 = (int)code_of<T>(cw[0][p][j1], sh, mask);
                const int c10 = (int)code_of<T>(cw[1][p][j0], sh, mask), c11 = (int)code_of<T>(cw[1][p][j1], sh, mask);
                c16[p] = wy0 * (wx0 * c00 + wx1 * c01) + wy1 * (wx0 * c10 + wx1 * c11);
            }
            to_rgb((int)code_of<T>(Yc[i], sh, mask), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
        }
    } else {                                                      // element by element; also the items that straddle an edge
#pragma unroll
        for (int i = 0; i < COLS; ++i) {
            const int x = x0 + i;
            if (x >= 0 && x < W) {
                const int64_t j0 = SX == 2 ? x >> 1 : x;
                const int64_t j1 = SX == 2 ? clampi((int)j0 + ((x & 1) ? 1 : -1), 0, Wc - 1) : j0;
                const int wx0 = SX == 2 ? ((x & 1) ? t.xo0 : t.xe0) : 4, wx1 = SX == 2 ? ((x & 1) ? t.xo1 : t.xe1) : 0;
                int c16[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const T* r0 = p ? v0 : u0;
                    const T* r1 = p ? v1 : u1;
                    int near = wx0 * (int)code_of<T>((unsigned)r0[CS * j0], sh, mask);
                    if (wx1) near += wx1 * (int)code_of<T>((unsigned)r0[CS * j1], sh, mask);
                    c16[p] = wy0 * near;
                    if (wy1) {
                        int far = wx0 * (int)code_of<T>((unsigned)r1[CS * j0], sh, mask);
                        if (wx1) far += wx1 * (int)code_of<T>((unsigned)r1[CS * j1], sh, mask);
                        c16[p] += wy1 * far;
                    }
                }
                to_rgb((int)code_of<T>((unsigned)yrow[x], sh, mask), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
            }
        }
    }
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

struct Fmt {
    bool il;
    int bits, sh, sx, sy;
};

bool format_of(int layout, int bits, int shift, int sx, int sy, Fmt& f)
{
    if (layout != LAYOUT_PLANAR && layout != LAYOUT_SEMIPLANAR) return false;
    if (!((bits == 8 && shift == 0) || (bits == 10 && (shift == 0 || shift == 6)))) return false;
    if (!((sx == 2 && sy == 2) || (sx == 2 && sy == 1) || (sx == 1 && sy == 1))) return false;
    f = Fmt{layout == LAYOUT_SEMIPLANAR, bits, shift, sx, sy};
    return true;
}

bool site_ok(int s) { return s == SITE_CENTRE || s == SITE_COSITED; }

// the levels are those of the shared header for the depth: NV12's for 8 bits, P010's for 10
bool depth_levels(int bits, int range, Levels& lv) { return levels_of(bits == 10 ? PC_YUV_P010 : PC_YUV_NV12, range, lv); }

// One picture of W luma columns in format f; the batch strides are not looked at.
bool picture_ok(const Fmt& f, const pc_frame* fr, int W)
{
    if (!fr) return false;
    const int es = f.bits == 10 ? 2 : 1;
    const int64_t Wc = cdiv(W, f.sx);
    if (!plane_ok(fr->y, fr->y_row, es, W)) return false;
    if (f.il) return plane_ok(fr->u, fr->u_row, es, 2 * Wc);
    return plane_ok(fr->u, fr->u_row, es, Wc) && plane_ok(fr->v, fr->v_row, es, Wc);
}

// the weights of one axis of the ingest: (near, far) at an even and at an odd luma index
void axis_taps(bool subsampled, bool linear, bool cosited, int& e0, int& e1, int& o0, int& o1)
{
    e0 = o0 = 4;
    e1 = o1 = 0;
    if (!subsampled || !linear) return;
    if (cosited) { o0 = 2; o1 = 2; }
    else { e0 = o0 = 3; e1 = o1 = 1; }
}

Taps taps_of(int sx, int sy, int hsite, int vsite, bool linear, int shift)
{
    Taps t;
    axis_taps(sx == 2, linear, hsite == SITE_COSITED, t.xe0, t.xe1, t.xo0, t.xo1);
    axis_taps(sy == 2, linear, vsite == SITE_COSITED, t.ye0, t.ye1, t.yo0, t.yo1);
    t.sh = shift;
    return t;
}

template <int N>
using Int = std::integral_constant<int, N>;

// f(element, interleaved, SX, SY) with the format's compile-time values
template <class F>
void with_format(const Fmt& fm, F f)
{
    auto sub = [&](auto el, auto il) {
        if (fm.sy == 2) f(el, il, Int<2>{}, Int<2>{});
        else if (fm.sx == 2) f(el, il, Int<2>{}, Int<1>{});
        else f(el, il, Int<1>{}, Int<1>{});
    };
    if (fm.bits == 8) {
        if (fm.il) sub(uint8_t{}, std::true_type{}); else sub(uint8_t{}, std::false_type{});
    } else {
        if (fm.il) sub(uint16_t{}, std::true_type{}); else sub(uint16_t{}, std::false_type{});
    }
}

}  // namespace

#endif  // PC_CHROMA_ITEMS_H
