// pc_frames.hip -- YUV 4:2:0 frames (NV12 / I420 / P010) <-> the codec's float32 RGB planes on gfx950 (pc_frames.h).  Definition:
// DESIGN.md section 13.
//
// A work item is eight consecutive luma columns: of ONE padded row for the ingest (its two chroma rows are chosen per luma row, so a
// row pair shares no arithmetic there), of one ROW PAIR of the window for the emit (four chroma samples, each the mean of 2 x 2 luma
// positions).  A thread takes one item, a block NT consecutive items of ONE picture.  Eight columns, not four, so that every plane
// moves at least 32 bits per access (four I420 chroma bytes) and the float planes two 128-bit words.  The access path (WIDE: four
// elements of a plane and four floats per access; else one by one) only changes the load and store instructions, never which thread
// handles which sample or in which order it adds: the bits are the same on both.  No LDS on the data path; the sums go thread, wave
// tree, waves in order (12 words of LDS), then emit_final over the block partials, no atomics (image_csrc/pc_reduce.h).  The ingest
// of one item is cut_item of image_csrc/pc_yuv_items.h, as in pc_frame_tiles.hip and pc_clips.hip.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"

#include "pc_frames.h"

namespace {

template <class T>
struct BatchPlanes {                     // pc_frame with typed pointers; strides in elements.  Only this library has batches
    T* y;
    int64_t yb, yr;
    T* u;
    int64_t ub, ur;
    T* v;
    int64_t vb, vr;
};

// Items are the eight-column groups of the PADDED rows: item -> (yp, g), columns 8g .. 8g+7 of row yp of dst.  G = ceil(Wp / 8),
// items = Hp * G per picture, blocks = ceil(items / NT) per picture.  SH: the bits below the code in an element (P010: 6).
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void ingest_kernel(BatchPlanes<const T> s, int H, int W, int Hc, int Wc, float* __restrict__ dst, int Hp,
                                                    int Wp, int top, int left, int G, int items, int blocks, int linear, Levels lv,
                                                    IngestCoef k)
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
        cut_item<T, IL, WIDE, true>(pic, W, Hc, Wc, y, x0, linear, lv, k, o);
    }
    const int64_t plane = (int64_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) store8<WIDE>(dst + (b * (int64_t)3 + c) * plane + (int64_t)yp * Wp + xp0, o[c], n);   // WIDE: Wp is a multiple of 8, n == 8
}

// One item of the emit: rows 2i and 2i+1 (`rows` of them exist), luma columns x0 .. x0+n-1, chroma row i, columns x0/2 ...  FULL: n == 8
// and every access is wide; else element by element.  The whole item is compiled twice, not only its loads and stores, so that the
// two kinds of access never meet in one basic block (where the compiler merges them into the narrow kind).
template <class T, bool IL, bool FULL, bool HAS_REF>
__device__ __forceinline__ void emit_item(const F32& x, int top, int left, int H, const BatchPlanes<T>& dst, const BatchPlanes<const T>& ref, int b,
                                          int i, int x0, int n, const Levels& lv, const EmitCoef& k, unsigned long long su[3])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;
    const int nc = (n + 1) >> 1;
    const int rows = min(2, H - 2 * i);                       // 1 at the odd last row
    unsigned yq[2][COLS], cq[2][4];
    float ub[2][COLS], ur[2][COLS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int yy = min(2 * i + r, H - 1);                 // the last row stands in for the one below it
        float c[3][COLS];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = x.p + b * x.st + ch * x.sc + (int64_t)(top + yy) * x.sh + left + x0;
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
        for (int q = 0; q < COLS; ++q) emit_px(c[0][q], c[1][q], c[2][q], lv, k, yq[r][q], ub[r][q], ur[r][q]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cq[0][j] = (unsigned)emit_chroma(ub[0][2 * j], ub[0][2 * j + 1], ub[1][2 * j], ub[1][2 * j + 1], lv);
        cq[1][j] = (unsigned)emit_chroma(ur[0][2 * j], ur[0][2 * j + 1], ur[1][2 * j], ur[1][2 * j + 1], lv);
    }
    if (dst.y) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r < rows) {
                T* d = dst.y + b * dst.yb + (int64_t)(2 * i + r) * dst.yr + x0;
                if (FULL) {
                    unsigned w[COLS];
#pragma unroll
                    for (int q = 0; q < COLS; ++q) w[q] = yq[r][q] << SH;
                    store4(d, w);
                    store4(d + 4, w + 4);
                } else {
#pragma unroll
                    for (int q = 0; q < COLS; ++q)
                        if (q < n) d[q] = (T)(yq[r][q] << SH);
                }
            }
        }
        T* du = dst.u + b * dst.ub + (int64_t)i * dst.ur + CS * (int64_t)(x0 >> 1);
        T* dv = IL ? du + 1 : dst.v + b * dst.vb + (int64_t)i * dst.vr + (x0 >> 1);
        if (FULL) {
            if (IL) {
                unsigned w[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[2 * j] = cq[0][j] << SH; w[2 * j + 1] = cq[1][j] << SH; }
                store4(du, w);
                store4(du + 4, w + 4);
            } else {
                unsigned w[2][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[0][j] = cq[0][j] << SH; w[1][j] = cq[1][j] << SH; }
                store4(du, w[0]);
                store4(dv, w[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nc) { du[CS * j] = (T)(cq[0][j] << SH); dv[CS * j] = (T)(cq[1][j] << SH); }
        }
    }
    if (HAS_REF) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r < rows) {
                const T* s = ref.y + b * ref.yb + (int64_t)(2 * i + r) * ref.yr + x0;
                unsigned w[COLS];
                if (FULL) {
                    load4(s, w);
                    load4(s + 4, w + 4);
                } else {
#pragma unroll
                    for (int q = 0; q < COLS; ++q) w[q] = q < n ? (unsigned)s[q] : 0u;
                }
#pragma unroll
                for (int q = 0; q < COLS; ++q) {
                    if (q < n) {
                        const int e = (int)yq[r][q] - (int)(w[q] >> SH);
                        su[0] += (unsigned long long)(e * e);
                    }
                }
            }
        }
        const T* ru = ref.u + b * ref.ub + (int64_t)i * ref.ur + CS * (int64_t)(x0 >> 1);
        const T* rv = IL ? ru + 1 : ref.v + b * ref.vb + (int64_t)i * ref.vr + (x0 >> 1);
        unsigned w[2][4];
        if (FULL) {
            if (IL) {
                unsigned e[8];
                load4(ru, e);
                load4(ru + 4, e + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[0][j] = e[2 * j]; w[1][j] = e[2 * j + 1]; }
            } else {
                load4(ru, w[0]);
                load4(rv, w[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[0][j] = j < nc ? (unsigned)ru[CS * j] : 0u;
                w[1][j] = j < nc ? (unsigned)rv[CS * j] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nc) {
                const int eb = (int)cq[0][j] - (int)(w[0][j] >> SH), er = (int)cq[1][j] - (int)(w[1][j] >> SH);
                su[1] += (unsigned long long)(eb * eb);
                su[2] += (unsigned long long)(er * er);
            }
        }
    }
}

// Items are the eight-column groups of the WINDOW's row pairs: item -> (i, g), rows 2i and 2i+1, columns 8g .. 8g+7 of the picture,
// chroma row i, columns 4g .. 4g+3.  G = ceil(W / 8), items = Hc * G per picture.  partials: [gridDim.x][3].
template <class T, bool IL, bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void emit_kernel(F32 x, int top, int left, int H, int W, BatchPlanes<T> dst, BatchPlanes<const T> ref, int G,
                                                  int items, int blocks, Levels lv, EmitCoef k,
                                                  unsigned long long* __restrict__ partials)
{
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    const int item = blk * NT + threadIdx.x;
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    if (item < items) {
        const int i = item / G, g = item - i * G;
        const int x0 = COLS * g, n = min(COLS, W - x0);           // n luma columns exist
        if (WIDE && n == COLS) emit_item<T, IL, true, HAS_REF>(x, top, left, H, dst, ref, b, i, x0, n, lv, k, su);
        else emit_item<T, IL, false, HAS_REF>(x, top, left, H, dst, ref, b, i, x0, n, lv, k, su);
    }
    if (HAS_REF) block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One block per picture: its block partials (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void emit_final_kernel(const unsigned long long* __restrict__ partials, int blocks,
                                                        unsigned long long* __restrict__ sse)
{
    const int b = blockIdx.x;
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    gather_partials<Sum>(partials + (int64_t)b * blocks * 3, 0, blocks, (int)threadIdx.x, NT, su);
    block_reduce<Sum>(su, sse + b * 3);
}

// One plane of B pictures of `rows` rows of `len` elements: pointer aligned to its element, strides in range; `disjoint`
// (destinations): rows inside pictures, which is sufficient (not necessary) for no element of the plane to be written twice.
bool batch_plane_ok(const void* p, int64_t sb, int64_t sr, int es, int B, int rows, int64_t len, bool disjoint)
{
    if (!p || reinterpret_cast<uintptr_t>(p) % es || sr < len || sb < 1) return false;
    if (disjoint && B > 1 && sb < (int64_t)(rows - 1) * sr + len) return false;
    return true;
}

bool batch_frame_ok(int fmt, const pc_frame* f, int B, int H, int W, bool disjoint)
{
    if (!f || !fmt_ok(fmt)) return false;
    const int es = elem_bytes(fmt), Hc = (int)cdiv(H, 2);
    const int64_t Wc = cdiv(W, 2);
    if (!batch_plane_ok(f->y, f->y_batch, f->y_row, es, B, H, W, disjoint)) return false;
    if (interleaved(fmt)) return batch_plane_ok(f->u, f->u_batch, f->u_row, es, B, Hc, 2 * Wc, disjoint);
    return batch_plane_ok(f->u, f->u_batch, f->u_row, es, B, Hc, Wc, disjoint) && batch_plane_ok(f->v, f->v_batch, f->v_row, es, B, Hc, Wc, disjoint);
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
bool batch_frame_wide(int fmt, const pc_frame* f)
{
    const uintptr_t a = 4 * (uintptr_t)elem_bytes(fmt);
    if (reinterpret_cast<uintptr_t>(f->y) % a || !mult4(f->y_batch) || !mult4(f->y_row)) return false;
    if (reinterpret_cast<uintptr_t>(f->u) % a || !mult4(f->u_batch) || !mult4(f->u_row)) return false;
    if (!interleaved(fmt) && (reinterpret_cast<uintptr_t>(f->v) % a || !mult4(f->v_batch) || !mult4(f->v_row))) return false;
    return true;
}

// The one place that decides the access path: the calls launch from it, pc_frames_plan reports it.
bool wide_path(int op, int fmt, const pc_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh, int left,
               const pc_frame* ref)
{
    if (!f32_wide(f32, fb, fc, fh)) return false;
    if (op == PC_FRAMES_INGEST) return fh % 8 == 0 && left % 8 == 0 && batch_frame_wide(fmt, frame);     // fh = Wp: no partial last item
    return left % 4 == 0 && (!frame || batch_frame_wide(fmt, frame)) && (!ref || batch_frame_wide(fmt, ref));
}

bool window_ok(int B, int H, int W, int Hp, int Wp, int top, int left)
{
    if (B < 1 || H < 1 || W < 1 || top < 0 || left < 0 || Hp < 1 || Wp < 1) return false;
    return (int64_t)top + H <= Hp && (int64_t)left + W <= Wp;
}

template <class T>
BatchPlanes<T> batch_planes_of(const pc_frame* f)
{
    if (!f) return BatchPlanes<T>{nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0};
    return BatchPlanes<T>{static_cast<T*>(f->y), f->y_batch, f->y_row, static_cast<T*>(f->u), f->u_batch, f->u_row, static_cast<T*>(f->v),
                          f->v_batch, f->v_row};
}

template <class T, bool IL>
void launch_ingest(bool wide, dim3 grid, hipStream_t st, const pc_frame* src, int H, int W, float* dst, int Hp, int Wp, int top, int left,
                   const Items& g, int linear, const Levels& lv, const IngestCoef& k)
{
    const BatchPlanes<const T> s = batch_planes_of<const T>(src);
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    if (wide)
        hipLaunchKernelGGL((ingest_kernel<T, IL, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, dst, Hp, Wp, top, left, g.G, g.items,
                           g.blocks, linear, lv, k);
    else
        hipLaunchKernelGGL((ingest_kernel<T, IL, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, dst, Hp, Wp, top, left, g.G, g.items,
                           g.blocks, linear, lv, k);
}

template <class T, bool IL>
void launch_emit(bool wide, bool has_ref, dim3 grid, hipStream_t st, const F32& x, int top, int left, int H, int W, const pc_frame* dst,
                 const pc_frame* ref, const Items& g, const Levels& lv, const EmitCoef& k, unsigned long long* part)
{
    const BatchPlanes<T> d = batch_planes_of<T>(dst);
    const BatchPlanes<const T> r = batch_planes_of<const T>(ref);
#define PC_EMIT(WIDE, REF)                                                                                                            \
    hipLaunchKernelGGL((emit_kernel<T, IL, WIDE, REF>), grid, dim3(NT), 0, st, x, top, left, H, W, d, r, g.G, g.items, g.blocks, lv, k, \
                       part)
    if (has_ref) {
        if (wide) PC_EMIT(true, true); else PC_EMIT(false, true);
    } else {
        if (wide) PC_EMIT(true, false); else PC_EMIT(false, false);
    }
#undef PC_EMIT
}

}  // namespace

extern "C" int pc_frames_plan(int op, int fmt, const pc_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh, int left,
                              const pc_frame* ref, int* wide)
{
    if ((op != PC_FRAMES_INGEST && op != PC_FRAMES_EMIT) || !fmt_ok(fmt) || !f32 || !wide || left < 0) return PC_ERR_ARG;
    if (op == PC_FRAMES_INGEST) ref = nullptr;
    if (!frame && (op != PC_FRAMES_EMIT || !ref)) return PC_ERR_ARG;
    for (const pc_frame* f : {frame, ref})
        if (f && !planes_set(fmt, f)) return PC_ERR_ARG;
    *wide = wide_path(op, fmt, frame, f32, fb, fc, fh, left, ref) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_frames_ingest(const pc_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int B, int H,
                                int W, float* dst, int Hp, int Wp, int top, int left, void* stream)
{
    Items g;
    Levels lv;
    if (!dst || !aligned(dst, 4) || !window_ok(B, H, W, Hp, Wp, top, left)) return PC_ERR_ARG;
    if (!batch_frame_ok(fmt, src, B, H, W, false) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!upsample_ok(upsample)) return PC_ERR_ARG;
    if (!items_of(B, Hp, Wp, g)) return PC_ERR_ARG;
    const int64_t plane = (int64_t)Hp * Wp;
    const bool wide = wide_path(PC_FRAMES_INGEST, fmt, src, dst, 3 * plane, plane, Wp, left, nullptr);
    const IngestCoef k{a, b, c, d};
    const int linear = upsample == PC_FRAMES_LINEAR;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks));
    if (fmt == PC_FRAMES_NV12) launch_ingest<uint8_t, true>(wide, grid, st, src, H, W, dst, Hp, Wp, top, left, g, linear, lv, k);
    else if (fmt == PC_FRAMES_I420) launch_ingest<uint8_t, false>(wide, grid, st, src, H, W, dst, Hp, Wp, top, left, g, linear, lv, k);
    else launch_ingest<uint16_t, true>(wide, grid, st, src, H, W, dst, Hp, Wp, top, left, g, linear, lv, k);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_frames_emit_workspace_size(int B, int H, int W)
{
    Items g;
    return H >= 1 && items_of(B, (int)cdiv(H, 2), W, g) ? (size_t)B * g.blocks * 3 * sizeof(unsigned long long) : 0;
}

extern "C" int pc_frames_emit(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H,
                              int W, int fmt, int range, float kr, float kg, float kb, float ib, float ir, const pc_frame* dst,
                              const pc_frame* ref, void* workspace, size_t workspace_bytes, uint64_t* sse, void* stream)
{
    Items g;
    Levels lv;
    if (!x || !aligned(x, 4) || !window_ok(B, H, W, Hp, Wp, top, left)) return PC_ERR_ARG;
    if (sxh < Wp || sxc < 1 || sxb < 1 || !fmt_ok(fmt) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!dst && !ref) return PC_ERR_ARG;
    if (dst && !batch_frame_ok(fmt, dst, B, H, W, true)) return PC_ERR_ARG;
    if (ref && !batch_frame_ok(fmt, ref, B, H, W, false)) return PC_ERR_ARG;
    if (!items_of(B, (int)cdiv(H, 2), W, g)) return PC_ERR_ARG;
    if (ref) {
        if (!workspace || !aligned(workspace, 8) || !sse || !aligned(sse, 8)) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)B * g.blocks * 3 * sizeof(unsigned long long)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_FRAMES_EMIT, fmt, dst, x, sxb, sxc, sxh, left, ref);
    const F32 xv{x, sxb, sxc, sxh};
    const EmitCoef k{kr, kg, kb, ib, ir};
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks));
    if (fmt == PC_FRAMES_NV12) launch_emit<uint8_t, true>(wide, ref != nullptr, grid, st, xv, top, left, H, W, dst, ref, g, lv, k, part);
    else if (fmt == PC_FRAMES_I420) launch_emit<uint8_t, false>(wide, ref != nullptr, grid, st, xv, top, left, H, W, dst, ref, g, lv, k, part);
    else launch_emit<uint16_t, true>(wide, ref != nullptr, grid, st, xv, top, left, H, W, dst, ref, g, lv, k, part);
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(emit_final_kernel, dim3((unsigned)B), dim3(NT), 0, st, part, g.blocks, reinterpret_cast<unsigned long long*>(sse));
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_frames_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG: return "invalid argument, unknown format, unsupported shape or workspace too small (pc_frames_emit_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_frames_last_hip_error(void) { return g_last_hip.load(); }
