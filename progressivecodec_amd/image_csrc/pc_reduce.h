// pc_reduce.h -- the two-stage reduction of the image-side kernels: thread -> wave tree -> the block's waves in order through LDS
// -> one partial per block; then one wave (or one block) over the partials.  No atomics; every operand is an integer, so the result
// does not depend on the order.  N numbers are reduced side by side; Op says how number c combines (a compile-time policy: Sum for
// sums, or a library's own, such as clip_tol's sum / sum / max).  Include after pc_image_host.h.
#ifndef PC_REDUCE_H
#define PC_REDUCE_H

namespace {

constexpr int NT = 256;                  // threads per block (4 waves) of every image-side kernel

struct Sum {
    template <class V>
    static __device__ __forceinline__ V op(int, V a, V b) { return a + b; }
};

// lane 0 of each wave ends up with the wave's N numbers
template <class Op, class A, int N>
__device__ __forceinline__ void wave_reduce(A (&ac)[N])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const A o = __shfl_down(ac[c], off, 64);
            ac[c] = Op::op(c, ac[c], o);
        }
    }
}

// The N numbers of a block of NT threads -> out[0 .. N-1]: the wave tree, then thread c combines the waves' number c in order.
// Every thread of the block calls it (there is a barrier inside).
template <class Op, class A, int N>
__device__ __forceinline__ void block_reduce(A (&ac)[N], u64* __restrict__ out)
{
    __shared__ A red[NT / 64][N];
    wave_reduce<Op>(ac);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) red[threadIdx.x >> 6][c] = ac[c];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int c = threadIdx.x;
        u64 s = red[0][c];
        for (int wv = 1; wv < NT / 64; ++wv) s = Op::op(c, s, (u64)red[wv][c]);
        out[c] = s;
    }
}

// Row t of p, n partials of N numbers each, into ac (which the caller has set to the operation's zero), the calling threads taking
// partial first, first + step, ...; the caller reduces ac further.
template <class Op, int N>
__device__ __forceinline__ void gather_partials(const u64* __restrict__ p, int64_t t, int n, int first, int step, u64 (&ac)[N])
{
    for (int b = first; b < n; b += step) {
#pragma unroll
        for (int c = 0; c < N; ++c) ac[c] = Op::op(c, ac[c], p[(t * n + b) * N + c]);
    }
}

// The body of a kernel of one wave per row: row t = blockIdx.x of p, n partials of N numbers -> out[t * N .. t * N + N - 1].
template <class Op, int N>
__device__ __forceinline__ void row_final(const u64* __restrict__ p, int n, u64* __restrict__ out)
{
    const int64_t t = blockIdx.x;
    u64 ac[N] = {};
    gather_partials<Op>(p, t, n, (int)threadIdx.x, 64, ac);
    wave_reduce<Op>(ac);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) out[t * N + c] = ac[c];
    }
}

}  // namespace

#endif  // PC_REDUCE_H
