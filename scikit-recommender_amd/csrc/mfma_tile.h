// mfma_tile.h -- the device helpers the model kernels share around v_mfma_f32_16x16x4_f32 (exact fp32 operands): a
// wavefront owns a 16-row tile of A, the B tile lies in LDS, and four accumulators hold a 16 x 64 result.
//
// Lane (r, g) of a wavefront is r = lane & 15, g = lane >> 4.  One MFMA step sums over four k, one per 16-lane group g: the
// lane hands in A[row r][k] and B[row 16 nb + r][k] and receives, in acc[nb][rr], the result's row 4 g + rr, column
// 16 nb + r.  Which k a lane carries in step kk is the caller's choice, as long as A and B agree.  Two mappings are in use:
//
//   k = K g + kk   a lane's K steps read K CONSECUTIVE floats of an operand row: K / 4 16-byte LDS reads instead of K
//                  4-byte ones, and A operands come straight from global rows as float4.  load_row_a, load_slab,
//                  column_sum's images and tile_product.  K = 16 (a whole 64-float row per pass) in bm3.hip, selfcf.hip
//                  and dens.hip; K = 8 (a 32-feature chunk) in knn.hip.
//   k = 4 kk + g   the four groups read four neighbouring floats: the same LDS tile serves as B by rows (the logits) and
//                  by columns (the products from the transposed side).  load_a and logits_tile, over the tiles of
//                  tile_range and load_tile.  multvae.hip's decoder passes and lightgcl.hip's InfoNCE passes.
//
// Table rows are 64 floats.  LD is the row stride of an LDS image in floats.
#pragma once
#include "skr_common.h"

namespace skr {

using f32x4 = __attribute__((ext_vector_type(4))) float;

__host__ __device__ inline int64_t round4(int64_t x) { return (x + 3) & ~static_cast<int64_t>(3); }

// over the 16 lanes of a group g: every lane of the group gets the result
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float max16(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the sum of v over a workgroup of 1024 threads by a fixed tree, in every thread; s [1024] may be reused at once
__device__ __forceinline__ float block_sum_1024(float v, float* s) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) s[t] += s[t + o];
        __syncthreads();
    }
    return s[0];
}

__device__ __forceinline__ void zero_acc(f32x4 acc[4]) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

__device__ __forceinline__ int64_t checked(int id, int limit) { return id >= 0 && id < limit ? id : -1; }

// ---- k = K g + kk -------------------------------------------------------------------------------
// a[kk] = row[16 g + kk] of the table's row `node` (zeros for node < 0): the lane's share of an A operand
__device__ __forceinline__ void load_row_a(float a[16], const float* __restrict__ X, int64_t node, int g) {
    if (node < 0) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) a[kk] = 0.0f;
        return;
    }
    const float4* p = reinterpret_cast<const float4*>(X + node * 64 + 16 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = p[q];
        a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
}

// the same share of row `row` of an LDS image
template <int LD>
__device__ __forceinline__ void load_slab(float a[16], const float* __restrict__ s, int row, int g) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(s + row * LD + 16 * g + 4 * q);
        a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
}

// the sum of the 64 floats of row `col` of a transposed LDS image, in a fixed order
template <int LD>
__device__ __forceinline__ float column_sum(const float* __restrict__ sXT, int col) {
    float t = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(sXT + col * LD + 4 * q);
        t += (v.x + v.y) + (v.z + v.w);
    }
    return t;
}

// acc[nb][rr] += sum_k A[4 g + rr][k] * B[16 nb + r][k] over 4 K values of k: a[] the lane's share of A's row r, sB rows
// of stride LD
template <int LD, int K>
__device__ __forceinline__ void tile_product(f32x4 acc[4], const float (&a)[K], const float* __restrict__ sB, int r, int g) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        float4 w[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) w[nb] = *reinterpret_cast<const float4*>(sB + (nb * 16 + r) * LD + K * g + 4 * q);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 0], w[nb].x, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 1], w[nb].y, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 2], w[nb].z, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 3], w[nb].w, acc[nb], 0, 0, 0);
    }
}

// ---- k = 4 kk + g -------------------------------------------------------------------------------
// the tiles [t0, t1) of a persistent workgroup
__device__ __forceinline__ void tile_range(int tiles, int& t0, int& t1) {
    t0 = static_cast<int>(static_cast<int64_t>(blockIdx.x) * tiles / gridDim.x);
    t1 = static_cast<int>(static_cast<int64_t>(blockIdx.x + 1) * tiles / gridDim.x);
}

// W[row0 .. row0 + 64) into LDS by a workgroup of NW wavefronts, rows beyond the table as zeros
template <int LD, int NW>
__device__ __forceinline__ void load_tile(float* __restrict__ sW, const float* __restrict__ W, int row0, int n_rows) {
    const float4* W4 = reinterpret_cast<const float4*>(W);
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = threadIdx.x + i * NW * 64, row = idx >> 4, c4 = idx & 15;
        const int gr = row0 + row;
        v[i] = gr < n_rows ? W4[static_cast<int64_t>(gr) * 16 + c4] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = threadIdx.x + i * NW * 64, row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<float4*>(sW + row * LD + c4 * 4) = v[i];
    }
}

// the wavefront's rows qb .. qb + 15 of Q [n, 64] as the A operand of 16 k-steps: lane (r, g) holds Q[qb + r][4 kk + g]
__device__ __forceinline__ void load_a(float a[16], const float* __restrict__ Q, int qb, int n, int r, int g) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) a[kk] = qb + r < n ? Q[static_cast<int64_t>(qb + r) * 64 + 4 * kk + g] : 0.0f;
}

// acc[nb][rr] = <Q[row 4 g + rr], W[row 16 nb + r]>
template <int LD>
__device__ __forceinline__ void logits_tile(f32x4 acc[4], const float a[16], const float* __restrict__ sW, int r, int g) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], sW[(nb * 16 + r) * LD + 4 * kk + g], acc[nb], 0, 0, 0);
    }
}

// ---- float64 accumulators ------------------------------------------------------------------------
// The same fp32 operands in the same lanes, added on v_mfma_f64_16x16x4_f64 and rounded once by the caller: for the sums whose
// fp32 noise an optimiser magnifies (freedom.hip's weight gradient, mgcn.hip's products).  The lane's four results are the rows
// g + 4 rr -- not 4 g + rr -- of column 16 nb + r.
using f64x4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ void zero_acc64(f64x4 acc[4]) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = f64x4{0.0, 0.0, 0.0, 0.0};
}
__device__ __forceinline__ f64x4 mfma64(float a, float b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(static_cast<double>(a), static_cast<double>(b), c, 0, 0, 0);
}
__device__ __forceinline__ double sum16d(double v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// tile_product of mfma_tile.h with float64 accumulators: acc[nb][rr] += sum_k A[g + 4 rr][k] * B[16 nb + r][k]
template <int LDS, int K>
__device__ __forceinline__ void tile_product64(f64x4 acc[4], const float (&a)[K], const float* __restrict__ sB, int r, int g) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        float4 w[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) w[nb] = *reinterpret_cast<const float4*>(sB + (nb * 16 + r) * LDS + K * g + 4 * q);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a[4 * q + 0], w[nb].x, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a[4 * q + 1], w[nb].y, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a[4 * q + 2], w[nb].z, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a[4 * q + 3], w[nb].w, acc[nb]);
    }
}
// logits_tile of mfma_tile.h with float64 accumulators: acc[nb][rr] = <Q[row g + 4 rr], W[row 16 nb + r]>
template <int LDS>
__device__ __forceinline__ void logits_tile64(f64x4 acc[4], const float a[16], const float* __restrict__ sW, int r, int g) {
    zero_acc64(acc);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(a[kk], sW[(nb * 16 + r) * LDS + 4 * kk + g], acc[nb]);
    }
}

}  // namespace skr
