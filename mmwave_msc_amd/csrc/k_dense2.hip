// k_dense2.hip -- the two kernels the batched estimate_posture of the C-ABI (mmw_posture_attach / mmw_estimate_posture) adds to
// the CNN chain of k_mars.hip / k_dense.hip:
//
//   k_mars_dense2     Dense-2 of define_CNN_3D (train.py:92; BatchNormalization folded in): kp[n][57] = bias2 + hidden[n][K] . w2[57][K]^T
//                     in fp32 on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, one rounding per
//                     product), fp32 out.
//   k_split_weights   fp32 w[n][ldw] -> the split-fp16 operand of k_mars_dense1 (k_dense.hip), what mars.interleave_split builds with
//                     torch: hi = fp16(a), lo' = fp16((a - hi) * 2^11), stored in runs of [hi 32 | lo' 32].
//   k_range_check     the range word of k_split_weights for arrays that are not split ahead of time (the conv kernels and biases:
//                     k_mars_conv16 splits them as it stages them).
//
// k_mars_dense2 is a stream over `hidden`: at the end-to-end workload (31.7 k rows, K = 1536) it reads 195 MB of activations once and
// 350 KB of weights, and does 6.2 GFLOP -- 31 us at the HBM copy rate, 40 us on the fp32 matrix cores (64 FLOP per clock and SIMD: a
// 32-row tile per SIMD, 992 tiles on 1024 SIMDs).  So: a workgroup of four waves owns 128 rows, one 32-row tile per wave against all
// 64 (57 padded) columns = two 32x32 output tiles; K is walked in chunks of 32, each chunk of the 128 x 32 activation tile and the
// 64 x 32 weight tile loaded with 16-byte loads that cover whole 128-byte lines (eight lanes per row), parked in registers while the
// previous chunk is multiplied, and handed over through a double-buffered LDS image: `hidden` is read exactly once, the weights come
// out of the L2 (one 8 KB chunk per workgroup and step).  Rows are 36 floats apart in LDS: the ds_read_b128 of the sixteen lanes
// that are serviced together (sixteen distinct rows mod 16, one k offset) then falls into sixteen different 4-bank slots.
//
// Operand maps (v_mfma_f32_32x32x2_f32): lane l gives A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31].  A lane reads ONE
// float4 per operand and 8-deep step -- floats 8s + 4h .. + 3 of its row, h = l >> 5 -- and component j feeds MFMA j of the step, so
// MFMA j sums k = 8s + j, then k = 8s + 4 + j, into accumulator j: four chains over k = j, 4 + j, 8 + j ... that are added as
// (0 + 1) + (2 + 3) in the epilogue.  The order of the sum is therefore fixed per output, the same for every row, batch size and
// run (no atomics, no split over workgroups): GPU == GPU.
// A row only ever meets its own accumulator rows: a NaN in one sample stays in that sample's keypoints.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmw_kernels.hpp"

namespace mmw {

namespace dense2 {
constexpr int kRows = 128, kCols = 64, kKC = 32, kLd = kKC + 4, kThreads = 256, kOut = 57;
}
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(dense2::kThreads) void k_mars_dense2(const float *__restrict__ hidden, long long ldh, const float *__restrict__ w2,
                                                                  const float *__restrict__ bias2, float *__restrict__ kp, int n_rows, int K)
{
    using namespace dense2;
    __shared__ __attribute__((aligned(16))) float sA[2][kRows * kLd];
    __shared__ __attribute__((aligned(16))) float sB[2][kCols * kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long row_base = (long long)blockIdx.x * kRows;
    // loader: eight lanes per row (one 128-byte line), 32 rows per pass; the tile's rows past n_rows, the weight rows past 57 and a
    // last chunk's floats past K are zeros (never read from memory)
    const int lrow = tid >> 3, lk = (tid & 7) * 4;
    float4 ra[4], rb[2];
    auto fetch = [&](int k0) {
        const bool kin = k0 + lk < K;   // (K is a multiple of 4: a float4 is inside or outside as a whole)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const long long row = row_base + lrow + 32 * i;
            ra[i] = (kin && row < n_rows) ? *reinterpret_cast<const float4 *>(hidden + row * ldh + k0 + lk) : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int col = lrow + 32 * i;
            rb[i] = (kin && col < kOut) ? *reinterpret_cast<const float4 *>(w2 + (long long)col * K + k0 + lk) : float4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<float4 *>(&sA[buf][(lrow + 32 * i) * kLd + lk]) = ra[i];
#pragma unroll
        for (int i = 0; i < 2; i++) *reinterpret_cast<float4 *>(&sB[buf][(lrow + 32 * i) * kLd + lk]) = rb[i];
    };
    // Four accumulators per 32-column tile, one per float4 component: four interleaved chains of K / 4 terms instead of one of K
    // (the rounding error of an fp32 chain grows with its length), summed pairwise at the end.  The first starts as the bias of
    // its column (C/D map: column = lane & 31 in every register).
    const float b0 = bias2[r], b1 = (32 + r < kOut) ? bias2[32 + r] : 0.f;
    f32x16 acc0[4], acc1[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 16; i++) { acc0[j][i] = j == 0 ? b0 : 0.f; acc1[j][i] = j == 0 ? b1 : 0.f; }
    const int chunks = (K + kKC - 1) / kKC;
    fetch(0);
    park(0);
    __syncthreads();
    for (int ch = 0; ch < chunks; ch++) {
        const int buf = ch & 1;
        if (ch + 1 < chunks) fetch((ch + 1) * kKC);   // in flight while this chunk is multiplied
        const float *a_row = &sA[buf][(wave * 32 + r) * kLd + 4 * h];
        const float *b_row0 = &sB[buf][r * kLd + 4 * h], *b_row1 = &sB[buf][(32 + r) * kLd + 4 * h];
#pragma unroll
        for (int s = 0; s < kKC / 8; s++) {
            const float4 a = *reinterpret_cast<const float4 *>(a_row + 8 * s);
            const float4 p = *reinterpret_cast<const float4 *>(b_row0 + 8 * s), q = *reinterpret_cast<const float4 *>(b_row1 + 8 * s);
            acc0[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, p.x, acc0[0], 0, 0, 0);
            acc1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q.x, acc1[0], 0, 0, 0);
            acc0[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, p.y, acc0[1], 0, 0, 0);
            acc1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q.y, acc1[1], 0, 0, 0);
            acc0[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, p.z, acc0[2], 0, 0, 0);
            acc1[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q.z, acc1[2], 0, 0, 0);
            acc0[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, p.w, acc0[3], 0, 0, 0);
            acc1[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q.w, acc1[3], 0, 0, 0);
        }
        // the other buffer was last read in the step before this one, which ended in a barrier
        if (ch + 1 < chunks) park(buf ^ 1);
        __syncthreads();
    }
    // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Rows past n_rows are never written.
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const long long row = row_base + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (row < n_rows) {
            kp[row * kOut + r] = (acc0[0][i] + acc0[1][i]) + (acc0[2][i] + acc0[3][i]);
            if (32 + r < kOut) kp[row * kOut + 32 + r] = (acc1[0][i] + acc1[1][i]) + (acc1[2][i] + acc1[3][i]);
        }
    }
}

void launch_mars_dense2(const float *hidden, long long ldh, const float *w2, const float *bias2, float *kp, int n_rows, int K, hipStream_t stream)
{
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(k_mars_dense2, dim3((n_rows + dense2::kRows - 1) / dense2::kRows), dim3(dense2::kThreads), 0, stream, hidden, ldh, w2, bias2, kp,
                       n_rows, K);
}

// The split of k_mars.hip (split16) on a whole matrix: exact inside fp16's range only, so a value of magnitude >= 65 504 or one that
// is not finite raises bit 0 of *range_flag (its halves are what the conversions give: inf and -inf / NaN).
constexpr float kSplitScale2 = 2048.0f;   // 2^11
__device__ __forceinline__ bool outside_fp16(float a) { return !(fabsf(a) < 65504.0f); }

// One thread per 8 consecutive values of a row: two 16-byte loads, the eight hi halves as one 16-byte store at (j / 32) * 64 + j % 32
// of the row, the eight lo' halves 32 further.
__global__ __launch_bounds__(256) void k_split_weights(const float *__restrict__ w, long long ldw, _Float16 *__restrict__ w16, long long ld16, int n,
                                                       int k, int32_t *__restrict__ range_flag)
{
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));
    const long long per_row = k / 8, g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= per_row * n) return;
    const long long row = g / per_row;
    const int j0 = (int)(g - row * per_row) * 8;
    const float4 u = *reinterpret_cast<const float4 *>(w + row * ldw + j0), v = *reinterpret_cast<const float4 *>(w + row * ldw + j0 + 4);
    const float a[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    half8 hi, lo;
    bool over = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        over |= outside_fp16(a[i]);
        const _Float16 t = (_Float16)a[i];
        hi[i] = t;
        lo[i] = (_Float16)((a[i] - (float)t) * kSplitScale2);
    }
    _Float16 *dst = w16 + row * ld16 + (j0 / 32) * 64 + (j0 % 32);
    *reinterpret_cast<half8 *>(dst) = hi;
    *reinterpret_cast<half8 *>(dst + 32) = lo;
    if (over && range_flag) atomicOr(range_flag, 1);
}

__global__ __launch_bounds__(256) void k_range_check(const float *__restrict__ a, long long count, int32_t *__restrict__ range_flag)
{
    bool over = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) over |= outside_fp16(a[i]);
    if (over) atomicOr(range_flag, 1);
}

void launch_split_weights(const float *w, long long ldw, void *w16, long long ld16, int n, int k, int32_t *range_flag, hipStream_t stream)
{
    const long long items = (long long)n * (k / 8);
    if (items <= 0) return;
    hipLaunchKernelGGL(k_split_weights, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, w, ldw, reinterpret_cast<_Float16 *>(w16), ld16, n, k,
                       range_flag);
}

void launch_range_check(const float *a, long long count, int32_t *range_flag, hipStream_t stream)
{
    if (count <= 0) return;
    const long long blocks = (count + 255) / 256;
    hipLaunchKernelGGL(k_range_check, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, a, count, range_flag);
}

}  // namespace mmw
