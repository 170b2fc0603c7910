// k_mars2d.hip -- the two Conv2D layers of the single-frame MARS regressor (reference src/train.py:35-44, define_CNN:
// Conv2D(16,3x3,same,relu) -> Conv2D(32,3x3,same,relu)) fused in one kernel on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x2_f32: exact f32 fma chains) -- the single-frame counterpart of k_mars_conv
// (k_mars.hip), which hard-codes the 5 x 10 x 10 volume of define_CNN_3D.
//
// Per sample the work is two implicit GEMMs over ONE zero-padded 10 x 10 plane per channel, kept in LDS:
//   conv1: [64 positions] x [K = 9 taps x 5 ch = 45 -> 48] x [16 out]     0.09 MFLOP   four 16-position tiles
//   conv2: [64 positions] x [K = 9 taps x 16 ch = 144] x [32 out]         0.59 MFLOP   two 32-position tiles
// A workgroup is two waves sharing one sample (two conv1 tiles and one conv2 tile each) and loops over samples; conv2's weights
// live in registers as MFMA B operands for the whole kernel (72 VGPRs per lane), conv1's in LDS; the A operands are single
// ds_read_b32 per MFMA from the padded plane (tap and channel offsets are immediates), the intermediate activation never leaves LDS.
// Input = mmw_features' channels-last tensor at ring 1, [n][8][8][5]; output [n][64][32] is the Keras Flatten order (h,w,c), so
// Dense-1 takes Keras' weight rows as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmw_kernels.hpp"

namespace mmw {

namespace conv2d {
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPP = 100;      // padded plane 10 x 10 per channel
constexpr int kIn = 11;       // the interior starts at (1,1)
constexpr int kK1 = 12;       // conv1 k-steps of 4 (45 -> 48)
constexpr int kK2 = 72;       // conv2 k-steps of 2 (144)
constexpr int kPer = 64 * 5, kFlat = 64 * 32;

__device__ __forceinline__ int padded_origin(int pos)  // position (h,w) -> index of its (kh,kw)=(0,0) tap
{
    return (pos >> 3) * 10 + (pos & 7);
}
constexpr int tap_off(int tap) { return (tap / 3) * 10 + tap % 3; }
__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }   // (NaN stays NaN, as Keras')
}  // namespace conv2d

__global__ __launch_bounds__(128) void k_mars_conv2d(const float *__restrict__ feat, const float *__restrict__ w1, const float *__restrict__ b1,
                                                     const float *__restrict__ w2, const float *__restrict__ b2, float *__restrict__ out, int B,
                                                     const int32_t *__restrict__ dev_rows)
{
    using namespace conv2d;
    // (dev_rows: a row count that only the device knows -- the range fix-up's flagged samples, the one-scene chain's eligible
    //  tracks: workgroups past it leave at once)
    if (dev_rows != nullptr) B = dev_rows[0] < B ? dev_rows[0] : B;
    if ((int)blockIdx.x >= B) return;
    __shared__ float Xp[5 * kPP];         // input, channel-major, zero border
    __shared__ float H1[16 * kPP];        // relu(conv1), channel-major, zero border
    __shared__ float W1s[4 * kK1 * 16];   // conv1 kernel [k = tap*5+ic][oc], rows 45..47 = zero padding of K
    __shared__ int A1s[4 * kK1];          // LDS offset of tap/channel k relative to a position's origin
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < 5 * kPP; i += 128) Xp[i] = 0.f;
    for (int i = tid; i < 16 * kPP; i += 128) H1[i] = 0.f;

    // ---- weights as MFMA B operands, resident for the whole kernel ----
    // conv2 (32x32x2): lane l holds B[k = 2*ks + (l>>5)][oc = l&31], k = tap*16 + ic  (Keras kernel (kh,kw,in,out))
    float w2r[kK2];
#pragma unroll
    for (int ks = 0; ks < kK2; ks++) w2r[ks] = w2[(2 * ks + (lane >> 5)) * 32 + (lane & 31)];
    // conv1 (16x16x4): lane l needs B[k = 4*ks + (l>>4)][oc = l&15], k = tap*5 + ic (k = 45..47 pad K: zero weights, and the
    // offset of a cell of the position's own receptive field); weights and offset table stay in LDS
    for (int i = tid; i < 4 * kK1 * 16; i += 128) W1s[i] = i < 45 * 16 ? w1[i] : 0.f;
    if (tid < 4 * kK1) {
        const bool real = tid < 45;
        const int tap = real ? tid / 5 : 0, ic = real ? tid - 5 * tap : 0;
        A1s[tid] = ic * kPP + tap_off(tap);
    }
    const float bias1 = b1[lane & 15], bias2 = b2[lane & 31];
    // conv2 A operand: lane l reads channel (2*ks)%16 + (l>>5) at position (wave*32 + (l&31)) shifted by the tap
    const int a2base = (lane >> 5) * kPP + padded_origin(wave * 32 + (lane & 31));
    __syncthreads();

    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        // ---- input sample (channels-last [64][5]) into the padded planes ----
        const float *x = feat + (size_t)b * kPer;
        for (int e = tid; e < kPer; e += 128) {
            const int pos = e / 5, c = e - pos * 5;
            Xp[c * kPP + padded_origin(pos) + kIn] = x[e];
        }
        __syncthreads();
        // ---- conv1 + bias + relu -> H1 : 4 tiles of 16 positions, 2 per wave, as two independent accumulator chains ----
        {
            const int aorg0 = padded_origin((wave * 2) * 16 + (lane & 15)), aorg1 = padded_origin((wave * 2 + 1) * 16 + (lane & 15));
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < kK1; ks++) {
                const int k = 4 * ks + (lane >> 4);
                const int ao = A1s[k];
                const float wv = W1s[k * 16 + (lane & 15)];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(Xp[ao + aorg0], wv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(Xp[ao + aorg1], wv, acc1, 0, 0, 0);
            }
            // C/D: col = lane&15 (out channel), row = (lane>>4)*4 + reg (position in tile)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int p0 = (wave * 2) * 16 + (lane >> 4) * 4 + r;
                const float v0 = acc0[r] + bias1, v1 = acc1[r] + bias1;
                H1[(lane & 15) * kPP + padded_origin(p0) + kIn] = relu(v0);
                H1[(lane & 15) * kPP + padded_origin(p0 + 16) + kIn] = relu(v1);
            }
        }
        __syncthreads();
        // ---- conv2 + bias + relu -> out[b][pos][oc] : 2 tiles of 32 positions, 1 per wave ----
        f32x16 cc;
#pragma unroll
        for (int r = 0; r < 16; r++) cc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < kK2; ks++) {
            const int tap = (2 * ks) / 16, ic0 = (2 * ks) % 16;
            const int koff = ic0 * kPP + tap_off(tap);  // compile-time constant
            cc = __builtin_amdgcn_mfma_f32_32x32x2f32(H1[a2base + koff], w2r[ks], cc, 0, 0, 0);
        }
        // C/D: col = lane&31 (out channel), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
        float *o = out + (size_t)b * kFlat;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(wave * 32 + row) * 32 + (lane & 31)] = relu(cc[r] + bias2);
        }
        __syncthreads();  // both waves are done reading Xp / H1 before the next sample overwrites them
    }
}

void launch_mars_conv2d(const float *feat, const float *w1, const float *b1, const float *w2, const float *b2, float *out, int B,
                        hipStream_t stream, const int32_t *dev_rows)
{
    if (B <= 0) return;
    const int grid = B < 1024 ? B : 1024;  // 4 workgroups per CU (11.4 KB of LDS, two waves each), persistent over samples
    hipLaunchKernelGGL(k_mars_conv2d, dim3(grid), dim3(128), 0, stream, feat, w1, b1, w2, b2, out, B, dev_rows);
}

void launch_mars_conv_f32(int frames, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2, float *out, int B,
                          hipStream_t stream, const int32_t *dev_rows)
{
    if (frames == 3) launch_mars_conv(feat, w1, b1, w2, b2, out, B, stream, dev_rows);
    else launch_mars_conv2d(feat, w1, b1, w2, b2, out, B, stream, dev_rows);
}

}  // namespace mmw
