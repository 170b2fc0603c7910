// mmw_normalize.hpp -- what the kernels that produce ring rows share: Utils.normalize_data on R raw rows per thread
// (k_normalize, k_normalize_tlv: k_misc.hip; k_uart_read: k_uart.hip), the decode of one detected-points object and the
// site's mounting in place of the context's.  One body each: the operation order is what pins the rows to the reference bit for bit.
#pragma once

#include "mmw_device.hpp"
#include "mmw_math.hpp"

namespace mmw {

// The body both entries share: R raw rows (x, y, z, doppler, peakVal as doubles) of this thread -> the reference's arithmetic ->
// ordered compaction -> whole-row stores.  All 256 threads of the workgroup call (one barrier).
template <int R>
__device__ __forceinline__ void normalize_rows(const DevCfg &cfg, int s, int n, const double (&v)[R][5], double *__restrict__ out,
                                               int32_t *__restrict__ n_out, int *wcnt /* LDS [R * 4] */)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *dst = out + (size_t)s * cfg.max_pts * 8;
    double o[R][8];
    unsigned long long bal[R];
#pragma unroll
    for (int q = 0; q < R; q++) {
        const int i = q * 256 + tid;
        const double x = v[q][0], y = v[q][1], z = v[q][2], dop = v[q][3], pk = v[q][4];
        const double r = sqrt((x * x + y * y) + z * z);
        double vx, vy, vz;
        if (r == 0) { vx = 0; vy = dop; vz = 0; }           // Utils.py:387-390
        else { vx = dop * x / r; vy = dop * y / r; vz = dop * z / r; }
        o[q][0] = x;                                         // T . R_inv . [x,y,z,1]  (Utils.py:312-328)
        o[q][1] = cfg.tilt_cos * y + (-cfg.tilt_sin) * z;
        o[q][2] = (cfg.tilt_sin * y + cfg.tilt_cos * z) + cfg.s_height;
        o[q][3] = vx;
        o[q][4] = cfg.tilt_cos * vy + (-cfg.tilt_sin) * vz;
        o[q][5] = cfg.tilt_sin * vy + cfg.tilt_cos * vz;
        o[q][6] = dop;
        o[q][7] = pk;
        {   // Non-finite rows.  The reference multiplies full homogeneous 4-vectors by full 4 x 4 matrices, zeros included
            // (Utils.py:311-326): one NaN / infinite coordinate meets a zero (0 * inf = NaN) and makes all three transformed
            // coordinates NaN -- the filter below then drops the row (NaN compares false) --, one non-finite velocity component
            // (a NaN / infinite doppler) makes all three velocities NaN on a row that is kept.  Finite rows: nothing changes.
            constexpr int kNanInf = 0x3 | 0x4 | 0x200;
            const double qnan = __longlong_as_double(0x7ff8000000000000LL);
            if (__builtin_amdgcn_class(x, kNanInf) || __builtin_amdgcn_class(y, kNanInf) || __builtin_amdgcn_class(z, kNanInf)) o[q][0] = o[q][1] = o[q][2] = qnan;
            if (__builtin_amdgcn_class(vx, kNanInf) || __builtin_amdgcn_class(vy, kNanInf) || __builtin_amdgcn_class(vz, kNanInf)) o[q][3] = o[q][4] = o[q][5] = qnan;
        }
        const bool keep = i < n && o[q][2] <= 2.5 && o[q][2] > 0 && o[q][1] > 0;   // Utils.py:423-427
        bal[q] = __ballot(keep);
        if (lane == 0) wcnt[q * 4 + wave] = __popcll(bal[q]);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int q = 0; q < R; q++) {
        int off = total;                                     // rows kept in the 64-row blocks before this one (blocks are in row order)
#pragma unroll
        for (int w = 0; w < 4; w++) { const int c = wcnt[q * 4 + w]; if (w < wave) off += c; total += c; }
        if ((bal[q] >> lane) & 1ULL) {
            double2 *d = reinterpret_cast<double2 *>(dst + (size_t)(off + __popcll(bal[q] & lanemask_lt())) * 8);   // (whole rows: 16-byte stores)
#pragma unroll
            for (int u = 0; u < 4; u++) d[u] = double2{o[q][2 * u], o[q][2 * u + 1]};
        }
    }
    if (tid == 0) n_out[s] = total;
}

// One object of the detected-points TLV, its six little-endian u16 words (rangeIdx, dopplerIdx, peakVal, x, y, z) -> the raw row
// (x, y, z, doppler, peakVal) as ReadIWR14xx.read makes it (ReadDataIWR1443.py:150-171): doppler indices above half_bins =
// numDopplerBins / 2 - 1 get 65535 subtracted in int16, q = xyz_q_divisor(xyzQFormat).
__device__ __forceinline__ void decode_tlv_object(const unsigned short (&w)[6], double q, double half_bins, double doppler_res, double (&v)[5])
{
    short dop = (short)w[1];
    if ((double)dop > half_bins) dop = (short)((int)dop - 65535);   // ReadDataIWR1443.py:150-157 (wraps in int16)
    v[0] = (double)(short)w[3] / q;
    v[1] = (double)(short)w[4] / q;
    v[2] = (double)(short)w[5] / q;
    v[3] = (double)dop * doppler_res;
    v[4] = (double)(short)w[2];
}

// Per-scene sites (mmw_set_sites): a kernel's `cfg` with the site's values in place of the context's, so that a kernel's SITE = true
// instantiation runs the SAME body as its SITE = false one, the plain kernel -- the operation order of normalize_rows, features_scene and table_slot (which takes the window as scalars) is what pins them to the
// reference bit for bit.  The table is written by an earlier call on the same stream, never by the launch that reads it: it
// may come through the scalar cache, and needs no invalidate (unlike the gate records of k_track).
// Mounting (k_normalize*, k_uart_read): one workgroup is one scene, so the site is wave-uniform -- `site` is sites + blockIdx.x of a
// const __restrict__ kernel argument and arrives as scalar operands (s_load), like DevCfg itself.
__device__ __forceinline__ DevCfg cfg_with_mounting(DevCfg cfg, const mmw_scene_site *__restrict__ site)
{
    cfg.s_height = site->s_height;
    cfg.tilt_cos = site->tilt_cos;
    cfg.tilt_sin = site->tilt_sin;
    return cfg;
}
}  // namespace mmw
