// k_sample.hip -- the training samples (mmw_samples_*): what preprocessing.py:192-220 saves of a scene after its track() -- when
// effective_tracks[0] was just updated (lifetime 0) and holds points, that track's ring made relative to its centroid
// (relative_coordinates, Utils.py:437-465) as the 3 x 64 row block of format_batched_frames (Utils.py:523-548) -- for every asked
// scene in one output, scenes ascending, with a directory entry per sample.  Reads SceneHdr, order, TrackRec and the track rings
// after the step, as k_cloud_write does; nothing of the step is touched and nothing is kept between two calls.
//   k_sample_count   a lane per scene: does the scene give a sample (0 / 1 into both count arrays)
//   k_pair_scan      (k_scan.hip) one workgroup: the offset scans, the capacity decision, the total
//   k_sample_write   a workgroup per scene, which leaves at once without a sample -- only if everything fits
//     MMW_SAMPLE_BLOCK   double[192][5]: a wave per frame, newest first, a lane per row
//     MMW_SAMPLE_INPUT   float[8][8][5]: format_single_frame_mode(np.float32(block), mean, std, 1, fuse=True) (Utils.py:551-572) of
//                        the block's newest frame: one wave, a lane per row, the bitonic network of k_features (mmw_sort.hpp)
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_math.hpp"
#include "mmw_ring.hpp"
#include "mmw_sort.hpp"
#include "mmw_dispatch.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_sample_entry) == 48 && alignof(mmw_sample_entry) == 8, "mmw_sample_entry");
static_assert(offsetof(mmw_sample_entry, rows) == 16 && offsetof(mmw_sample_entry, cut) == 28 && offsetof(mmw_sample_entry, centroid) == 32, "no padding");

constexpr int kSampleFrames = 3, kSampleRows = 64, kSampleCols = 5;   // the block of format_batched_frames: 3 x 64 rows of 5 columns
constexpr int kFrameUnits = kSampleRows * kSampleCols * 8 / 16;       // a frame of the block = 2560 bytes = 160 16-byte units
constexpr int kInputUnits = kSampleRows * kSampleCols * 4 / 16;       // the fp32 form = 1280 bytes = 80 units

// The sample of scene s, if it has one: the record of effective_tracks[0], the frames of its ring NEWEST first (rows the
// reference holds, rows to copy, physical slot), the rows beyond 64.
struct Sample {
    const TrackRec *rec;
    int rslot, frames, cut;
    int held[kSampleFrames], take[kSampleFrames], phys[kSampleFrames];
};
__device__ __forceinline__ bool sample_of(const DevCfg &cfg, const DevState &st, const int32_t *__restrict__ flags, int s, Sample &m)
{
    if (flags && flags[s] == 0) return false;            // not asked
    if (live_tracks(cfg, st, s) < 1) return false;       // effective_tracks is empty
    m.rslot = live_slot(cfg, st, s, 0);
    m.rec = st.trk + (size_t)s * cfg.t_cap + m.rslot;
    if (!(m.rec->lifetime == 0.0)) return false;          // position 0 was not updated by this frame
    const Ring r = track_ring(cfg, m.rec);
    m.frames = min(r.len, kSampleFrames);                 // (the entry points refuse a ring of more than three frames)
    m.cut = 0;
    int total = 0;
#pragma unroll
    for (int j = 0; j < kSampleFrames; j++) {
#ifdef MMW_MUTANT_SAMPLE_OLDEST_FIRST   // (diagnostic build `make DIAG=sampleorder DIAGFLAGS=-DMMW_MUTANT_SAMPLE_OLDEST_FIRST`, never the
                                        //  product: the frames oldest first -- what tests/test_gpu_samples.py's oracle comparison must catch)
        const int k = j;
#else
        const int k = r.len - 1 - j;
#endif
        int held = 0, stored = 0, phys = 0;
#pragma unroll
        for (int q = 0; q < MMW_RING_MAX; q++)
            if (q == k && q < r.len) { held = max(m.rec->ring_n[q], 0); stored = r.n[q]; phys = r.phys[q]; }
        m.held[j] = held;
        m.take[j] = min(stored, kSampleRows);
        m.phys[j] = phys;
        m.cut += max(held - kSampleRows, 0);
        total += held;
    }
    return total > 0;                                     // batch.effective_data is not empty
}

__global__ __launch_bounds__(256) void k_sample_count(DevCfg cfg, DevState st, ExportScratch sc, const int32_t *__restrict__ flags)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= cfg.n_scenes) return;
    Sample m;
    const int c = sample_of(cfg, st, flags, s, m) ? 1 : 0;
    sc.off[s] = c;
    sc.off[cfg.n_scenes + 1 + s] = c;
}

// row `lane` of frame j of the sample as the block holds it: columns [0, 1, 2, 6, 7] of the ring row, x and y made relative in
// fp64; a row the frame does not hold is a true zero row (the pad rows are not shifted)
__device__ __forceinline__ void sample_row(const DevCfg &cfg, const DevState &st, int s, int rslot, int phys, int take, int lane, double cx, double cy,
                                           double (&v)[kSampleCols])
{
#pragma unroll
    for (int c = 0; c < kSampleCols; c++) v[c] = 0.0;
    if (lane < take) {
        const double *p = st.trk_ring + ((((size_t)s * cfg.t_cap + rslot) * cfg.ring + phys) * cfg.ring_rows + lane) * 8;
        const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 6);
        v[0] = a.x - cx;   // relative_coordinates Utils.py:455-463 (the other six columns have 0 subtracted: unchanged)
        v[1] = a.y - cy;
        v[2] = p[2];
        v[3] = b.x;
        v[4] = b.y;
    }
}

__device__ __forceinline__ uint2 bits_of(double d)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return uint2{(uint32_t)u, (uint32_t)(u >> 32)};
}

// BLOCK: 192 threads, wave j = frame j of the block.  A lane's row is 40 bytes, so the rows go through LDS (7680 bytes) and leave as
//        16-byte units, 160 per wave and contiguous: absent frames and pad rows are zeros written by the same stores.
// INPUT: 64 threads.  Every value rounded once to fp32, the intensity normalised by two fp32 operations, rows that are all zero
//        after that behind the others as true zero rows, then the stable sort on x: ties by (is-all-zero, row position).  The
//        1280 bytes leave through LDS as 80 16-byte units.
// SITE:  (INPUT) the scene's own intensity scale, where k_features<true> takes it.
template <int MODE, bool SITE>
__global__ __launch_bounds__(MODE == MMW_SAMPLE_BLOCK ? 64 * kSampleFrames : 64)
void k_sample_write(DevCfg cfg, const mmw_scene_site *__restrict__ sites, DevState st, ExportScratch sc, const int32_t *__restrict__ flags,
                    mmw_sample_entry *__restrict__ dir, void *__restrict__ out, int absolute, int scene_base)
{
    __shared__ uint4 stage[MODE == MMW_SAMPLE_BLOCK ? kSampleFrames * kFrameUnits : kInputUnits];
    if (!sc.totals[2]) return;   // (uniform over the launch) the samples do not fit: neither buffer is written
    const int s = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Sample m;
    if (!sample_of(cfg, st, flags, s, m)) return;   // (uniform over the workgroup)
    const int e = sc.off[s];
    const double c0 = m.rec->centroid[0], c1 = m.rec->centroid[1];
    const double cx = absolute ? 0.0 : c0, cy = absolute ? 0.0 : c1;
    if (threadIdx.x < 6) {   // the 48-byte entry as six 8-byte pieces
        uint2 w;
        if (threadIdx.x == 0) w = uint2{(uint32_t)(scene_base + s), (uint32_t)m.rec->uid};
        else if (threadIdx.x == 1) w = uint2{(uint32_t)m.frames, 0u};
        else if (threadIdx.x == 2) w = uint2{(uint32_t)m.held[0], (uint32_t)m.held[1]};
        else if (threadIdx.x == 3) w = uint2{(uint32_t)m.held[2], (uint32_t)m.cut};
        else w = bits_of(threadIdx.x == 4 ? c0 : c1);
        reinterpret_cast<uint2 *>(dir + e)[threadIdx.x] = w;
    }
    if constexpr (MODE == MMW_SAMPLE_BLOCK) {
        double v[kSampleCols];
        const int j = wave;   // (a scalar, as the sample's fields are)
        const int take = j == 0 ? m.take[0] : (j == 1 ? m.take[1] : m.take[2]), phys = j == 0 ? m.phys[0] : (j == 1 ? m.phys[1] : m.phys[2]);
        sample_row(cfg, st, s, m.rslot, phys, take, lane, cx, cy, v);
        double *mine = reinterpret_cast<double *>(stage + j * kFrameUnits) + lane * kSampleCols;
#pragma unroll
        for (int c = 0; c < kSampleCols; c++) mine[c] = v[c];
        __syncthreads();
        uint4 *dst = reinterpret_cast<uint4 *>(out) + ((size_t)e * kSampleFrames + j) * kFrameUnits;
        const uint4 *src = stage + j * kFrameUnits;
        dst[lane] = src[lane];
        dst[64 + lane] = src[64 + lane];
        if (lane < kFrameUnits - 128) dst[128 + lane] = src[128 + lane];
    } else {
        double v[kSampleCols];
        sample_row(cfg, st, s, m.rslot, m.phys[0], m.take[0], lane, cx, cy, v);
        const double mu = SITE ? sites[s].intensity_mu : cfg.intensity_mu, sd = SITE ? sites[s].intensity_std : cfg.intensity_std;
        float x0 = (float)v[0], x1 = (float)v[1], x2 = (float)v[2], x3 = (float)v[3];
        float x4 = ((float)v[4] - (float)mu) / (float)sd;   // Utils.py:556 on the float32 block
        const bool zero = x0 == 0.f && x1 == 0.f && x2 == 0.f && x3 == 0.f && x4 == 0.f;   // Utils.py:563: such a row is dropped and padded back
        if (zero) x0 = x1 = x2 = x3 = x4 = 0.f;
        double key = (double)x0;
        int src = (zero ? 64 : 0) | lane;
        bitonic_sort64(lane, key, src);
        src &= 63;
        float *mine = reinterpret_cast<float *>(stage) + lane * kSampleCols;
        mine[0] = __shfl(x0, src);
        mine[1] = __shfl(x1, src);
        mine[2] = __shfl(x2, src);
        mine[3] = __shfl(x3, src);
        mine[4] = __shfl(x4, src);
        __syncthreads();
        uint4 *dst = reinterpret_cast<uint4 *>(out) + (size_t)e * kInputUnits;
        dst[lane] = stage[lane];
        if (lane < kInputUnits - 64) dst[64 + lane] = stage[64 + lane];
    }
}

void launch_samples(const DevCfg &cfg, const mmw_scene_site *sites, const DevState &s, const ExportScratch &sc, mmw_sample_entry *dir, int cap_samples,
                    void *out, int mode, const int32_t *scene_flags, int scene_base, hipStream_t st)
{
    const int absolute = (mode & MMW_SAMPLE_ABSOLUTE) ? 1 : 0;
    hipLaunchKernelGGL(k_sample_count, dim3((cfg.n_scenes + 255) / 256), dim3(256), 0, st, cfg, s, sc, scene_flags);
    launch_pair_scan(cfg.n_scenes, sc.off, sc.totals, cap_samples, cap_samples, st);
    if ((mode & 1) == MMW_SAMPLE_BLOCK)
        hipLaunchKernelGGL((k_sample_write<MMW_SAMPLE_BLOCK, false>), dim3(cfg.n_scenes), dim3(64 * kSampleFrames), 0, st, cfg, sites, s, sc, scene_flags, dir, out, absolute, scene_base);
    else
        with_flag(sites != nullptr, [&](auto SITE) {
            hipLaunchKernelGGL((k_sample_write<MMW_SAMPLE_INPUT, decltype(SITE)::value>), dim3(cfg.n_scenes), dim3(64), 0, st, cfg, sites, s, sc, scene_flags, dir, out, absolute, scene_base);
        });
}

}  // namespace mmw
