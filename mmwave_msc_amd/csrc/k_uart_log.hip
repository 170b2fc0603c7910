// k_uart_log.hip -- the radar log's export (mmw_uart_log_*): every scene's staged frame -- what k_uart_read<., ., LOG = true> (k_uart.hip) kept of
// the last read() that decoded one: its wire objects and its log word -- as the reference's `frameNumber, detObj`
// (DataLogging.py:30-38), compacted into one output in ascending scene order with a directory entry per frame.
//   k_ulog_count   a lane per scene: is the scene emitted, and with how many objects
//   k_pair_scan    (k_scan.hip) one workgroup: the two offset scans, the capacity decision, the totals
//   k_ulog_write   a workgroup per scene: marks the asked scene's frame exported and, if it is emitted, writes its directory entry
//                  and its rows -- only if everything fits
// The decode is the readers' own (decode_tlv_object, xyz_q_divisor: mmw_normalize.hpp, mmw_device.hpp), so a row equals what the
// same read handed to normalize_rows, and the reference's detObj, bit for bit.
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_math.hpp"
#include "mmw_normalize.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_uart_frame) == 32 && offsetof(mmw_uart_frame, t) == 16 && offsetof(mmw_uart_frame, reserved_) == 28, "mmw_uart_frame");
static_assert(sizeof(mmw_uart_object) == 48 && offsetof(mmw_uart_object, range) == 40, "mmw_uart_object");

struct __attribute__((packed, aligned(4))) Obj12 { uint32_t x, y, z; };   // one wire object: a 12-byte load that is only 4-byte aligned
constexpr int kObjUnits = 3;   // a row = 6 fp64 = three 16-byte units

// the frame staged for scene s, if this call emits it: objects it holds (clamped into the staging area), else -1
__device__ __forceinline__ int emitted_count(const DevCfg &cfg, const UartLogWord &w, int frame_select)
{
    if (!w.fresh || w.frame % (uint32_t)frame_select != 0) return -1;
    return min(max(w.count, 0), cfg.max_pts);
}

__global__ __launch_bounds__(256) void k_ulog_count(DevCfg cfg, UartLog log, ExportScratch sc, const int32_t *__restrict__ flags, int frame_select)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= cfg.n_scenes) return;
    int c = -1;
    if (!flags || flags[s] != 0) c = emitted_count(cfg, log.word[s], frame_select);
    sc.off[s] = c >= 0 ? 1 : 0;
    sc.off[cfg.n_scenes + 1 + s] = max(c, 0);
}

// A lane per 16-byte piece, three per object (x, y | z, doppler | peak_val, range): a wave instruction stores 1 KiB contiguously.
// Each lane decodes its object whole -- the three lanes of an object read the same 12 bytes -- and keeps its pair.
__global__ __launch_bounds__(256) void k_ulog_write(DevCfg cfg, UartState us, UartLog log, ExportScratch sc, const int32_t *__restrict__ flags, int frame_select,
                                                    mmw_uart_frame *__restrict__ dir, mmw_uart_object *__restrict__ rows, int scene_base)
{
    if (!sc.totals[2]) return;   // (uniform over the launch) something does not fit: nothing is written, no frame is consumed
    const int s = blockIdx.x, tid = threadIdx.x;
    if (flags && flags[s] == 0) return;   // not asked: the scene keeps its frame
    UartLogWord *lw = log.word + s;
    const UartLogWord w = *lw;
    __syncthreads();   // every wave has read `fresh` before it is cleared
    if (tid == 0) lw->fresh = 0;
    const int n = emitted_count(cfg, w, frame_select);
    if (n < 0) return;   // (uniform) nothing staged, or filtered out by frame_select
    const int e = sc.off[s], first = sc.off[cfg.n_scenes + 1 + s];
    const unsigned qf = w.head >> 16;
    if (tid == 0) dir[e] = mmw_uart_frame{scene_base + s, w.frame, first, n, w.t, (int32_t)qf, 0};
    const double q = xyz_q_divisor(qf);
    const double half_bins = us.scene[s].half_bins, doppler_res = us.scene[s].doppler_res;
    const uint8_t *src = log.obj + (size_t)s * cfg.max_pts * 12;
    uint4 *dst = reinterpret_cast<uint4 *>(rows + first);
    for (int u = tid; u < n * kObjUnits; u += 256) {
        const int j = u / kObjUnits, k = u - j * kObjUnits;
        const Obj12 o = *reinterpret_cast<const Obj12 *>(src + 12 * j);
        const unsigned short h[6] = {(unsigned short)o.x, (unsigned short)(o.x >> 16), (unsigned short)o.y, (unsigned short)(o.y >> 16),
                                     (unsigned short)o.z, (unsigned short)(o.z >> 16)};
        double v[5];
        decode_tlv_object(h, q, half_bins, doppler_res, v);
        const double range = (double)(short)h[0] * w.range_scale;   // as mmw_parse_uart_cap's range_out
        const double a = k == 0 ? v[0] : (k == 1 ? v[2] : v[4]);
        const double b = k == 0 ? v[1] : (k == 1 ? v[3] : range);
        const unsigned long long ab = (unsigned long long)__double_as_longlong(a), bb = (unsigned long long)__double_as_longlong(b);
        dst[u] = uint4{(uint32_t)ab, (uint32_t)(ab >> 32), (uint32_t)bb, (uint32_t)(bb >> 32)};
    }
}

void launch_uart_log(const DevCfg &cfg, const UartState &us, const UartLog &log, const ExportScratch &sc, mmw_uart_frame *dir, int cap_frames,
                     mmw_uart_object *rows, int cap_rows, const int32_t *scene_flags, int frame_select, int scene_base, hipStream_t st)
{
    hipLaunchKernelGGL(k_ulog_count, dim3((cfg.n_scenes + 255) / 256), dim3(256), 0, st, cfg, log, sc, scene_flags, frame_select);
    launch_pair_scan(cfg.n_scenes, sc.off, sc.totals, cap_frames, cap_rows, st);
    hipLaunchKernelGGL(k_ulog_write, dim3(cfg.n_scenes), dim3(256), 0, st, cfg, us, log, sc, scene_flags, frame_select, dir, rows, scene_base);
}

}  // namespace mmw
