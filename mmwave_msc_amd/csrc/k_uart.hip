// k_uart.hip -- the device-resident radar readers (mmw_uart_open / mmw_uart_read, include/mmw.h):
//   k_uart_read      ReadIWR14xx.read (ReadDataIWR1443.py:27-201) + Utils.normalize_data for every scene: one workgroup per
//                    scene keeps that scene's 2^15-byte byteBuffer in global memory, appends the bytes that arrived, cuts to
//                    the last magic word, decodes one packet into registers, drops it and normalises the rows
//                    SITE = true: the same body with each scene's own mounting (mmw_set_sites)
//                    LOG = true: the same body again, which also leaves the decoded frame as it came off the wire in the scene's
//                    radar log (mmw_uart_log_enable; exported by k_uart_log.hip).  Launched only while the log is on.
//                    Both false: the plain kernel, which looks at neither its `sites` nor its `log` argument.
//   k_uart_set_time  main.py's `t` restarted
// The buffer discipline is the reference's to the byte: its two slice assignments (66-69, 191-195) are moves of the buffer
// onto itself, and what they leave behind past byteBufferLength is read again by a later packet whose objects reach past the
// bytes received (the stale bytes).  So the moves are PHYSICAL here too, and nothing else ever writes the buffer.
#include "mmw_device.hpp"
#include "mmw_math.hpp"
#include "mmw_normalize.hpp"
#include "mmw_launch.hpp"
#include "mmw_dispatch.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

// a 16-byte load that is only 4-byte aligned (global_load_dwordx4 takes it)
struct __attribute__((packed, aligned(4))) U4A { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(4))) U3A { uint32_t x, y, z; };

// the bytes lo <= b < hi of a dword, as a mask (any lo, hi)
__device__ __forceinline__ uint32_t byte_mask(int lo, int hi)
{
    const uint32_t ml = lo <= 0 ? 0xffffffffu : (lo >= 4 ? 0u : 0xffffffffu << (8 * lo));
    const uint32_t mh = hi >= 4 ? 0xffffffffu : (hi <= 0 ? 0u : (1u << (8 * hi)) - 1u);
    return ml & mh;
}

// buf[d0 .. d0 + cnt) = src[s0 .. s0 + cnt), by the whole workgroup (every argument uniform; buf 16-byte aligned, src 4-byte
// aligned; d0 + cnt <= kUartBuf).  The destination is written in ALIGNED 16-byte pieces, a thread per piece and 4 KiB per
// pass; the byte shift between the two sides is absorbed where the piece is loaded -- five aligned dwords, v_alignbyte --,
// and the pieces at either end keep the bytes outside the range (they are loaded first and merged in).  Of src only whole
// dwords that start in [0, src_bytes) are read.
// src may be buf itself with s0 > d0 = 0 (the reference's moves to the front): a pass loads, passes a barrier, then stores.
// The sources of a later pass lie above everything an earlier pass stored (s0 > 0), so one barrier per pass is enough; the
// closing one stands between the last stores and whoever reads the buffer next.
__device__ __forceinline__ void move_bytes(uint8_t *buf, int d0, const uint8_t *src, long long s0, long long src_bytes, int cnt)
{
    if (cnt <= 0) return;
    const int tid = threadIdx.x;
    const int v_last = (d0 + cnt - 1) >> 4;
    for (int vb = d0 >> 4; vb <= v_last; vb += 256) {
        const int v = vb + tid;
        const bool active = v <= v_last;
        uint32_t w[5] = {0, 0, 0, 0, 0};
        uint4 old = {0, 0, 0, 0};
        int lo = 0, hi = 0;
        unsigned sh = 0;
        if (active) {
            const long long sa = s0 + (long long)(16 * v - d0);   // where the piece's byte 0 comes from (< 0 in front of a first piece)
            const long long a = sa & ~3LL;
            sh = (unsigned)(sa & 3);
            if (a >= 0 && a <= src_bytes - 20) {
                const U4A q = *reinterpret_cast<const U4A *>(src + a);
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
                w[4] = *reinterpret_cast<const uint32_t *>(src + a + 16);
            } else {
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    const long long o = a + 4 * k;
                    if (o >= 0 && o < src_bytes) w[k] = *reinterpret_cast<const uint32_t *>(src + o);
                }
            }
            lo = max(d0 - 16 * v, 0);
            hi = min(d0 + cnt - 16 * v, 16);
            if (lo > 0 || hi < 16) old = *reinterpret_cast<const uint4 *>(buf + 16 * v);
        }
        __syncthreads();
        if (active) {
            const uint32_t o[4] = {old.x, old.y, old.z, old.w};
            uint32_t r[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t nw = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
                const uint32_t m = byte_mask(lo - 4 * i, hi - 4 * i);
                r[i] = (nw & m) | (o[i] & ~m);
            }
            *reinterpret_cast<uint4 *>(buf + 16 * v) = uint4{r[0], r[1], r[2], r[3]};
        }
    }
    __syncthreads();
}

// The last position loc < limit at which the magic word 02 01 04 03 06 05 08 07 starts in buf, -1 if none (uniform; limit =
// byteBufferLength - 8 > 8).  Backwards, 4096 positions per pass: a lane takes 16 positions -- an aligned 16-byte piece and
// the 8 bytes behind it -- and thread 0 the highest, so the first lane of the first wave with a hit holds the answer.
__device__ __forceinline__ int find_last_magic(const uint8_t *buf, int limit, int *red /* LDS [4] */)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int vt = (limit - 1) >> 4; vt >= 0; vt -= 256) {
        const int v = vt - tid;
        int best = -1;
        if (v >= 0) {
            const int p0 = 16 * v;
            const uint4 a = *reinterpret_cast<const uint4 *>(buf + p0);
            uint2 b = {0, 0};
            if (p0 + 16 < kUartBuf) b = *reinterpret_cast<const uint2 *>(buf + p0 + 16);
            const uint32_t w[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t l = __builtin_amdgcn_alignbyte(w[j / 4 + 1], w[j / 4], (unsigned)(j & 3));
                const uint32_t h = __builtin_amdgcn_alignbyte(w[j / 4 + 2], w[j / 4 + 1], (unsigned)(j & 3));
                if (l == 0x03040102u && h == 0x07080506u) m |= 1u << j;
            }
            const int room = limit - p0;   // (> 0) positions of this piece that count
            if (room < 16) m &= (1u << room) - 1u;
            if (m) best = p0 + 31 - __clz(m);
        }
        const unsigned long long bal = __ballot(best >= 0);
        int wbest = -1;
        if (bal) wbest = __shfl(best, __ffsll((long long)bal) - 1);
        if (lane == 0) red[wave] = wbest;
        __syncthreads();
        int r = -1;
#pragma unroll
        for (int k = 0; k < 4; k++) { const int c = red[k]; if (r < 0) r = c; }
        __syncthreads();   // (red is written again by the next pass)
        if (r >= 0) return r;
    }
    return -1;
}

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }

// One read() of scene blockIdx.x, then normalize_data on what it decoded.  R = rows per thread, as in k_normalize_tlv.
// LOG: a read that gives MMW_UART_POINTS also stores its wire objects and the scene's log word (UartLog, mmw_device.hpp).
template <int R, bool LOG>
__device__ __forceinline__ void uart_read_scene(const DevCfg &cfg, const UartState &us, const uint8_t *__restrict__ chunks,
                                                const long long *__restrict__ chunk_off, long long chunks_bytes, const int32_t *__restrict__ flags,
                                                double now, double *__restrict__ out, int32_t *__restrict__ n_out, double *__restrict__ dt_out,
                                                int32_t *__restrict__ status, uint32_t *__restrict__ frame_number, int *wcnt /* LDS [R * 4] */,
                                                int *red /* LDS [4] */, const UartLog &log)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    UartScene *sc = us.scene + s;
    uint8_t *buf = us.buf + (size_t)s * kUartBuf;
    int refused = -1;
    long long off0 = 0, cnt = 0;
    if (flags && flags[s] == 0) refused = MMW_UART_SKIPPED;
    else {
        off0 = chunk_off[s];
        const long long off1 = chunk_off[s + 1];
        if (off0 < 0 || off1 < off0 || off1 > chunks_bytes) refused = MMW_UART_BADCHUNK;   // (no sum of an offset: nothing overflows)
        else cnt = off1 - off0;
    }
    if (refused >= 0) {   // uniform: no read() happens
        if (tid == 0) { n_out[s] = 0; dt_out[s] = 0.0; status[s] = refused; frame_number[s] = 0; }
        return;
    }
    int len = sc->len;
    const double half_bins = sc->half_bins, doppler_res = sc->doppler_res;
    // 1. "check that the buffer is not full, and then add the data to the buffer" (42-46)
    int dropped = 0;
    if ((long long)len + cnt < kUartBuf) {
        move_bytes(buf, len, chunks, off0, chunks_bytes, (int)cnt);
        len += (int)cnt;
    } else dropped = MMW_UART_CHUNK_DROPPED;
    // 2.-4. the last magic word, the cut to it, and whether the packet is all there (49-80)
    bool complete = false;
    uint32_t total = 0;
    if (len > 16) {
        const int loc = find_last_magic(buf, len - 8, red);
        if (loc >= 0) {
            if (loc > 0) {
                move_bytes(buf, 0, buf, loc, kUartBuf, len - loc);
                len -= loc;
            }
            if (len > 16) {
                total = ld32(buf + 12);               // totalPacketLen: any value, 0 included
                complete = (uint32_t)len >= total;
            }
        }
    }
    // 5. header, TLV head, objects (85-150): idx is the reference's idX when it reaches "remove already processed data"
    int st = MMW_UART_NONE, idx = 36, n = 0;
    uint32_t frame = 0, head_word = 0;
    double q = 1.0;
    if (complete) {
        st = MMW_UART_PACKET;
        frame = ld32(buf + 20);
        if (ld32(buf + 28) != 0) {                    // numDetectedObj > 0
            idx = 44;
            if (ld32(buf + 36) == 1) {                // MMWDEMO_UART_MSG_DETECTED_POINTS
                const uint32_t head = ld32(buf + 44);
                const int num = (int)(head & 0xffffu);
                if (num > (kUartBuf - 48) / 12) {     // an object past the end of the buffer: np.matmul of a short slice raises
                    st = MMW_UART_RAISED;
                    frame = 0;
                } else {
                    idx = 48 + 12 * num;
                    if (num > cfg.max_pts) st = MMW_UART_OVERFLOW;
                    else { st = MMW_UART_POINTS; n = num; q = xyz_q_divisor(head >> 16); head_word = head; }
                }
            }
        }
    }
    double v[R][5];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int i = r * 256 + tid;
        unsigned short w[6] = {0, 0, 0, 0, 0, 0};
        if (i < n) {   // (48 + 12 i + 12 <= kUartBuf: num was checked) -- bytes past len are the buffer's stale bytes
            const U3A o = *reinterpret_cast<const U3A *>(buf + 48 + 12 * i);
            if constexpr (LOG) *reinterpret_cast<U3A *>(log.obj + ((size_t)s * cfg.max_pts + i) * 12) = o;   // (n <= max_pts; contiguous across lanes)
            w[0] = (unsigned short)o.x; w[1] = (unsigned short)(o.x >> 16);
            w[2] = (unsigned short)o.y; w[3] = (unsigned short)(o.y >> 16);
            w[4] = (unsigned short)o.z; w[5] = (unsigned short)(o.z >> 16);
        }
        decode_tlv_object(w, q, half_bins, doppler_res, v[r]);
    }
    // 6. "remove already processed data" (188-195): totalPacketLen bytes, whatever it says (<= len; 0 moves nothing).  The
    // objects are in registers: the first barrier of the move stands between their loads and its stores.
    if (complete && st != MMW_UART_RAISED && len > idx) {
        if (total > 0) move_bytes(buf, 0, buf, (long long)total, kUartBuf, len - (int)total);
        len -= (int)total;
    }
    // 7. normalize_data, and the words of this read
    normalize_rows<R>(cfg, s, n, v, out, n_out, wcnt);
    if (tid == 0) {
        if (st == MMW_UART_OVERFLOW) n_out[s] = MMW_BAD_FRAME;   // (the same thread wrote the 0)
        double dt = 0.0;
        if (st == MMW_UART_POINTS) {                 // main.py:44-47
            dt = now - sc->t_last;
            sc->t_last = now;
        }
        dt_out[s] = dt;
        status[s] = st | dropped;
        frame_number[s] = frame;
        sc->len = len;
        if constexpr (LOG) {
            if (st == MMW_UART_POINTS) {             // (every other status leaves the log alone: OVERFLOW and RAISED log nothing)
                UartLogWord *lw = log.word + s;
                lw->t = now;
                *reinterpret_cast<uint4 *>(&lw->frame) = uint4{frame, (uint32_t)n, head_word, 1u};   // frame, count, head, fresh
            }
        }
    }
}

template <int R, bool SITE, bool LOG>
__global__ __launch_bounds__(256) void k_uart_read(DevCfg cfg, const mmw_scene_site *__restrict__ sites, UartState us, UartLog log,
                                                   const uint8_t *__restrict__ chunks, const long long *__restrict__ chunk_off, long long chunks_bytes,
                                                   const int32_t *__restrict__ flags, double now, double *__restrict__ out, int32_t *__restrict__ n_out,
                                                   double *__restrict__ dt_out, int32_t *__restrict__ status, uint32_t *__restrict__ frame_number)
{
    __shared__ int wcnt[R * 4];
    __shared__ int red[4];
    if constexpr (SITE)
        uart_read_scene<R, LOG>(cfg_with_mounting(cfg, sites + blockIdx.x), us, chunks, chunk_off, chunks_bytes, flags, now, out, n_out, dt_out, status,
                                frame_number, wcnt, red, log);
    else
        uart_read_scene<R, LOG>(cfg, us, chunks, chunk_off, chunks_bytes, flags, now, out, n_out, dt_out, status, frame_number, wcnt, red, log);
}

__global__ __launch_bounds__(256) void k_uart_set_time(UartState us, const int32_t *__restrict__ flags, double t, int n_scenes)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_scenes && (!flags || flags[s] != 0)) us.scene[s].t_last = t;
}

void launch_uart_read(const DevCfg &cfg, const mmw_scene_site *sites, const UartState &us, const UartLog *log, const uint8_t *chunks, const long long *chunk_off,
                      long long chunks_bytes, const int32_t *flags, double now, double *out, int32_t *n_out, double *dt_out, int32_t *status,
                      uint32_t *frame_number, hipStream_t st)
{
    const UartLog lg = log ? *log : UartLog{};   // (LOG = true only while the radar log is enabled)
    with_rows(rows_per_thread(cfg.max_pts), [&](auto R) { with_flag(sites != nullptr, [&](auto SITE) { with_flag(log != nullptr, [&](auto LOG) {
        mmw_launch(k_uart_read<decltype(R)::value, decltype(SITE)::value, decltype(LOG)::value>, dim3(cfg.n_scenes), dim3(256), 0, st, cfg, sites, us, lg,
                   chunks, chunk_off, chunks_bytes, flags, now, out, n_out, dt_out, status, frame_number);
    }); }); });
}
void launch_uart_set_time(const DevCfg &cfg, const UartState &us, const int32_t *flags, double t, hipStream_t st)
{
    hipLaunchKernelGGL(k_uart_set_time, dim3((cfg.n_scenes + 255) / 256), dim3(256), 0, st, us, flags, t, (int)cfg.n_scenes);
}

}  // namespace mmw
