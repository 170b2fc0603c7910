// api_uart.hip -- the C-ABI (include/mmw.h): the radar's UART packets -- decoded on the host (mmw_parse_uart*, mmw_find_tlv: no
// context, no HIP call), and the device-resident readers (mmw_uart_*: their state, and the launch of k_uart.hip; the radar log
// they feed is api_uart_log.hip's).
#include <cstring>

#include "mmw_ctx.hpp"

// The packet part of ReadIWR14xx.read (ReadDataIWR1443.py:47-113), shared by mmw_parse_uart and mmw_find_tlv: the LAST magic word
// that starts in buf[0 .. len-8), more than 16 bytes from there and at least totalPacketLen of them -- whatever totalPacketLen
// says, 0 and 20 included: the reference then reads the header, the TLV head and the objects all the same.  Every word it reads
// must lie in buf[0 .. cap): past `len` it is whatever the caller's buffer holds there (the reference's stale bytes), past `cap`
// the reference's np.matmul of a short slice raises ValueError (-1 here).  Otherwise MMW_UART_NONE (no complete packet),
// MMW_UART_PACKET (complete: no objects announced, or another TLV first) or MMW_UART_POINTS with *body = offset from buf of the
// TLV body (u16 numObj, u16 Q, objects).
static int find_tlv_body(const uint8_t *buf, size_t len, size_t cap, size_t *body, uint32_t *num_obj, uint32_t *qfmt, uint32_t *frame_number,
                         size_t *packet_start, size_t *packet_len)
{
    static const uint8_t magic[8] = {2, 1, 4, 3, 6, 5, 8, 7};
    if (frame_number) *frame_number = 0;
    if (packet_start) *packet_start = 0;
    if (packet_len) *packet_len = 0;
    if (len <= 16) return MMW_UART_NONE;
    size_t start = len;  // the last magic word that starts in buf[0 .. len-8)
    for (size_t loc = len - 8; loc-- > 0;)
        if (memcmp(buf + loc, magic, 8) == 0) { start = loc; break; }
    if (start == len) return MMW_UART_NONE;
    if (packet_start) *packet_start = start;
    const size_t rem = len - start;
    if (rem <= 16) return MMW_UART_NONE;
    const uint8_t *p = buf + start;  // offsets below are relative to the packet
    const size_t room = cap - start; // bytes of the packet that may be read (> rem > 16)
    auto u32 = [&](size_t o) { return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24); };
    auto u16 = [&](size_t o) { return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8); };
    const size_t total = u32(12);
    if (rem < total) return MMW_UART_NONE;
    if (room < 36) return -1;  // the header words (85-92)
    if (packet_len) *packet_len = total;
    if (frame_number) *frame_number = u32(20);
    if (u32(28) == 0) return MMW_UART_PACKET;  // no objects announced (101)
    if (room < 44) return -1;                  // TLV type, length (103-106)
    if (u32(36) != 1) return MMW_UART_PACKET;  // another TLV first (109)
    if (room < 48) return -1;                  // numObj, xyzQFormat (116-121)
    const uint32_t num = u16(44), q = u16(46);
    if ((room - 48) / 12 < num) return -1;     // the objects (131-150)
    *body = start + 44;
    *num_obj = num;
    *qfmt = q;
    return MMW_UART_POINTS;
}

int mmw_parse_uart_cap(const uint8_t *buf, size_t len, size_t cap, const mmw_uart_cfg *cfg, double *raw, double *range_out, int32_t max_obj,
                       int32_t *n_obj, uint32_t *frame_number, size_t *packet_start, size_t *packet_len)
{
    if (!buf || !cfg || !raw || !n_obj || max_obj < 0 || cap < len) return MMW_E_ARG;
    *n_obj = 0;
    size_t body = 0;
    uint32_t num = 0, qfmt = 0;
    const int rc = find_tlv_body(buf, len, cap, &body, &num, &qfmt, frame_number, packet_start, packet_len);
    if (rc < 0) return MMW_E_CAPACITY;
    if (rc != MMW_UART_POINTS) return rc;
    if ((int64_t)num > (int64_t)max_obj) return MMW_E_ARG;
    auto u16 = [&](size_t o) { return (uint32_t)buf[o] | ((uint32_t)buf[o + 1] << 8); };
    size_t idx = body + 4;
    const double q = mmw::xyz_q_divisor(qfmt);
    const double half = cfg->num_doppler_bins / 2.0 - 1;
    for (uint32_t o = 0; o < num; o++, idx += 12) {
        const int16_t range_idx = (int16_t)u16(idx), peak = (int16_t)u16(idx + 4);
        int16_t dop = (int16_t)u16(idx + 2);
        const int16_t x = (int16_t)u16(idx + 6), y = (int16_t)u16(idx + 8), z = (int16_t)u16(idx + 10);
        if ((double)dop > half) dop = (int16_t)((int32_t)dop - 65535);  // ReadDataIWR1443.py:150-157 (wraps in int16)
        raw[o * 5 + 0] = (double)x / q;
        raw[o * 5 + 1] = (double)y / q;
        raw[o * 5 + 2] = (double)z / q;
        raw[o * 5 + 3] = (double)dop * cfg->doppler_resolution_mps;
        raw[o * 5 + 4] = (double)peak;
        if (range_out) range_out[o] = (double)range_idx * cfg->range_idx_to_meters;
    }
    *n_obj = (int32_t)num;
    return MMW_UART_POINTS;
}

// The first form of the host decode, kept for its callers: nothing past len is read (cap = len), 1 = points parsed, 0 = none of
// them -- no complete packet, a complete one without points, or one whose words reach past len --, MMW_E_ARG as above.
int mmw_parse_uart(const uint8_t *buf, size_t len, const mmw_uart_cfg *cfg, double *raw, double *range_out, int32_t max_obj,
                   int32_t *n_obj, uint32_t *frame_number, size_t *packet_start, size_t *packet_len)
{
    const int rc = mmw_parse_uart_cap(buf, len, len, cfg, raw, range_out, max_obj, n_obj, frame_number, packet_start, packet_len);
    if (rc == MMW_E_ARG) return MMW_E_ARG;
    return rc == MMW_UART_POINTS ? 1 : 0;
}

int mmw_find_tlv(const uint8_t *buf, size_t len, int64_t *body_offset, int32_t *n_obj, uint32_t *frame_number, size_t *packet_start, size_t *packet_len)
{
    if (!buf || !body_offset || !n_obj) return MMW_E_ARG;
    *body_offset = -1;
    *n_obj = 0;
    size_t body = 0;
    uint32_t num = 0, qfmt = 0;
    // (no buffer history: cap = len -- a packet whose words reach past len is refused)
    if (find_tlv_body(buf, len, len, &body, &num, &qfmt, frame_number, packet_start, packet_len) != MMW_UART_POINTS) return 0;
    *body_offset = (int64_t)body;
    *n_obj = (int32_t)num;
    return 1;
}

// ---- the device-resident readers ----
static_assert((MMW_UART_BUFFER - 48) / 12 == 2726, "the rule behind MMW_E_CAPACITY above, with the packet at the head of the buffer (k_uart.hip)");

int mmw_uart_close(mmw_ctx *c)
{
    if (!c) return MMW_E_ARG;
    if (!c->uart.buf) return MMW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (a read may still be queued on what is freed here)
    uart_log_free(c);
    HIPCHK(c, hipFree(c->uart.buf));
    c->uart = UartState{};
    c->uart_range.clear();
    return MMW_OK;
}

int mmw_uart_open(mmw_ctx *c, const mmw_uart_cfg *cfg, int32_t n_cfg, double t0)
{
    if (!c || !cfg) return fail(c, MMW_E_ARG, "mmw_uart_open: null argument");
    const size_t S = c->dc.n_scenes;
    if (n_cfg != 1 && (size_t)n_cfg != S) return fail(c, MMW_E_ARG, "mmw_uart_open: n_cfg=%d must be 1 or n_scenes=%zu", n_cfg, S);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->uart.buf) {
        uint8_t *p = nullptr;
        HIPCHK(c, hipMalloc((void **)&p, S * (MMW_UART_BUFFER + sizeof(UartScene))));
        c->uart.buf = p;
        c->uart.scene = reinterpret_cast<UartScene *>(p + S * MMW_UART_BUFFER);
    }
    std::vector<UartScene> h(S);
    c->uart_range.resize(S);
    for (size_t s = 0; s < S; s++) {
        const mmw_uart_cfg &u = cfg[n_cfg == 1 ? 0 : s];
        h[s] = UartScene{t0, u.num_doppler_bins / 2.0 - 1, u.doppler_resolution_mps, 0, 0};
        c->uart_range[s] = u.range_idx_to_meters;
    }
    HIPCHK(c, hipMemsetAsync(c->uart.buf, 0, S * MMW_UART_BUFFER, c->stream));   // np.zeros(2**15) (ReadDataIWR1443.py:15)
    HIPCHK(c, hipMemcpyAsync(c->uart.scene, h.data(), S * sizeof(UartScene), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (h goes out of scope)
    return uart_log_rearm(c);   // (a log that is on starts again: no staged frame survives the new readers)
}

int mmw_uart_read(mmw_ctx *c, const uint8_t *chunks, const int64_t *chunk_off, size_t chunks_bytes, const int32_t *scene_flags, double now,
                  double *pts, int32_t *n_out, double *dt_out, int32_t *status, uint32_t *frame_number)
{
    if (!c || !chunks || !chunk_off || !pts || !n_out || !dt_out || !status || !frame_number) return fail(c, MMW_E_ARG, "mmw_uart_read: null pointer");
    if (!c->uart.buf) return fail(c, MMW_E_ARG, "mmw_uart_read: the readers are not open (mmw_uart_open)");
    if (((uintptr_t)pts & 15) != 0 || ((uintptr_t)chunks & 3) != 0) return fail(c, MMW_E_ARG, "mmw_uart_read: pts must be 16-byte aligned, chunks 4-byte aligned");
    if (chunks_bytes > (size_t)INT64_MAX) return fail(c, MMW_E_ARG, "mmw_uart_read: chunks_bytes out of range");
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(long long) == sizeof(int64_t), "chunk offsets");
    launch_uart_read(c->dc, sites_or_null(c), c->uart, c->ulog.word ? &c->ulog : nullptr, chunks, reinterpret_cast<const long long *>(chunk_off), (long long)chunks_bytes, scene_flags, now, pts,
                     n_out, dt_out, status, frame_number, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_uart_get_state(mmw_ctx *c, int32_t scene, uint8_t *buf, int32_t *len, double *t_last)
{
    if (!c || !buf || !len || !t_last) return fail(c, MMW_E_ARG, "mmw_uart_get_state: null argument");
    if (!c->uart.buf) return fail(c, MMW_E_ARG, "mmw_uart_get_state: the readers are not open (mmw_uart_open)");
    if (scene < 0 || scene >= c->dc.n_scenes) return fail(c, MMW_E_ARG, "mmw_uart_get_state: scene %d out of range", scene);
    HIPCHK(c, hipSetDevice(c->device));
    UartScene h;
    MMW_TRY(d2h_after_kernels(c, buf, c->uart.buf + (size_t)scene * MMW_UART_BUFFER, MMW_UART_BUFFER));
    MMW_TRY(d2h_after_kernels(c, &h, c->uart.scene + scene, sizeof(h)));
    *len = h.len;
    *t_last = h.t_last;
    return MMW_OK;
}

int mmw_uart_set_state(mmw_ctx *c, int32_t scene, const uint8_t *buf, int32_t len, double t_last)
{
    if (!c || !buf) return fail(c, MMW_E_ARG, "mmw_uart_set_state: null argument");
    if (!c->uart.buf) return fail(c, MMW_E_ARG, "mmw_uart_set_state: the readers are not open (mmw_uart_open)");
    if (scene < 0 || scene >= c->dc.n_scenes) return fail(c, MMW_E_ARG, "mmw_uart_set_state: scene %d out of range", scene);
    if (len < 0 || len >= MMW_UART_BUFFER) return fail(c, MMW_E_ARG, "mmw_uart_set_state: len=%d must be in [0, %d)", len, MMW_UART_BUFFER);
    HIPCHK(c, hipSetDevice(c->device));
    UartScene h;
    MMW_TRY(d2h_after_kernels(c, &h, c->uart.scene + scene, sizeof(h)));   // (the scene keeps its scales)
    h.t_last = t_last;
    h.len = len;
    HIPCHK(c, hipMemcpyAsync(c->uart.buf + (size_t)scene * MMW_UART_BUFFER, buf, MMW_UART_BUFFER, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->uart.scene + scene, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}

int mmw_uart_set_time(mmw_ctx *c, const int32_t *scene_flags, double t)
{
    if (!c) return MMW_E_ARG;
    if (!c->uart.buf) return fail(c, MMW_E_ARG, "mmw_uart_set_time: the readers are not open (mmw_uart_open)");
    HIPCHK(c, hipSetDevice(c->device));
    // (the flags travel through the context's [S + 1]-word scratch, as those of mmw_reset_scenes do)
    if (scene_flags) HIPCHK(c, hipMemcpyAsync(c->d_row_off, scene_flags, sizeof(int32_t) * c->dc.n_scenes, hipMemcpyHostToDevice, c->stream));
    launch_uart_set_time(c->dc, c->uart, scene_flags ? c->d_row_off : nullptr, t, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MMW_OK;
}
