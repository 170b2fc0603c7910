// api_uart.hip -- the C-ABI (include/mmw.h): the radar's UART packets, decoded on the host (no context, no HIP call).
#include <cstring>

#include "mmw_device.hpp"

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
