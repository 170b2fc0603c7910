// api_uart_log.hip -- the C-ABI (include/mmw.h): the radar log.  mmw_uart_log_enable owns the staged frames that the logging twins of
// the readers fill (k_uart.hip), mmw_uart_log_async queues the kernels of k_uart_log.hip and the copy of the two counts,
// mmw_uart_log_wait waits for that copy.
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_uart_frame) == 32, "mmw_uart_frame: the numpy layout of mmwave_msc_amd/_lib.py");
static_assert(sizeof(mmw_uart_object) == 48, "mmw_uart_object: the numpy layout of mmwave_msc_amd/_lib.py");

void uart_log_free(mmw_ctx *c)
{
    export_free(c->ulog_x);
    c->ulog = UartLog{};
}

// every scene's log word as new -- nothing staged, the scene's rangeIdxToMeters in place -- at enable and at mmw_uart_open
int uart_log_rearm(mmw_ctx *c)
{
    if (!c->ulog.word) return MMW_OK;
    const size_t S = c->dc.n_scenes;
    std::vector<UartLogWord> h(S);
    for (size_t s = 0; s < S; s++) h[s] = UartLogWord{0.0, c->uart_range[s], 0u, 0, 0u, 0};
    HIPCHK(c, hipMemcpyAsync(c->ulog.word, h.data(), S * sizeof(UartLogWord), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (h goes out of scope)
    for (int k = 0; k < kTickets; k++) c->ulog_x.issued[k] = false;
    return MMW_OK;
}

int mmw_uart_log_enable(mmw_ctx *c, int32_t on)
{
    if (!c) return MMW_E_ARG;
    if (!c->uart.buf) return fail(c, MMW_E_ARG, "mmw_uart_log_enable: the readers are not open (mmw_uart_open)");
    HIPCHK(c, hipSetDevice(c->device));
    if (!on) {
        if (!c->ulog_x.d_block) return MMW_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (a read or an export may still be queued on what is freed here)
        uart_log_free(c);
        return MMW_OK;
    }
    if (c->ulog_x.d_block) return MMW_OK;   // already on: the staged frames stay
    // the staged frames lie in front of the scratch, in the same device block: [S] log words | [S][max_pts] 12-byte objects
    const size_t S = c->dc.n_scenes, word_i32 = sizeof(UartLogWord) / sizeof(int32_t);
    MMW_TRY(export_alloc(c, c->ulog_x, S * word_i32 + S * (size_t)c->dc.max_pts * 3, "mmw_uart_log_enable"));
    c->ulog.word = reinterpret_cast<UartLogWord *>(c->ulog_x.d_block);
    c->ulog.obj = reinterpret_cast<uint8_t *>(c->ulog.word + S);
    const int rc = uart_log_rearm(c);
    if (rc) uart_log_free(c);
    return rc;
}

int mmw_uart_log_async(mmw_ctx *c, mmw_uart_frame *dir, int32_t cap_frames, mmw_uart_object *rows, int32_t cap_rows, const int32_t *scene_flags,
                       int32_t frame_select, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (!c->ulog_x.d_block) return fail(c, MMW_E_ARG, "mmw_uart_log: the radar log is not enabled (mmw_uart_log_enable)");
    if (cap_frames < 0 || cap_rows < 0 || (cap_frames > 0 && !dir) || (cap_rows > 0 && !rows))
        return fail(c, MMW_E_ARG, "mmw_uart_log: cap_frames = %d, cap_rows = %d with dir %s, rows %s", cap_frames, cap_rows, dir ? "set" : "NULL", rows ? "set" : "NULL");
    if (frame_select < 1) return fail(c, MMW_E_ARG, "mmw_uart_log: frame_select = %d must be at least 1", frame_select);
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_uart_log: ticket %d outside [0, %d)", ticket, kTickets);
    if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)dir & 7) != 0) return fail(c, MMW_E_ARG, "mmw_uart_log: rows must be 16-byte aligned, dir 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    launch_uart_log(c->dc, c->uart, c->ulog, c->ulog_x.sc, dir, cap_frames, rows, cap_rows, scene_flags, frame_select, scene_base, c->stream);
    return export_issue(c, c->ulog_x, ticket);
}

int mmw_uart_log_wait(mmw_ctx *c, int32_t ticket, int32_t *n_frames, int32_t *n_rows)
{
    if (!c) return MMW_E_ARG;
    if (!c->ulog_x.d_block) return fail(c, MMW_E_ARG, "mmw_uart_log_wait: the radar log is not enabled (mmw_uart_log_enable)");
    const int32_t *h;
    MMW_TRY(export_wait(c, c->ulog_x, ticket, "mmw_uart_log_wait", "no export", &h));
    if (n_frames) *n_frames = h[0];
    if (n_rows) *n_rows = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_uart_log: %d frames and %d objects do not fit the buffers: nothing was written, no frame was consumed", h[0], h[1]);
    return MMW_OK;
}

int mmw_uart_log(mmw_ctx *c, mmw_uart_frame *dir, int32_t cap_frames, mmw_uart_object *rows, int32_t cap_rows, const int32_t *scene_flags,
                 int32_t frame_select, int32_t scene_base, int32_t *n_frames, int32_t *n_rows)
{
    const int rc = mmw_uart_log_async(c, dir, cap_frames, rows, cap_rows, scene_flags, frame_select, scene_base, kTickets - 1);
    return rc ? rc : mmw_uart_log_wait(c, kTickets - 1, n_frames, n_rows);
}
