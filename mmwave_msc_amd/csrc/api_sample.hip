// api_sample.hip -- the C-ABI (include/mmw.h): the training samples.  mmw_samples_async queues the kernels of k_sample.hip and the
// copy of the count, mmw_samples_wait waits for that copy.  The first call allocates the context's scratch; mmw_destroy frees it.
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_sample_entry) == 48, "mmw_sample_entry: the ctypes / numpy layouts of mmwave_msc_amd/_lib.py");

int mmw_samples_async(mmw_ctx *c, mmw_sample_entry *dir, int32_t cap_samples, void *out, int32_t mode, const int32_t *scene_flags, int32_t scene_base,
                      int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (cap_samples < 0 || (cap_samples > 0 && (!dir || !out)))
        return fail(c, MMW_E_ARG, "mmw_samples: cap_samples = %d with dir %s, out %s", cap_samples, dir ? "set" : "NULL", out ? "set" : "NULL");
    if (mode < 0 || mode > (MMW_SAMPLE_INPUT | MMW_SAMPLE_ABSOLUTE)) return fail(c, MMW_E_ARG, "mmw_samples: mode %d outside {0, 1, 2, 3}", mode);
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_samples: ticket %d outside [0, %d)", ticket, kTickets);
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)dir & 7) != 0) return fail(c, MMW_E_ARG, "mmw_samples: out must be 16-byte aligned, dir 8-byte aligned");
    if (c->dc.ring > 3)
        return fail(c, MMW_E_ARG, "mmw_samples: a ring of %d frames does not fit the 3 x 64 row block (format_batched_frames raises there)", c->dc.ring);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->sample.d_block) MMW_TRY(export_alloc(c, c->sample, 0, "mmw_samples"));
    launch_samples(c->dc, sites_or_null(c), c->st, c->sample.sc, dir, cap_samples, out, mode, scene_flags, scene_base, c->stream);
    return export_issue(c, c->sample, ticket);
}

int mmw_samples_wait(mmw_ctx *c, int32_t ticket, int32_t *n_samples)
{
    if (!c) return MMW_E_ARG;
    const int32_t *h;
    MMW_TRY(export_wait(c, c->sample, ticket, "mmw_samples_wait", "nothing", &h));
    if (n_samples) *n_samples = h[0];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_samples: %d samples do not fit the buffers: nothing was written", h[0]);
    return MMW_OK;
}

int mmw_samples(mmw_ctx *c, mmw_sample_entry *dir, int32_t cap_samples, void *out, int32_t mode, const int32_t *scene_flags, int32_t scene_base,
                int32_t *n_samples)
{
    const int rc = mmw_samples_async(c, dir, cap_samples, out, mode, scene_flags, scene_base, kTickets - 1);
    return rc ? rc : mmw_samples_wait(c, kTickets - 1, n_samples);
}
