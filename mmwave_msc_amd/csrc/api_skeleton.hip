// api_skeleton.hip -- the C-ABI (include/mmw.h): the live tracks' room-frame skeletons.  mmw_skeletons_async queues the kernels of
// k_skeleton.hip and the copy of the two counts, mmw_skeletons_wait waits for that copy.  The first call allocates the context's
// scratch; mmw_destroy frees it.  mmw_skeleton_tables is host data only.
#include "mmw_ctx.hpp"

static_assert(sizeof(mmw_skeleton) == 256, "mmw_skeleton: the numpy layout of mmwave_msc_amd/_lib.py");

int mmw_skeletons_async(mmw_ctx *c, mmw_skeleton *out, int32_t cap, int32_t mode, int32_t scene_base, int32_t ticket)
{
    if (!c) return MMW_E_ARG;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, MMW_E_ARG, "mmw_skeletons: cap = %d with out %s", cap, out ? "set" : "NULL");
    if (mode != MMW_SKEL_ALL && mode != MMW_SKEL_DRAWN) return fail(c, MMW_E_ARG, "mmw_skeletons: mode %d outside {0, 1}", mode);
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_skeletons: ticket %d outside [0, %d)", ticket, kTickets);
    if (((uintptr_t)out & 15) != 0) return fail(c, MMW_E_ARG, "mmw_skeletons: out must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->skel.d_block) MMW_TRY(export_alloc(c, c->skel, 0, "mmw_skeletons"));
    launch_skeletons(c->dc, c->st, c->skel.sc, out, cap, mode, scene_base, c->stream);
    return export_issue(c, c->skel, ticket);
}

int mmw_skeletons_wait(mmw_ctx *c, int32_t ticket, int32_t *n_out, int32_t *n_live)
{
    if (!c) return MMW_E_ARG;
    const int32_t *h;
    MMW_TRY(export_wait(c, c->skel, ticket, "mmw_skeletons_wait", "nothing", &h));
    if (n_out) *n_out = h[0];
    if (n_live) *n_live = h[1];
    if (!h[2]) return fail(c, MMW_E_CAPACITY, "mmw_skeletons: %d entries (%d live tracks) do not fit the buffer: nothing was written", h[0], h[1]);
    return MMW_OK;
}

int mmw_skeletons(mmw_ctx *c, mmw_skeleton *out, int32_t cap, int32_t mode, int32_t scene_base, int32_t *n_out, int32_t *n_live)
{
    const int rc = mmw_skeletons_async(c, out, cap, mode, scene_base, kTickets - 1);
    return rc ? rc : mmw_skeletons_wait(c, kTickets - 1, n_out, n_live);
}

// Visualizer.py:100-119: the bones, in the order the reference draws them (joints: 0 SpineBase, 1 SpineMid, 2 Neck, 3 Head,
// 4-6 left shoulder / elbow / wrist, 7-9 right, 10-13 left hip / knee / ankle / foot, 14-17 right, 18 SpineShoulder)
static const int32_t kSkelConnections[18][2] = {{0, 1}, {1, 18}, {2, 3}, {18, 4}, {18, 7}, {4, 5}, {5, 6}, {7, 8}, {8, 9},
                                                {0, 14}, {14, 15}, {15, 16}, {16, 17}, {0, 10}, {10, 11}, {11, 12}, {12, 13}, {2, 18}};
// Visualizer.py:122-142: 0 blue (trunk, shoulders, hips), 1 green (limbs), 2 red (the head: square marker, twice the size)
static const int32_t kSkelJointClass[19] = {0, 0, 0, 2, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0};

int mmw_skeleton_tables(const int32_t **connections, const int32_t **joint_class)
{
    if (connections) *connections = &kSkelConnections[0][0];
    if (joint_class) *joint_class = kSkelJointClass;
    return MMW_OK;
}
