// api_posture.hip -- the C-ABI (include/mmw.h): posture.  Feature tensors and keypoints of the tracks, the one-scene fp32 chain's
// model (mmw_attach_posture / _frames; mmw_frame_posture_host runs it), the batched chain (mmw_posture_attach / _frames / _models,
// the scene -> model map, mmw_estimate_posture) and the stateless mmw_mars_* entries over the CNN kernels.  Both chains serve the 3-frame model
// (define_CNN_3D) and the single-frame one (define_CNN): CnnDims has what differs between them.
#include <new>

#include "mmw_ctx.hpp"

static long long pb_act_ld(const CnnDims &d) { return 2LL * d.flat + 256; }   // the batched chain's activation row stride: mars.MarsCNN.ROW_PAD
constexpr int kPbWordRange = 0, kPbWordList = 2;
constexpr size_t pb_list_words = 2 + MMW_RANGE_FIXUP_CAP;   // one model's fix-up list
static void posture_refresh_grouped(PostureBatch *b)
{
    b->grouped = b->n_models > 1;
    for (int32_t m : b->h_map) b->grouped |= m == MMW_POSTURE_NONE;
}

void posture_batch_free(PostureBatch *b)
{
    if (!b) return;
    void *ptrs[] = {b->feat, b->hidden, b->kp, b->owner, b->uid, b->words, b->act16, b->fix_scratch, b->d_map, b->d_groups};
    for (void *p : ptrs) if (p) hipFree(p);
    for (void *p : b->w16) if (p) hipFree(p);
    if (b->h_total) hipHostFree(b->h_total);
    if (b->total_ev) hipEventDestroy(b->total_ev);
    delete b;
}

// what both chains ask of a model: every weight present, Dense-1 16-byte aligned with a leading dimension >= the model's flat
// size that is a multiple of 4; the batched chain's Dense-2 kernel reads its weights 16 bytes at a time as well
static bool posture_model_ok(const mmw_posture_model *m, const CnnDims &d, bool dense2_aligned)
{
    return m->conv1_w && m->conv1_b && m->conv2_w && m->conv2_b && m->dense1_w && m->dense1_b && m->dense2_w && m->dense2_b &&
           m->dense1_ld >= d.flat && (m->dense1_ld & 3) == 0 && ((uintptr_t)m->dense1_w & 15) == 0 &&
           (!dense2_aligned || ((uintptr_t)m->dense2_w & 15) == 0);
}

// the keypoint generation words as ticket k's k_features recorded them (mmw_ctx::d_kp_gen: [S] now | [kTickets][S])
static int32_t *kp_gen_snap(mmw_ctx *c, int ticket) { return c->d_kp_gen + (size_t)(1 + ticket) * c->dc.n_scenes; }

// The eligible tracks' feature tensors (scan, then k_features) and, behind the kernels, their total into pinned host memory with
// an event: whoever needs the total waits for the event, not for the stream
// (gen_snap: the [S] words that receive the scenes' keypoint generation, or nullptr)
static int features_and_total(mmw_ctx *c, float *feat, int32_t *owner, int32_t *uid, int32_t cap_rows, int32_t *h_total, hipEvent_t ev,
                              int32_t *gen_snap = nullptr)
{
    EventPair ep;
    launch_feat_scan(c->dc, c->st, c->d_row_off, c->stream);
    prof_begin(c, MMW_K_FEATURES, ep);
    launch_features(c->dc, sites_or_null(c), c->st, c->d_row_off, feat, owner, uid, cap_rows, c->stream, nullptr, nullptr, c->d_kp_gen, gen_snap);
    prof_end(c, ep);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_total, c->d_row_off + c->dc.n_scenes, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(ev, c->stream));
    return MMW_OK;
}

// the tail of a stateless entry: what its launches left behind
static int launches_done(const char *who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MMW_OK : fail(nullptr, MMW_E_HIP, "%s launch -> %s", who, hipGetErrorString(e));
}

int mmw_features_async(mmw_ctx *c, float *feat, int32_t *owner, int32_t *uid, int32_t cap_rows, int32_t ticket)
{
    if (!c || !feat || !owner || cap_rows < 0 || ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_features_async: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    // only mmw_features_wait(ticket) waits for the total
    c->feat_uid[ticket] = false;   // (a call that fails half way leaves no ticket to scatter by)
    MMW_TRY(features_and_total(c, feat, owner, uid, cap_rows, c->h_rows + ticket, c->feat_ev[ticket], uid ? kp_gen_snap(c, ticket) : nullptr));
    c->feat_cap[ticket] = cap_rows;
    c->feat_uid[ticket] = uid != nullptr;
    return MMW_OK;
}

int mmw_features_wait(mmw_ctx *c, int32_t ticket, int32_t *n_rows)
{
    if (!c || !n_rows || ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_features_wait: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->feat_ev[ticket]));
    const int32_t total = c->h_rows[ticket], cap_rows = c->feat_cap[ticket];
    *n_rows = total < cap_rows ? total : cap_rows;
    if (total > cap_rows) return fail(c, MMW_E_CAPACITY, "mmw_features: %d eligible tracks but cap_rows=%d", total, cap_rows);
    return MMW_OK;
}

int mmw_features(mmw_ctx *c, float *feat, int32_t *owner, int32_t cap_rows, int32_t *n_rows)
{
    if (!c || !feat || !owner || !n_rows || cap_rows < 0) return fail(c, MMW_E_ARG, "mmw_features: bad argument");
    const int rc = mmw_features_async(c, feat, owner, nullptr, cap_rows, kTickets - 1);
    return rc ? rc : mmw_features_wait(c, kTickets - 1, n_rows);
}

int mmw_format_frames(mmw_ctx *c, const double *frames, const int32_t *counts, const double *ref, float *feat, int32_t n_items)
{
    if (!c || n_items < 0 || (n_items > 0 && (!frames || !counts || !ref || !feat))) return fail(c, MMW_E_ARG, "mmw_format_frames: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    launch_format_frames(c->dc, frames, counts, ref, feat, n_items, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_set_keypoints(mmw_ctx *c, const float *kp, const int32_t *owner, int32_t n_rows)
{
    if (!c || (n_rows > 0 && (!kp || !owner)) || n_rows < 0) return fail(c, MMW_E_ARG, "mmw_set_keypoints: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    launch_set_kp(c->dc, c->st, kp, owner, n_rows, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_set_keypoints_uid(mmw_ctx *c, const float *kp, const int32_t *owner, const int32_t *uid, int32_t n_rows)
{
    if (!c || (n_rows > 0 && (!kp || !owner || !uid)) || n_rows < 0) return fail(c, MMW_E_ARG, "mmw_set_keypoints_uid: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    launch_set_kp_uid(c->dc, c->st, kp, owner, uid, n_rows, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

int mmw_set_keypoints_ticket(mmw_ctx *c, const float *kp, const int32_t *owner, const int32_t *uid, int32_t n_rows, int32_t ticket)
{
    if (!c || (n_rows > 0 && (!kp || !owner || !uid)) || n_rows < 0) return fail(c, MMW_E_ARG, "mmw_set_keypoints_ticket: bad argument");
    if (ticket < 0 || ticket >= kTickets) return fail(c, MMW_E_ARG, "mmw_set_keypoints_ticket: ticket %d outside [0, %d)", ticket, kTickets);
    if (!c->feat_uid[ticket])
        return fail(c, MMW_E_ARG, "mmw_set_keypoints_ticket: ticket %d holds no rows with uids (its last mmw_features_async passed uid = NULL, or there was none)", ticket);
    HIPCHK(c, hipSetDevice(c->device));
    launch_set_kp_uid(c->dc, c->st, kp, owner, uid, n_rows, c->stream, c->d_kp_gen, kp_gen_snap(c, ticket));
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

// ---- the one-scene fp32 chain (mmw_frame_posture_host, api_step.hip, runs it behind the step) ----
// (a context's ring never changes, so neither does the model it can hold: the buffers are sized once)
static int attach_posture_impl(mmw_ctx *c, const mmw_posture_model *m, int frames, const char *who)
{
    const CnnDims d = cnn_dims(frames);
    if (!posture_model_ok(m, d, false))
        return fail(c, MMW_E_ARG, "%s: null weight pointer, or Dense-1 not 16-byte aligned with a leading dimension >= %d that is a multiple of 4", who, d.flat);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_pchain) {
        const size_t cap = (size_t)c->dc.t_cap, per = d.per + d.flat + d.hidden + kCnnKpPad;   // floats per row
        HIPCHK(c, hipMalloc((void **)&c->d_pchain, cap * (per * sizeof(float) + 2 * sizeof(int32_t))));
        c->pc_feat = reinterpret_cast<float *>(c->d_pchain);
        c->pc_act = c->pc_feat + cap * d.per;
        c->pc_hidden = c->pc_act + cap * d.flat;
        c->pc_kp = c->pc_hidden + cap * d.hidden;
        c->pc_owner = reinterpret_cast<int32_t *>(c->pc_kp + cap * kCnnKpPad);
    }
    c->model = *m;
    c->model_frames = frames;
    c->has_model = true;
    return MMW_OK;
}

int mmw_attach_posture(mmw_ctx *c, const mmw_posture_model *m)
{
    if (!c) return fail(c, MMW_E_ARG, "mmw_attach_posture: null context");
    if (!m) { c->has_model = false; return MMW_OK; }
    if (c->dc.n_scenes != 1 || c->dc.ring != 3 || c->dc.t_cap > 64)
        return fail(c, MMW_E_ARG, "mmw_attach_posture: a one-scene context of the 3-frame model (FB_FRAMES_BATCH = 2) with track_cap <= 64");
    return attach_posture_impl(c, m, 3, "mmw_attach_posture");
}

// the `frames` argument of the _frames entries: 3 or 1, and the context's ring
static int frames_ok(mmw_ctx *c, int32_t frames, const char *who)
{
    if ((frames != 3 && frames != 1) || c->dc.ring != frames)
        return fail(c, MMW_E_ARG, "%s: frames = %d must be 3 (define_CNN_3D) or 1 (define_CNN) and the context's FB_FRAMES_BATCH + 1, this context has FB_FRAMES_BATCH = %d",
                    who, frames, c->dc.ring - 1);
    return MMW_OK;
}

int mmw_attach_posture_frames(mmw_ctx *c, const mmw_posture_model *m, int32_t frames)
{
    if (!c) return fail(c, MMW_E_ARG, "mmw_attach_posture_frames: null context");
    if (!m) { c->has_model = false; return MMW_OK; }
    MMW_TRY(frames_ok(c, frames, "mmw_attach_posture_frames"));
    if (c->dc.n_scenes != 1 || c->dc.t_cap > 64)
        return fail(c, MMW_E_ARG, "mmw_attach_posture_frames: a one-scene context with track_cap <= 64");
    return attach_posture_impl(c, m, frames, "mmw_attach_posture_frames");
}

// ---- the stateless entries over the CNN kernels ----
int mmw_mars_conv3d(void *hip_stream, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2,
                    float *out, int32_t n)
{
    if (n < 0 || (n > 0 && (!feat || !w1 || !b1 || !w2 || !b2 || !out))) return fail(nullptr, MMW_E_ARG, "mmw_mars_conv3d: bad argument");
    launch_mars_conv(feat, w1, b1, w2, b2, out, n, (hipStream_t)hip_stream);
    return launches_done("mmw_mars_conv3d");
}

int mmw_mars_conv2d(void *hip_stream, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2,
                    float *out, int32_t n)
{
    if (n < 0 || (n > 0 && (!feat || !w1 || !b1 || !w2 || !b2 || !out))) return fail(nullptr, MMW_E_ARG, "mmw_mars_conv2d: bad argument");
    if (n == 0) return MMW_OK;
    launch_mars_conv2d(feat, w1, b1, w2, b2, out, n, (hipStream_t)hip_stream);
    return launches_done("mmw_mars_conv2d");
}

int mmw_mars_conv_split(void *hip_stream, int32_t frames, const float *feat, const float *w1, const float *b1, const float *w2,
                        const float *b2, void *out16, int64_t ld_out, int32_t n, int32_t *range_flag, int32_t *sample_flags)
{
    if ((frames != 3 && frames != 1) || n < 0 || ld_out < 2 * (int64_t)frames * 2048 || (ld_out & 7) != 0 || ((uintptr_t)out16 & 15) != 0 ||
        (n > 0 && (!feat || !w1 || !b1 || !w2 || !b2 || !out16)))
        return fail(nullptr, MMW_E_ARG, "mmw_mars_conv_split: bad argument (frames must be 3 or 1, ld_out >= 2 * frames * 2048 and a multiple of 8)");
    if (launch_mars_conv16(frames, feat, w1, b1, w2, b2, out16, ld_out, n, range_flag, sample_flags, (hipStream_t)hip_stream) != 0)
        return fail(nullptr, MMW_E_HIP, "mmw_mars_conv_split: hipFuncSetAttribute(max dynamic LDS) failed on this device");
    return launches_done("mmw_mars_conv_split");
}

int mmw_mars_dense1_split(void *hip_stream, const void *a2, int64_t lda, const void *w2, int64_t ldw, const float *bias, float *out,
                          int32_t rows_padded, int32_t k, int32_t n)
{
    if (rows_padded < 0 || (rows_padded & 255) != 0 || k < 32 || (k & 31) != 0 || n < 128 || (n & 127) != 0 || lda < 2 * (int64_t)k || ldw < 2 * (int64_t)k ||
        ((lda | ldw) & 7) != 0 || (rows_padded > 0 && (!a2 || !w2 || !bias || !out)) || (((uintptr_t)a2 | (uintptr_t)w2) & 15) != 0)
        return fail(nullptr, MMW_E_ARG, "mmw_mars_dense1_split: rows_padded must be a multiple of 256, k of 32, n of 128; fp16 operands 16-byte aligned with leading dimensions >= 2 k that are multiples of 8");
    if (rows_padded == 0) return MMW_OK;
    if (launch_mars_dense1(a2, lda, w2, ldw, bias, out, rows_padded, k, n, (hipStream_t)hip_stream) != 0)
        return fail(nullptr, MMW_E_HIP, "mmw_mars_dense1_split: hipFuncSetAttribute failed");
    return launches_done("mmw_mars_dense1_split");
}

int mmw_mars_dense1_plan(int32_t rows_padded, int32_t n, int32_t out[4])
{
    if (!out || rows_padded < 0 || (rows_padded & 255) != 0 || n < 128 || (n & 127) != 0)
        return fail(nullptr, MMW_E_ARG, "mmw_mars_dense1_plan: rows_padded must be a multiple of 256, n of 128");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(nullptr, MMW_E_NODEVICE, "mmw_mars_dense1_plan: no current HIP device");
    const int n_cu = mars_dense1_cus(dev);
    const Dense1Plan p = mars_dense1_plan(rows_padded, n, n_cu);
    out[0] = p.bands192; out[1] = p.bands128; out[2] = p.bands_half; out[3] = n_cu;
    return MMW_OK;
}

int mmw_mars_head_small(void *hip_stream, const float *act, int64_t lda, const float *w1, int64_t ldw, const float *bias1, const float *w2,
                        const float *bias2, float *hidden, float *kp, int32_t n_rows, int32_t k, int32_t n1)
{
    if (n_rows < 0 || n_rows > 64 || k < 4 || (k & 3) != 0 || n1 < 1 || lda < k || ldw < k || ((lda | ldw) & 3) != 0 ||
        (n_rows > 0 && (!act || !w1 || !bias1 || !w2 || !bias2 || !hidden || !kp)) || (((uintptr_t)act | (uintptr_t)w1) & 15) != 0)
        return fail(nullptr, MMW_E_ARG, "mmw_mars_head_small: n_rows in [0, 64], k a multiple of 4, 16-byte aligned fp32 operands with leading dimensions >= k that are multiples of 4");
    if (n_rows == 0) return MMW_OK;
    launch_mars_head_small(act, lda, w1, ldw, bias1, w2, bias2, hidden, kp, n_rows, k, n1, MMW_NKP, (hipStream_t)hip_stream);
    return launches_done("mmw_mars_head_small");
}

// (the model's weights as the struct of the attach entries: dense1_ld is the entries' ldw)
static int range_fixup_impl(const char *who, void *hip_stream, int frames, const float *feat, int32_t *sample_flags, int32_t n, const mmw_posture_model &m,
                            void *scratch, float *kp, int32_t *range_flag)
{
    constexpr int kCap = MMW_RANGE_FIXUP_CAP;
    const CnnDims d = cnn_dims(frames);
    if (n < 0 || (n > 0 && (!feat || !sample_flags || !m.conv1_w || !m.conv1_b || !m.conv2_w || !m.conv2_b || !m.dense1_w || !m.dense1_b || !m.dense2_w ||
                            !m.dense2_b || !scratch || !kp)) ||
        m.dense1_ld < d.flat || (m.dense1_ld & 3) != 0 || (((uintptr_t)scratch | (uintptr_t)m.dense1_w) & 15) != 0)
        return fail(nullptr, MMW_E_ARG, "%s: bad argument", who);
    if (n == 0) return MMW_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    // scratch: small_feat[64][per], act[64][flat], hidden[64][hidden], kp_small[64][57] floats (behind 512 spare bytes; the 3-frame
    // model's 960 / 6144 / 1536 are what MMW_RANGE_FIXUP_SCRATCH holds, the single-frame model's 320 / 2048 / 512 fit inside);
    // sample_flags = the fix-up list k_mars_conv16 appended to: [0] running count, [1] taken by this call, [2 ..] sample indices
    float *small = reinterpret_cast<float *>(reinterpret_cast<char *>(scratch) + 512);
    float *act = small + (size_t)kCap * d.per, *hidden = act + (size_t)kCap * d.flat, *kps = hidden + (size_t)kCap * d.hidden;
    launch_range_gather(feat, sample_flags, n, d.per, kCap, small, range_flag, st);
    launch_mars_small_f32(frames, small, m, act, hidden, kps, kCap, st, sample_flags + 1);
    launch_range_scatter(kps, sample_flags, kp, kCap, MMW_NKP, n, st);
    return launches_done(who);
}

int mmw_mars_range_fixup(void *hip_stream, const float *feat, int32_t *sample_flags, int32_t n, const float *cw1, const float *cb1,
                         const float *cw2, const float *cb2, const float *w1, int64_t ldw, const float *bias1, const float *w2, const float *bias2,
                         void *scratch, float *kp, int32_t *range_flag)
{
    return range_fixup_impl("mmw_mars_range_fixup", hip_stream, 3, feat, sample_flags, n, {cw1, cb1, cw2, cb2, w1, ldw, bias1, w2, bias2}, scratch, kp, range_flag);
}

int mmw_mars_range_fixup_frames(void *hip_stream, int32_t frames, const float *feat, int32_t *sample_flags, int32_t n, const float *cw1,
                                const float *cb1, const float *cw2, const float *cb2, const float *w1, int64_t ldw, const float *bias1,
                                const float *w2, const float *bias2, void *scratch, float *kp, int32_t *range_flag)
{
    if (frames != 3 && frames != 1) return fail(nullptr, MMW_E_ARG, "mmw_mars_range_fixup_frames: frames = %d must be 3 or 1 (FB_FRAMES_BATCH + 1)", frames);
    return range_fixup_impl("mmw_mars_range_fixup_frames", hip_stream, frames, feat, sample_flags, n, {cw1, cb1, cw2, cb2, w1, ldw, bias1, w2, bias2}, scratch,
                            kp, range_flag);
}

int mmw_mars_dense2(void *hip_stream, const float *hidden, int64_t ldh, const float *w2, const float *bias2, float *kp, int32_t n_rows, int32_t k)
{
    if (n_rows < 0 || k < 4 || (k & 3) != 0 || ldh < k || (ldh & 3) != 0 || !hidden || !w2 || !bias2 || !kp ||
        (((uintptr_t)hidden | (uintptr_t)w2) & 15) != 0)
        return fail(nullptr, MMW_E_ARG, "mmw_mars_dense2: n_rows >= 0, k a multiple of 4, 16-byte aligned fp32 operands, ldh >= k and a multiple of 4");
    if (n_rows == 0) return MMW_OK;
    launch_mars_dense2(hidden, ldh, w2, bias2, kp, n_rows, k, (hipStream_t)hip_stream);
    return launches_done("mmw_mars_dense2");
}

int mmw_mars_split_weights(void *hip_stream, const float *w, int64_t ldw, void *w16, int64_t ld16, int32_t n, int32_t k, int32_t *range_flag)
{
    if (n < 0 || k < 32 || (k & 31) != 0 || ldw < k || (ldw & 3) != 0 || ld16 < 2 * (int64_t)k || (ld16 & 7) != 0 || !w || !w16 ||
        (((uintptr_t)w | (uintptr_t)w16) & 15) != 0)
        return fail(nullptr, MMW_E_ARG, "mmw_mars_split_weights: n >= 0, k a multiple of 32, w fp32 16-byte aligned with ldw >= k a multiple of 4, w16 16-byte aligned with ld16 >= 2 k a multiple of 8");
    if (n == 0) return MMW_OK;
    launch_split_weights(w, ldw, w16, ld16, n, k, range_flag, (hipStream_t)hip_stream);
    return launches_done("mmw_mars_split_weights");
}

// ---- the batched TrackBuffer.estimate_posture (Tracking.py:705-734) behind the C-ABI: any number of scenes, no torch ----
static int posture_detach(mmw_ctx *c)
{
    if (c->pb) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        posture_batch_free(c->pb);
        c->pb = nullptr;
    }
    return MMW_OK;
}

// (indexed: the entry takes an array of models and its messages name the offending one)
static int posture_attach_impl(mmw_ctx *c, const mmw_posture_model *models, int n_models, bool indexed, int frames, const int32_t *scene_model,
                               int32_t cap_rows, const char *who)
{
    const CnnDims d = cnn_dims(frames);
    const int S = c->dc.n_scenes;
    char at[32] = "";
    auto name = [&](int i) { if (indexed) snprintf(at, sizeof(at), " model %d:", i); return at; };
    if (cap_rows < 1) return fail(c, MMW_E_ARG, "%s: cap_rows = %d must be >= 1", who, cap_rows);
    if (cap_rows > INT32_MAX - 255 - 256 * MMW_POSTURE_MODELS_MAX) return fail(c, MMW_E_ARG, "%s: cap_rows = %d is too large", who, cap_rows);
    for (int i = 0; i < n_models; i++)
        if (!posture_model_ok(models + i, d, true))
            return fail(c, MMW_E_ARG, "%s:%s null weight pointer, or Dense-1 / Dense-2 not 16-byte aligned, or Dense-1's leading dimension not a multiple of 4 that is >= %d", who, name(i), d.flat);
    for (int s = 0; scene_model && s < S; s++)
        if (scene_model[s] < MMW_POSTURE_NONE || scene_model[s] >= n_models)
            return fail(c, MMW_E_ARG, "%s: scene %d is given model %d, there are %d models (MMW_POSTURE_NONE = -1: no model)", who, s, scene_model[s], n_models);
    HIPCHK(c, hipSetDevice(c->device));
    PostureBatch *b = new (std::nothrow) PostureBatch();
    if (!b) return fail(c, MMW_E_HIP, "%s: out of host memory", who);
    b->n_models = n_models;
    for (int i = 0; i < n_models; i++) b->model[i] = models[i];
    b->frames = frames;
    b->cap = cap_rows;
    const size_t cap = (((size_t)cap_rows + 255) & ~(size_t)255) + (n_models > 1 ? 256 * (size_t)n_models : 0);
    b->rows = (int32_t)cap;
    b->h_map.assign((size_t)S, 0);
    if (scene_model) b->h_map.assign(scene_model, scene_model + S);
    posture_refresh_grouped(b);
    const size_t n_lists = kPbWordList + (size_t)n_models * pb_list_words, n_words = n_lists + MMW_POSTURE_MODELS_MAX;
    hipError_t e = hipSuccess;
    auto grab = [&](void **p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    grab((void **)&b->feat, cap * d.per * sizeof(float));
    grab((void **)&b->owner, cap * 2 * sizeof(int32_t));
    grab((void **)&b->uid, cap * sizeof(int32_t));
    grab(&b->act16, cap * (size_t)pb_act_ld(d) * 2);
    grab((void **)&b->hidden, cap * d.hidden * sizeof(float));
    grab((void **)&b->kp, cap * MMW_NKP * sizeof(float));
    grab((void **)&b->words, n_words * sizeof(int32_t));
    grab(&b->fix_scratch, MMW_RANGE_FIXUP_SCRATCH);
    for (int i = 0; i < n_models; i++) grab(&b->w16[i], (size_t)d.hidden * 2 * d.flat * 2);
    grab((void **)&b->d_map, (size_t)S * sizeof(int32_t));
    grab((void **)&b->d_groups, 16 * sizeof(int32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_total, 16 * sizeof(int32_t));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&b->total_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(b->words, 0, n_words * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_groups, 0, 16 * sizeof(int32_t), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_map, b->h_map.data(), (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    int32_t bad[MMW_POSTURE_MODELS_MAX] = {};
    if (e == hipSuccess) {
        // every model's split Dense-1 operand, once; every weight that meets the split arithmetic must lie inside fp16's range
        for (int i = 0; i < n_models; i++) {
            const mmw_posture_model *m = models + i;
            int32_t *flag = b->words + n_lists + i;
            launch_split_weights(m->dense1_w, m->dense1_ld, b->w16[i], 2 * d.flat, d.hidden, d.flat, flag, c->stream);
            launch_range_check(m->conv1_w, d.taps * 5 * 16, flag, c->stream);
            launch_range_check(m->conv1_b, 16, flag, c->stream);
            launch_range_check(m->conv2_w, d.taps * 16 * 32, flag, c->stream);
            launch_range_check(m->conv2_b, 32, flag, c->stream);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(bad, b->words + n_lists, sizeof(bad), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) {
        hipStreamSynchronize(c->stream);   // (the map's copy may still be reading the mirror that is about to go)
        posture_batch_free(b);
        return fail(c, MMW_E_HIP, "%s: %s (cap_rows = %d, %d model(s))", who, hipGetErrorString(e), cap_rows, n_models);
    }
    for (int i = 0; i < n_models; i++) {
        if (!bad[i]) continue;
        posture_batch_free(b);
        return fail(c, MMW_E_ARG, "%s:%s a conv or Dense-1 weight is not finite or has a magnitude >= 65504: outside fp16's range, where the split arithmetic of this path is not exact (use a one-scene context's fp32 path, mmw_attach_posture, for such a model)", who, name(i));
    }
    if (c->pb) posture_batch_free(c->pb);   // (the stream was waited for above: nothing of the old chain is running)
    c->pb = b;
    return MMW_OK;
}

int mmw_posture_attach(mmw_ctx *c, const mmw_posture_model *m, int32_t cap_rows)
{
    if (!c) return fail(c, MMW_E_ARG, "mmw_posture_attach: null context");
    if (!m) return posture_detach(c);
    if (c->dc.ring != 3) return fail(c, MMW_E_ARG, "mmw_posture_attach: the 3-frame model only (FB_FRAMES_BATCH = 2), this context has FB_FRAMES_BATCH = %d", c->dc.ring - 1);
    return posture_attach_impl(c, m, 1, false, 3, nullptr, cap_rows, "mmw_posture_attach");
}

int mmw_posture_attach_models(mmw_ctx *c, const mmw_posture_model *models, int32_t n_models, int32_t frames, const int32_t *scene_model, int32_t cap_rows)
{
    if (!c) return fail(c, MMW_E_ARG, "mmw_posture_attach_models: null context");
    if (!models) return fail(c, MMW_E_ARG, "mmw_posture_attach_models: models is NULL (mmw_posture_attach(ctx, NULL, 0) detaches)");
    if (n_models < 1 || n_models > MMW_POSTURE_MODELS_MAX)
        return fail(c, MMW_E_ARG, "mmw_posture_attach_models: n_models = %d must be 1 .. %d", n_models, MMW_POSTURE_MODELS_MAX);
    MMW_TRY(frames_ok(c, frames, "mmw_posture_attach_models"));
    return posture_attach_impl(c, models, n_models, true, frames, scene_model, cap_rows, "mmw_posture_attach_models");
}

int mmw_posture_set_scene_models(mmw_ctx *c, const int32_t *scenes, int32_t n, const int32_t *model_of)
{
    if (!c) return fail(nullptr, MMW_E_ARG, "mmw_posture_set_scene_models: null context");
    PostureBatch *b = c->pb;
    if (!b) return fail(c, MMW_E_ARG, "mmw_posture_set_scene_models: no model attached (mmw_posture_attach_models)");
    const int S = c->dc.n_scenes;
    // every check first: a refused call changes no scene's model
    if (n < 0 || n > S) return fail(c, MMW_E_ARG, "mmw_posture_set_scene_models: n = %d, the context has %d scenes", n, S);
    if (n > 0 && !model_of) return fail(c, MMW_E_ARG, "mmw_posture_set_scene_models: model_of is NULL with n = %d", n);
    std::vector<char> seen(scenes ? (size_t)S : 0, 0);
    for (int i = 0; i < n; i++) {
        const int s = scenes ? scenes[i] : i;
        if (s < 0 || s >= S) return fail(c, MMW_E_ARG, "mmw_posture_set_scene_models: entry %d names scene %d, the context has %d scenes", i, s, S);
        if (scenes) {
            if (seen[s]) return fail(c, MMW_E_ARG, "mmw_posture_set_scene_models: entry %d names scene %d a second time", i, s);
            seen[s] = 1;
        }
        if (model_of[i] < MMW_POSTURE_NONE || model_of[i] >= b->n_models)
            return fail(c, MMW_E_ARG, "mmw_posture_set_scene_models: entry %d (scene %d) asks for model %d, there are %d models (MMW_POSTURE_NONE = -1: no model)", i, s, model_of[i], b->n_models);
    }
    HIPCHK(c, hipSetDevice(c->device));
    // the new map is put together on the host and travels as ONE copy, ordered on the context's stream (as mmw_set_sites' table)
    std::vector<int32_t> next = b->h_map;
    for (int i = 0; i < n; i++) next[scenes ? scenes[i] : i] = model_of[i];
    HIPCHK(c, hipMemcpyAsync(b->d_map, next.data(), sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (`next` is pageable and goes away)
    b->h_map.swap(next);
    posture_refresh_grouped(b);
    return MMW_OK;
}

int mmw_posture_get_scene_models(mmw_ctx *c, int32_t *out)
{
    if (!c || !out) return fail(c, MMW_E_ARG, "mmw_posture_get_scene_models: null argument");
    if (!c->pb) return fail(c, MMW_E_ARG, "mmw_posture_get_scene_models: no model attached (mmw_posture_attach_models)");
    memcpy(out, c->pb->h_map.data(), c->pb->h_map.size() * sizeof(int32_t));   // (the host mirror: no device access)
    return MMW_OK;
}

int mmw_posture_group_rows(mmw_ctx *c, int32_t *rows, int32_t *n_models)
{
    if (!c || !rows || !n_models) return fail(c, MMW_E_ARG, "mmw_posture_group_rows: null argument");
    if (!c->pb) return fail(c, MMW_E_ARG, "mmw_posture_group_rows: no model attached (mmw_posture_attach_models)");
    for (int i = 0; i < c->pb->n_models; i++) rows[i] = c->pb->last_total[i];
    *n_models = c->pb->n_models;
    return MMW_OK;
}

int mmw_posture_owners(mmw_ctx *c, int32_t *owner, int32_t cap, int32_t *n_rows)
{
    if (!c || !n_rows || cap < 0 || (cap > 0 && !owner)) return fail(c, MMW_E_ARG, "mmw_posture_owners: bad argument");
    PostureBatch *b = c->pb;
    if (!b) return fail(c, MMW_E_ARG, "mmw_posture_owners: no model attached (mmw_posture_attach_models)");
    int64_t total = 0;
    for (int i = 0; i < b->n_models; i++) total += b->last_total[i];
    if (total > cap) return fail(c, MMW_E_CAPACITY, "mmw_posture_owners: the last call estimated %lld rows but cap=%d (nothing was written)", (long long)total, cap);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int32_t *dst = owner;
    for (int i = 0; i < b->n_models; i++) {   // band by band, without the padding between them
        if (b->last_total[i] <= 0) continue;
        HIPCHK(c, hipMemcpyAsync(dst, b->owner + (size_t)b->last_base[i] * 2, (size_t)b->last_total[i] * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        dst += (size_t)b->last_total[i] * 2;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_rows = (int32_t)total;
    return MMW_OK;
}

int mmw_posture_attach_frames(mmw_ctx *c, const mmw_posture_model *m, int32_t frames, int32_t cap_rows)
{
    if (!c) return fail(c, MMW_E_ARG, "mmw_posture_attach_frames: null context");
    if (!m) return posture_detach(c);
    MMW_TRY(frames_ok(c, frames, "mmw_posture_attach_frames"));
    return posture_attach_impl(c, m, 1, false, frames, nullptr, cap_rows, "mmw_posture_attach_frames");
}

// one band of a call: the chain of the CNN kernels on `total` rows from row `base` of the shared buffers (a multiple of 256), with
// model i's weights, split operand and fix-up list, then track.keypoints = the band's rows
static int posture_band(mmw_ctx *c, PostureBatch *b, int i, int32_t base, int32_t total)
{
    const mmw_posture_model &m = b->model[i];
    const CnnDims d = cnn_dims(b->frames);
    const long long act_ld = pb_act_ld(d);
    const int rows_padded = (total + 255) & ~255;
    int32_t *range = b->words + kPbWordRange, *list = b->words + kPbWordList + (size_t)i * pb_list_words;
    float *feat = b->feat + (size_t)base * d.per, *hidden = b->hidden + (size_t)base * d.hidden, *kp = b->kp + (size_t)base * MMW_NKP;
    void *act16 = reinterpret_cast<char *>(b->act16) + (size_t)base * (size_t)act_ld * 2;
    if (launch_mars_conv16(b->frames, feat, m.conv1_w, m.conv1_b, m.conv2_w, m.conv2_b, act16, act_ld, total, range, list, c->stream) != 0 ||
        launch_mars_dense1(act16, act_ld, b->w16[i], 2 * d.flat, m.dense1_b, hidden, rows_padded, d.flat, d.hidden, c->stream) != 0)
        return fail(c, MMW_E_HIP, "mmw_estimate_posture: hipFuncSetAttribute(max dynamic LDS) failed on this device");
    launch_mars_dense2(hidden, d.hidden, m.dense2_w, m.dense2_b, kp, total, d.hidden, c->stream);
    HIPCHK(c, hipGetLastError());
    const int rc = range_fixup_impl("mmw_mars_range_fixup", c->stream, b->frames, feat, list, total, m, b->fix_scratch, kp, range);
    if (rc) return fail(c, rc, "mmw_estimate_posture: %s", mmw_last_error(nullptr));
    launch_set_kp(c->dc, c->st, kp, b->owner + (size_t)base * 2, total, c->stream);
    HIPCHK(c, hipGetLastError());
    return MMW_OK;
}

// mmw_estimate_posture of a context with several models, or with scenes on MMW_POSTURE_NONE: rows model by model
static int estimate_posture_grouped(mmw_ctx *c, PostureBatch *b, int32_t *n_rows)
{
    EventPair ep;
    launch_feat_count(c->dc, c->st, c->d_row_off, c->stream);
    launch_feat_scan_models(c->dc.n_scenes, b->n_models, b->rows, b->d_map, c->d_row_off, b->d_groups, c->stream);
    prof_begin(c, MMW_K_FEATURES, ep);
    // (cap_rows = the buffers' rows: an excluded scene's offset, and whatever a call that exceeds cap_rows would place behind them)
    launch_features(c->dc, sites_or_null(c), c->st, c->d_row_off, b->feat, b->owner, b->uid, b->rows, c->stream);
    prof_end(c, ep);
    HIPCHK(c, hipGetLastError());
    // every band's total and base in ONE copy; the host waits for them (not for the stream)
    HIPCHK(c, hipMemcpyAsync(b->h_total, b->d_groups, 16 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(b->total_ev, c->stream));
    HIPCHK(c, hipEventSynchronize(b->total_ev));
    int64_t total = 0;
    for (int i = 0; i < b->n_models; i++) total += b->h_total[i];
    if (total > b->cap)
        return fail(c, MMW_E_CAPACITY, "mmw_estimate_posture: %lld eligible tracks over %d models but cap_rows=%d (no keypoint was changed)", (long long)total, b->n_models, b->cap);
    for (int i = 0; i < b->n_models; i++) {
        b->last_total[i] = b->h_total[i];
        b->last_base[i] = b->h_total[8 + i];
        if (b->h_total[i] > 0) MMW_TRY(posture_band(c, b, i, b->h_total[8 + i], b->h_total[i]));
    }
    if (n_rows) *n_rows = (int32_t)total;
    return MMW_OK;
}

int mmw_estimate_posture(mmw_ctx *c, int32_t *n_rows)
{
    if (n_rows) *n_rows = 0;
    if (!c) return fail(c, MMW_E_ARG, "mmw_estimate_posture: null context");
    PostureBatch *b = c->pb;
    if (!b) return fail(c, MMW_E_ARG, "mmw_estimate_posture: no model attached (mmw_posture_attach)");
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < b->n_models; i++) b->last_total[i] = b->last_base[i] = 0;   // (a refused or empty call estimated nothing)
    if (b->grouped) return estimate_posture_grouped(c, b, n_rows);
    // one model, every scene on it: one band from row 0, behind k_feat_scan
    // the matrix kernels need their exact batch size: the host waits for the total (not for the stream)
    MMW_TRY(features_and_total(c, b->feat, b->owner, b->uid, b->cap, b->h_total, b->total_ev));
    HIPCHK(c, hipEventSynchronize(b->total_ev));
    const int32_t total = *b->h_total;
    if (total > b->cap) return fail(c, MMW_E_CAPACITY, "mmw_estimate_posture: %d eligible tracks but cap_rows=%d (no keypoint was changed)", total, b->cap);
    if (total <= 0) return MMW_OK;
    b->last_total[0] = total;
    MMW_TRY(posture_band(c, b, 0, 0, total));
    if (n_rows) *n_rows = total;
    return MMW_OK;
}

int mmw_posture_range(mmw_ctx *c, int32_t *word)
{
    if (!c || !word) return fail(c, MMW_E_ARG, "mmw_posture_range: null argument");
    if (!c->pb) return fail(c, MMW_E_ARG, "mmw_posture_range: no model attached (mmw_posture_attach)");
    HIPCHK(c, hipSetDevice(c->device));
    int32_t w = 0;
    MMW_TRY(d2h_after_kernels(c, &w, c->pb->words + kPbWordRange, sizeof(w)));
    if (w) {
        HIPCHK(c, hipMemsetAsync(c->pb->words + kPbWordRange, 0, sizeof(int32_t), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *word = w;
    return MMW_OK;
}
