// k_skeleton.hip -- the live tracks' room-frame skeletons (mmw_skeletons_*): every track's 57 keypoints mirrored and shifted to the
// track's position, with the plausibility check of Visualizer.update_posture (Visualizer.py:265-307), compacted into one output in
// the report's (scene, slot) order.  Reads SceneHdr, order and TrackRec after the step, the way k_report and k_cloud do; nothing of
// the step is touched, nothing is written to the state and nothing is kept between two calls.
//   k_skel_count   emitted entries and live tracks per scene: a wave per scene, a lane per track (t_cap <= 64)
//   k_pair_scan    (k_scan.hip) one workgroup: the two offset scans (emitted entries -> the position, all live tracks -> `row`),
//                  the capacity decision on the emitted total, the totals
//   k_skel_write   a wave per scene: 16 lanes own one entry's sixteen 16-byte pieces -- only if everything fits
//
// The arithmetic (include/mmw.h): kp viewed as reshape(3, 19), row 1 the height, row 2 the depth.
//   g_c = fp32(kp[19c + 1] - kp[19c + 2]);  s = (g_0^2 + g_1^2) + g_2^2 in fp64;  skipped iff s > 0.25;  gap = fp32(sqrt(s))
//   joint[j] = { fp32(-(double)kp[j] + x[0]), fp32((double)kp[38 + j] + x[1]), kp[19 + j] }      one rounding each, from fp64
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_math.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

static_assert(sizeof(mmw_skeleton) == 256 && alignof(mmw_skeleton) == 4, "mmw_skeleton");
static_assert(offsetof(mmw_skeleton, gap) == 20 && offsetof(mmw_skeleton, joint) == 24 && offsetof(mmw_skeleton, reserved_) + 4 == sizeof(mmw_skeleton),
              "mmw_skeleton has no padding");
static_assert(MMW_NKP == 57, "19 joints of three coordinates");
static_assert(MMW_TRACK_CAP_LIMIT <= 64, "one lane per track");

constexpr int kSkelJoints = 19;
constexpr int kSkelPieces = sizeof(mmw_skeleton) / 16;   // 16: an entry is sixteen 16-byte pieces, a wave stores four entries at once
constexpr int kSkelHead = 6;                             // words in front of joint[0][0]

// The reference's check on one track (all lanes may call; a lane without a track passes nullptr and is never skipped).
struct SkelCheck { bool skipped; float gap; };
__device__ __forceinline__ SkelCheck skel_check(const TrackRec *rec)
{
    SkelCheck c{false, 0.f};
    if (!rec) return c;
    const float g0 = rec->kp[1] - rec->kp[2];
    const float g1 = rec->kp[kSkelJoints + 1] - rec->kp[kSkelJoints + 2];
    const float g2 = rec->kp[2 * kSkelJoints + 1] - rec->kp[2 * kSkelJoints + 2];
    const double s = ((double)g0 * (double)g0 + (double)g1 * (double)g1) + (double)g2 * (double)g2;
    c.skipped = s > 0.25;   // (false for a NaN: the reference draws such a track)
    c.gap = (float)sqrt(s);
    return c;
}

// The record of the track in list position `lane` of scene `s`, nullptr past the scene's T tracks.
__device__ __forceinline__ const TrackRec *skel_track(const DevCfg &cfg, const DevState &st, int s, int lane, int T)
{
    if (lane >= T) return nullptr;
    return st.trk + (size_t)s * cfg.t_cap + live_slot(cfg, st, s, lane);
}

__global__ __launch_bounds__(256) void k_skel_count(DevCfg cfg, DevState st, ExportScratch sc, int mode)
{
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= cfg.n_scenes) return;   // (wave-uniform)
    const int T = live_tracks(cfg, st, s);
    const unsigned long long skipped = __ballot(skel_check(skel_track(cfg, st, s, lane, T)).skipped);
    if (lane == 0) {
        sc.off[s] = mode == MMW_SKEL_DRAWN ? T - __popcll(skipped) : T;
        sc.off[cfg.n_scenes + 1 + s] = T;
    }
}

// Where word w (0 .. 63) of an entry comes from: the keypoint it is formed from (any valid index for the words that need none, so
// that the load can always be issued) and which of the three joint rules applies.
struct SkelSrc { int kp, c; };
__device__ __forceinline__ SkelSrc skel_src(int w)
{
    const int q = min(max(w - kSkelHead, 0), MMW_NKP - 1), j = q / 3, c = q - 3 * j;
    return SkelSrc{c == 0 ? j : (c == 1 ? 2 * kSkelJoints + j : kSkelJoints + j), c};
}
// Word w of an entry from its keypoint k (skel_src), the track's position and the six words in front of the joints.  No branch.
__device__ __forceinline__ uint32_t skel_word(int w, int c, float k, double x0, double x1, const int (&head)[kSkelHead])
{
    const double v = c == 0 ? -(double)k + x0 : (double)k + x1;
    uint32_t r = __float_as_uint(c == 2 ? k : (float)v);
#pragma unroll
    for (int h = 0; h < kSkelHead; h++) r = (w == h) ? (uint32_t)head[h] : r;
    return w >= kSkelHead + MMW_NKP ? 0u : r;   // reserved_
}

// A wave per scene.  First a lane per track: the check, balloted, gives every track its position in the output (its rank among
// the scene's emitted entries).  Then the wave takes four tracks at a time: 16 lanes own one entry's 16 pieces, each lane loads the
// four keypoints its words are formed from, forms the words without a branch and stores them as ONE 16-byte piece -- the 16 lanes of an entry write its 256
// bytes contiguously, the wave 1 KiB per instruction in MMW_SKEL_ALL.  A skipped track's lanes store nothing in MMW_SKEL_DRAWN.
__global__ __launch_bounds__(256) void k_skel_write(DevCfg cfg, DevState st, ExportScratch sc, mmw_skeleton *__restrict__ out, int mode, int scene_base)
{
    if (!sc.totals[2]) return;   // (uniform over the launch) the entries do not fit: nothing is written
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, S = cfg.n_scenes;
    if (s >= S) return;          // (wave-uniform)
    const int T = live_tracks(cfg, st, s);
    const int row0 = sc.off[S + 1 + s], e0 = sc.off[s];

    const TrackRec *mine = skel_track(cfg, st, s, lane, T);
    const SkelCheck chk = skel_check(mine);
    const unsigned long long skipped = __ballot(chk.skipped);
    const int drawn_before = __popcll(~skipped & lanemask_lt());
    const int my_slot = mine ? (int)(mine - (st.trk + (size_t)s * cfg.t_cap)) : 0;
    const int my_pos = e0 + (mode == MMW_SKEL_DRAWN ? drawn_before : lane);

    const int piece = lane & (kSkelPieces - 1), sub = lane >> 4;
    const SkelSrc src[4] = {skel_src(piece * 4), skel_src(piece * 4 + 1), skel_src(piece * 4 + 2), skel_src(piece * 4 + 3)};
    uint4 *out4 = reinterpret_cast<uint4 *>(out);
    for (int b = 0; b < T; b += 4) {   // (uniform)
        const int t = b + sub;         // (< 64: b <= 60)
        const int slot = __shfl(my_slot, t), pos = __shfl(my_pos, t);
        const float gap = __shfl(chk.gap, t);
        const int flag = (int)((skipped >> t) & 1ULL);
        if (t < T && !(mode == MMW_SKEL_DRAWN && flag)) {
            const TrackRec *rec = st.trk + (size_t)s * cfg.t_cap + slot;
            const int head[kSkelHead] = {scene_base + s, t, rec->uid, row0 + t, flag ? MMW_SKEL_SKIPPED : 0, (int)__float_as_uint(gap)};
            const double x0 = rec->x[0], x1 = rec->x[1];
            float k[4];
#pragma unroll
            for (int i = 0; i < 4; i++) k[i] = rec->kp[src[i].kp];   // (all four in flight before the first is used)
            uint32_t word[4];
#pragma unroll
            for (int i = 0; i < 4; i++) word[i] = skel_word(piece * 4 + i, src[i].c, k[i], x0, x1, head);
            out4[(size_t)pos * kSkelPieces + piece] = uint4{word[0], word[1], word[2], word[3]};
        }
    }
}

void launch_skeletons(const DevCfg &cfg, const DevState &s, const ExportScratch &sc, mmw_skeleton *out, int cap, int mode, int scene_base, hipStream_t st)
{
    const dim3 grid((cfg.n_scenes + 3) / 4);
    hipLaunchKernelGGL(k_skel_count, grid, dim3(256), 0, st, cfg, s, sc, mode);
    launch_pair_scan(cfg.n_scenes, sc.off, sc.totals, cap, INT32_MAX, st);   // (emitted, live: only the emitted entries need room)
    hipLaunchKernelGGL(k_skel_write, grid, dim3(256), 0, st, cfg, s, sc, out, mode, scene_base);
}

}  // namespace mmw
