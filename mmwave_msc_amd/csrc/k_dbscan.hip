// k_dbscan.hip -- the step's DBSCAN kernels and their launchers: who runs apply_DBscan + _add_tracks (Utils.py:250-291,
// Tracking.py:576-589, 697-703; the BallTree emulation itself is mmw_balltree.hpp) for which cloud, and when.
//
// Who runs it: the cloud is the concatenation of <= ring frames of UNASSIGNED points, so its
// size U varies from a few dozen (steady state: clutter only) to ring*max_pts.
//   U <= 256          256 threads, thread i owns point i with all 8 columns in registers: the worker blocks of k_post
//   U <= 1920         512 threads (thread per point up to 512, strided build above): k_dbscan_big / k_dbscan_startup
//   both, early       the 512-thread workgroups of k_chain on a side stream, while k_track and k_post are still running
// k_track pushes every scene that must cluster into one of two queues (or, without side workers, a work list); LDS is
// carved per capacity so that small clouds do not pay for the largest one.
// The queue protocol and every worker's LDS plan: mmw_dbqueue.hpp.  Behind the step's kernels: seek_inner's per-track clustering
// (k_inner) and mmw_dbscan's caller-provided clouds (k_dbscan_only, k_dbscan_only_huge).
#include <cstdlib>
#include "mmw_dbqueue.hpp"
#include "mmw_kalman.hpp"
#include "mmw_launch.hpp"
#include "mmw_dispatch.hpp"
#include "mmw_kernels.hpp"

namespace mmw {

// The small queue from k_post (the step's pushes are complete): tickets are taken with one atomicAdd -- a ticket past the
// count ends the block, and the counters are reset before their parity is used again.  (k_chain claims with a
// compare-and-swap only when an entry is there, so a worker that gives up -- bounded wait -- never holds a ticket.)
template <int NT = 256>
__device__ __forceinline__ void chain_worker_loop(const DevCfg &cfg, const DevState &st, char *lds_raw, int UMc, int CL, int UM_out, int parity,
                                                  int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    DbLds L;
    db_lds_layout<true>(UMc, CL, true, lds_raw, &L);
    ScreenScratch *scr = reinterpret_cast<ScreenScratch *>(lds_raw + post_worker_plan(UMc, CL).tree_end);
    int *ticket = scr->ticket;
    int32_t *q = st.q + parity * 8;
    int32_t *ring = st.db_list;  // list 0
    bool have = false;  // an item of this block is being finished (uniform)
    for (;;) {
        __syncthreads();  // every thread is done with the previous scene: its stores are issued, LDS is free again
        if (threadIdx.x == 0) {
            if (have) { __threadfence(); atomicAdd(&q[kQDone], 1); }
            const int h = q_claim_ticket(q);
            *ticket = h >= 0 ? q_take_entry(st, q, ring + h) : -1;
        }
        __syncthreads();
        const int s = *ticket;  // (rewritten only behind the barrier at the top of the next round)
        if (s < 0) return;
        have = true;
        SceneHdr *hdr = st.hdr + s;
        const int U = hdr->db_u;
        // (seek_inner contexts run no k_chain; k_inner may have filled the track list after k_track queued the scene: then
        //  there is no apply_DBscan this frame -- uniform)
        if (!(cfg.seek_inner && !hdr->need_db)) {
            if (cloud_pairs_prove_no_core<NT>(cfg, ring_rows_of(cfg, st, hdr, s), U, scr->P4, scr->cnt, scr->mm, scr->flag))
                cloud_finish_empty(st, hdr, s, U, UM_out, labels_out, db_n_out);
            else
                spawn_scene<NT, true>(cfg, st, L, s, UMc, CL, UM_out, true, parity, labels_out, db_n_out);
        }
    }
}

// The clouds of more than 256 points (a scene without tracks clusters its whole ring: the start-up frames, and every scene
// whose tracks have all expired): 100-250 us of BallTree chain each on a 512-thread workgroup.  They sit in a queue k_track
// fills while it runs (q[kQBig + ...], ring = list 1).  Consumers:
//   k_chain           twelve workgroups on a side stream, BESIDE k_track and k_post, for this queue and the small clouds'
//                     (claims by compare-and-swap, leaves when k_post has begun and both queues are empty; not in the
//                     start-up frames, whose pushes carry no release: cfg.big_live);
//   k_dbscan_big      behind k_post on the context's stream: takes what is left (tickets by atomicAdd: the pushes are
//                     complete) and does not end before every claimed cloud is finished;
//   k_dbscan_startup  the same for the first frames after a reset, when every cloud fits one point per thread, under a
//                     register budget that lets two workgroups share a CU;
//   k_post            in contexts of <= kSmallContextScenes scenes, whose step is launch latency: its worker blocks take the
//                     large clouds too (256 threads, strided build -- rare there) and k_dbscan_big is not launched.
// Correctness never depends on k_chain having run.
constexpr int kBigThreads = 512;
template <int NT, bool TPP_ONLY>
__device__ __forceinline__ void big_worker_loop(const DevCfg &cfg, const DevState &st, char *lds_raw, int UMc, int CL, int UM_out, int parity,
                                                int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    DbLds L;
    int *ticket = reinterpret_cast<int *>(lds_raw + big_worker_plan(UMc, CL, TPP_ONLY).tree_end);
    int32_t *q = st.q + kQBig + parity * 8;
    int32_t *ring = st.db_list + cfg.n_scenes;  // list 1
    bool have = false;
    for (;;) {
        __syncthreads();  // every thread is done with the previous cloud: its stores are issued, LDS is free again
        if (threadIdx.x == 0) {
            if (have) { __threadfence(); atomicAdd(&q[kQDone], 1); }
            int h = -1;
            if ((q_load(&q[kQHead]) & kQIdxMask) < q_load(&q[kQCount])) h = q_claim_ticket(q);  // (an empty queue costs two loads, no atomic)
            *ticket = h >= 0 ? q_take_entry(st, q, ring + h) : -1;
        }
        __syncthreads();
        const int s = *ticket;
        if (s < 0) return;
        have = true;
        if (cfg.seek_inner && !st.hdr[s].need_db) continue;  // cancelled by k_inner (uniform)
        // a cloud that fits one point per thread takes the thread-per-point build of the small class (registers
        // hold the 8 columns, one bitonic sort per level): 3-4x less tree-build time than the strided build
        const bool tpp = TPP_ONLY || st.hdr[s].db_u <= NT;  // uniform
        db_lds_layout<true>(UMc, CL, tpp, lds_raw, &L);
        if (tpp) spawn_scene<NT, true>(cfg, st, L, s, UMc, CL, UM_out, false, parity, labels_out, db_n_out);
        else if constexpr (!TPP_ONLY) spawn_scene<NT, false>(cfg, st, L, s, UMc, CL, UM_out, false, parity, labels_out, db_n_out);
    }
}

// Next frame's schedule for k_track: scenes by descending track count -- a counting sort over the scene headers by ONE 256-thread
// workgroup of k_post (its own block: as a chore of the last worker block, two passes of one dependent load per 256 scenes, it was
// the longest chain of the launch -- 18 us at 4096 scenes); the order inside a count is irrelevant.  (Scenes without tracks
// FIRST -- they are the ones that cluster their whole ring, 100-250 us on a chain worker -- was tried: no measurable gain in either
// window, and they are the filler k_track's tail wants.)  The key is n_upd, which nothing in this launch writes: n_tracks may be
// raised by a spawning worker between the two passes, and a scene counted in one bin but scattered into another would break the
// permutation.
// TWO classes, each by descending track count: first the scenes that CAN reach apply_DBscan next frame (fewer than TR_MAX_TRACKS
// tracks: Tracking.py:693-697), then the full ones.  A cloud that needs the BallTree is a 45-60 us chain that starts when its
// scene's workgroup of k_track ends; pushed from the launch's first round it is finished long before k_post, pushed from the last
// one it is what k_post's block 0 -- and with it the step -- waits for.  With "most tracks first" alone the scenes that can push
// were the LAST of the launch: at K = T block 0 left at 45-60 us in two frames of three while the update blocks were done at 35
// (scripts/wg_times_post_frames.py, NOTEBOOK round 5).  (A full scene can still trigger when a track expires in this frame's
// maintenance; rare, and correct either way -- the order is a schedule, not a decision.)
// hist: LDS, 2 (t_cap + 1) + 1 ints.  Loads in batches of eight per thread, all in flight at once.
// (192: just above a ring of clutter; same box, alternating: 256 equal within the noise, 128 -- too many scenes in front -- 3-6 % slower)
#ifndef MMW_SCHED_BIG_U   // (diagnostic builds: another ring size from which a scene leads the schedule)
#define MMW_SCHED_BIG_U 192
#endif
template <int NT = 256>
__device__ __forceinline__ void post_schedule_sort(const DevCfg &cfg, const DevState &st, int parity, int *hist)
{
    const int tid = threadIdx.x, nb = cfg.t_cap + 1, S = cfg.n_scenes;
    auto key_of = [&](int sc) {
        return sc < S ? ((st.hdr[sc].n_upd < 0 ? 0 : st.hdr[sc].n_upd) & 0xffff) | (st.hdr[sc].db_u > MMW_SCHED_BIG_U ? 0x10000 : 0) : 0;
    };
    auto bin_of = [&](int key) {
        const int t = (key & 0xffff) > cfg.t_cap ? cfg.t_cap : (key & 0xffff);
        // (in front of everything: the scenes whose ring holds MORE THAN CLUTTER -- more than MMW_SCHED_BIG_U unassigned points: a cloud that
        //  was not clustered away this frame comes back next frame, a 45-250 us chain again --, then the scenes without tracks, then the
        //  first class by descending track count.
        //  Ascending -- "the fewer tracks a scene has kept, the more of its points are unassigned" -- was measured: the launch then
        //  ends on its heaviest workgroups, mixed population + 4 %)
        if (key >> 16) return 0;
        return t == 0 ? 1 : (t < cfg.tr_max_tracks ? 1 : 1 + nb) + (nb - t);
    };
    for (int i = tid; i <= 2 * nb + 1; i += NT) hist[i] = 0;
    __syncthreads();
    for (int base = 0; base < S; base += NT * 8) {
        int key[8];
#pragma unroll
        for (int u = 0; u < 8; u++) key[u] = key_of(base + u * NT + tid);
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (base + u * NT + tid < S) atomicAdd(&hist[bin_of(key[u])], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int b = 0; b <= 2 * nb + 1; b++) { const int c = hist[b]; hist[b] = run; run += c; }
    }
    __syncthreads();
    for (int base = 0; base < S; base += NT * 8) {
        int key[8];
#pragma unroll
        for (int u = 0; u < 8; u++) key[u] = key_of(base + u * NT + tid);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int sc = base + u * NT + tid;
            if (sc < S) st.perm[(size_t)(parity ^ 1) * S + atomicAdd(&hist[bin_of(key[u])], 1)] = sc;
        }
    }
}

// k_post: what follows the association of a frame, in ONE launch of 256-thread workgroups of two kinds:
//   blocks [0, G0)   apply_DBscan + _add_tracks (Tracking.py:697-703) for the clouds of <= 256 points k_track's / k_scene's
//                    screens could not rule out (work list 3, and what k_chain has left of queue 0): the exact pair
//                    count once more (a few microseconds, for the handful of scenes per step that arrive), then the
//                    BallTree, a latency chain of ~60 us that would otherwise leave the chip idle;
//   block G0         next frame's schedule for k_track (post_schedule_sort above; not in the fused step)
//   the others       _update_all (Tracking.py:598-603) of four (scene, quarter) units each, one wave per unit
//                    (update_tracks_wave, mmw_kalman.hpp) -- the bulk work the BallTree scenes hide under.
// The two touch disjoint state: the update covers the hdr->n_upd tracks that existed before this frame's
// clusters, the spawn appends records behind them.
// Two waves per SIMD (no register cap: the BallTree path of the worker blocks takes ~205 VGPRs, the update 156).  Rounds 2-4 ran
// the launch under a 168-VGPR cap (three waves per SIMD) for the update's sake, the workers spilling 54 VGPRs / 188 bytes of
// scratch per lane; since the update's broadcasts moved from the LDS to DPP moves (round 4) the third wave buys it nothing --
// same box, alternating (scripts/ab_libs.sh, profiles/NOTEBOOK.md round 5): 4096 scenes k_post 36-38 us either way, 512 scenes
// (whose DBSCAN is all in these worker blocks) 16.6 -> 14.5 us, the step 0.0648 -> 0.0627 ms -- and nothing spills.
#ifndef MMW_POST_OCC   // (diagnostic builds: another register budget for the launch)
#define MMW_POST_OCC 2
#endif
template <int DX, int NT>
__global__ __launch_bounds__(NT, MMW_POST_OCC) void k_post(DevCfg cfg, DevState st, const int32_t *__restrict__ n_pts, int nq, int G0, int UMc, int CL,
                                              int UMb, int CLb, int UM_out, int parity, int epoch, int32_t *__restrict__ labels_out,
                                              int32_t *__restrict__ db_n_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
#if defined(MMW_STAMPS) && defined(MMW_STAMPS_POST)   // diagnostic build: start / end of every workgroup of this launch (scripts/wg_times_post.py)
    struct WgStamp {
        unsigned long long *w;
        __device__ WgStamp(const DevState &st) : w(nullptr) {
            if (threadIdx.x == 0 && blockIdx.x < 2048) {
                w = st.stats + kStatSlots * kStatWords + 256 + blockIdx.x * 4;
                w[0] = __builtin_amdgcn_s_memrealtime();
                w[1] = __builtin_amdgcn_s_memtime();
            }
        }
        __device__ ~WgStamp() { if (w) { w[2] = __builtin_amdgcn_s_memrealtime(); w[3] = __builtin_amdgcn_s_memtime(); } }
    } wg_stamp(st);
#endif
    // k_track has finished: no more pushes this step.  Block 0 says so before anything else, in EVERY step (side workers or not: the
    // stop epoch is what paces the side stream, k_chain claims only when it is exactly one step behind its own)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&st.q[kQStop], epoch);
    if ((int)blockIdx.x < G0) {
        __builtin_amdgcn_s_setprio(3);  // the latency chain goes first whenever it has an instruction ready
        // Side-stream workers (the large contexts): k_track is complete, so the queues' counts are final and their heads only grow --
        // one round trip tells a worker block that nothing is left to claim, and it is gone: its workgroup slot is one the Kalman
        // update behind it is waiting for (the four dependent atomics / loads of the queue protocol kept all 256 of them for 17 us).
        // Block 0 stays: it releases k_chain and holds the launch until every claimed cloud is finished.
        if (cfg.side_worker && blockIdx.x != 0) {
            // (k_chain moves the head WHILE this is read: one thread decides for the workgroup -- waves that read different
            //  heads would part ways in front of the worker loop's barriers)
            int *leave = reinterpret_cast<int *>(lds_raw);
            if (threadIdx.x == 0) {
                const int c3 = st.db_count[parity * 4 + 3], c0 = q_load(&st.q[parity * 8 + kQCount]), h0 = q_load(&st.q[parity * 8 + kQHead]) & kQIdxMask;
                const int cb = UMb > 0 ? q_load(&st.q[kQBig + parity * 8 + kQCount]) - (q_load(&st.q[kQBig + parity * 8 + kQHead]) & kQIdxMask) : 0;
                *leave = (c3 == 0 && h0 >= c0 && cb <= 0) ? 1 : 0;
            }
            __syncthreads();
            const int go = *leave;
            __syncthreads();  // (the word is the worker loop's LDS again from here)
            if (go) return;
        }
        // No side-stream workers this step (small contexts, the start-up frames, a profiler): what the work list and the two
        // queues hold now is all there is, and nobody else can have claimed any of it -- three counters in one round trip, and
        // a worker of a step without apply_DBscan (most steps) is gone; the atomics below are 4 dependent round trips more.
        if (!cfg.side_worker) {
            const int c3 = st.db_count[parity * 4 + 3], c0 = st.q[parity * 8 + kQCount], cb = st.q[kQBig + parity * 8 + kQCount];
            if ((c3 | c0 | cb) == 0) return;  // (uniform: the same words in every thread)
        }
        {   // list 3 (the clouds k_track did not queue early): a static share per block, as short as a pair count each
            DbLds L;
            db_lds_layout<true>(UMc, CL, true, lds_raw, &L);
            ScreenScratch *scr = reinterpret_cast<ScreenScratch *>(lds_raw + post_worker_plan(UMc, CL).tree_end);
            const int count = st.db_count[parity * 4 + 3];
            for (int w = blockIdx.x; w < count; w += G0) {
                const int s = st.db_list[(size_t)3 * cfg.n_scenes + w];
                SceneHdr *hdr = st.hdr + s;
                const int U = hdr->db_u;
                if (cfg.seek_inner && !hdr->need_db) continue;  // k_inner filled the track list: no apply_DBscan this frame (uniform)
                if (cloud_pairs_prove_no_core<NT>(cfg, ring_rows_of(cfg, st, hdr, s), U, scr->P4, scr->cnt, scr->mm, scr->flag))
                    cloud_finish_empty(st, hdr, s, U, UM_out, labels_out, db_n_out);
                else
                    spawn_scene<NT, true>(cfg, st, L, s, UMc, CL, UM_out, true, parity, labels_out, db_n_out);
                __syncthreads();  // LDS is reused by the next scene
            }
        }
        chain_worker_loop<NT>(cfg, st, lds_raw, UMc, CL, UM_out, parity, labels_out, db_n_out);
        if (UMb > 0 && st.q[kQBig + parity * 8 + kQCount] != 0) {  // small context: the large clouds here as well (k_track is complete: plain load)
            big_worker_loop<NT, false>(cfg, st, lds_raw, UMb, CLb, UM_out, parity, labels_out, db_n_out);
            if (blockIdx.x == 0 && threadIdx.x == 0) q_wait_done(st, st.q + kQBig + parity * 8);
        }
        // block 0 holds the launch until every claimed scene is finished (k_chain may still hold one)
        if (blockIdx.x == 0 && threadIdx.x == 0) q_wait_done(st, st.q + parity * 8);
        return;
    }
    if ((int)blockIdx.x == G0) {  // (not launched by the fused step: k_scene reads no schedule, every scene is resident)
        post_schedule_sort<NT>(cfg, st, parity, reinterpret_cast<int *>(lds_raw));
        return;
    }
    const int wave = threadIdx.x >> 6;
    const int unit = ((int)blockIdx.x - G0 - 1) * (NT / 64) + wave;
    if (unit >= cfg.n_scenes * nq) return;
    double *scratch = reinterpret_cast<double *>(lds_raw) + (size_t)wave * 4 * kUpdScratch;
    if (tracks_dense(cfg, nq)) {  // four real tracks per wave, from the lists k_track built this frame
        update_tracks_dense<DX>(cfg, st, unit, cfg.n_scenes * nq, parity, scratch);
        return;
    }
    const int us = unit / nq, q = unit - us * nq;
    const int s = st.perm[(size_t)parity * cfg.n_scenes + us];  // this step's schedule (the worker above writes the next one)
    update_tracks_wave<DX>(cfg, st, n_pts, s, q, nq, scratch);
}

// The chain workers of the side stream: 512-thread workgroups that serve BOTH queues while k_track and k_post run -- the
// large clouds first (the longer chains), then the small ones (pair-count screen, then the BallTree on the thread-per-point
// build).  One kernel, one stream: every further stream with a spinning kernel is one more hardware queue the context's
// stream must not share (see probe_side_streams in api_context.hip).
__global__ __launch_bounds__(kBigThreads) void k_chain(DevCfg cfg, DevState st, int UMc, int CL, int UM_out, int parity, int epoch,
                                               int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    DbLds L;
    ScreenScratch *scr = reinterpret_cast<ScreenScratch *>(lds_raw + big_worker_plan(UMc, CL, false).tree_end);  // (= chain_worker_plan's: the scratch takes the ticket's place)
    int *ticket = scr->ticket;  // [2]: scene, queue
    int32_t *qs = st.q + parity * 8, *qb = st.q + kQBig + parity * 8;
    int have = 0;  // queue of the item this workgroup is finishing (1 small, 2 large; uniform)
    for (;;) {
        __syncthreads();  // every thread is done with the previous cloud: its stores are issued, LDS is free again
        if (threadIdx.x == 0) {
            if (have) { __threadfence(); atomicAdd(&(have == 2 ? qb : qs)[kQDone], 1); }
            int s = -1, h = -1, kind = 0;
            for (int spins = 0; spins < kIdleLimit + cfg.n_scenes; spins++) {  // (k_track's first push comes later in a larger context)
                // Whose pushes are these?  The queues of a parity serve every second step and this launch knows only ITS step's
                // arguments (output buffers, big_live).  It is paced by the stop epochs alone (no event orders the two streams), and it
                // idles out after ~3 ms: with steps queued ahead of a stalled context stream (a long upload, a caller's kernel) the
                // launches of several steps can pass through here before the first k_track runs.  So: claim only while the step
                // before ours has reached its k_post (the counters of our parity were reset by its k_track, what is pushed now is
                // ours) and no later step has (ours is over: a launch that comes this late leaves).
                const int stop = q_load(&st.q[kQStop]);
#ifndef MMW_MUTANT_CHAIN_NOGATE   // (diagnostic build: tests/test_gpu_runahead.py must FAIL without the two lines below)
                if (stop - epoch >= 1) break;
                if (stop - (epoch - 1) < 0) { __builtin_amdgcn_s_sleep(8); continue; }
#endif
                // (a claim is a compare-and-swap on TAG + index: the head word was tagged with our step's number when the queue was reset
                //  for us; a worker that read `stop` above and was then held up for two steps fails here instead of taking a later
                //  step's cloud into ITS step's output buffers -- what the stop check alone let happen under six processes)
                const int hb = q_load(&qb[kQHead]), cb = cfg.big_live ? q_load(&qb[kQCount]) : 0;  // (start-up frames: pushed without a release, not ours)
                if ((hb & ~kQIdxMask) == q_tag(epoch) && (hb & kQIdxMask) < cb) {
                    if (atomicCAS(&qb[kQHead], hb, hb + 1) == hb) { h = hb & kQIdxMask; kind = 2; break; }
                    continue;
                }
                const int hs = q_load(&qs[kQHead]), cs = q_load(&qs[kQCount]);
                if ((hs & ~kQIdxMask) == q_tag(epoch) && (hs & kQIdxMask) < cs) {
                    if (atomicCAS(&qs[kQHead], hs, hs + 1) == hs) { h = hs & kQIdxMask; kind = 1; break; }
                    continue;
                }
                if (stop - epoch >= 0) break;  // k_post of this step had begun before the queues were looked at, and both are empty: done
                __builtin_amdgcn_s_sleep(8);
            }
            if (h >= 0) s = q_take_entry(st, kind == 2 ? qb : qs, st.db_list + (kind == 2 ? cfg.n_scenes : 0) + h);
            ticket[0] = s;
            ticket[1] = kind;
        }
        __syncthreads();
        const int s = ticket[0];  // (rewritten only behind the barrier at the top of the next round)
        if (s < 0) return;
        have = ticket[1];
        SceneHdr *hdr = st.hdr + s;
        const int U = hdr->db_u;
        if (have == 2) {
            const bool tpp = U <= kBigThreads;  // uniform
            db_lds_layout<true>(UMc, CL, tpp, lds_raw, &L);
            if (tpp) spawn_scene<kBigThreads, true>(cfg, st, L, s, UMc, CL, UM_out, false, parity, labels_out, db_n_out);
            else spawn_scene<kBigThreads, false>(cfg, st, L, s, UMc, CL, UM_out, false, parity, labels_out, db_n_out);
        } else {
            db_lds_layout<true>(UMc, CL, true, lds_raw, &L);
            if (cloud_pairs_prove_no_core<kBigThreads>(cfg, ring_rows_of(cfg, st, hdr, s), U, scr->P4, scr->cnt, scr->mm, scr->flag))
                cloud_finish_empty(st, hdr, s, U, UM_out, labels_out, db_n_out);
            else
                spawn_scene<kBigThreads, true>(cfg, st, L, s, UMc, CL, UM_out, true, parity, labels_out, db_n_out);
        }
    }
}

// k_dbscan_big / k_dbscan_startup: big_worker_loop over the whole queue, under two register budgets (launch_dbscan_big) -- two entry
// points with their own launch bounds, the three lines written out in each (behind one shared inlined body the compiler scheduled
// k_dbscan_big differently: profiles/dbscan_workers_attempts.txt)
__global__ __launch_bounds__(kBigThreads) void k_dbscan_big(DevCfg cfg, DevState st, int UMc, int CL, int UM_out, int parity,
                                                    int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    // (k_track is complete: the count is final and a plain load.  No large cloud this step -- nearly every step of a
    // tracked scene set -- and the whole launch leaves on that one word)
    if (st.q[kQBig + parity * 8 + kQCount] == 0) return;
    big_worker_loop<kBigThreads, false>(cfg, st, lds_raw, UMc, CL, UM_out, parity, labels_out, db_n_out);
    if (blockIdx.x == 0 && threadIdx.x == 0) q_wait_done(st, st.q + kQBig + parity * 8);
}

__global__ __launch_bounds__(kBigThreads, 4) void k_dbscan_startup(DevCfg cfg, DevState st, int UMc, int CL, int UM_out, int parity,
                                                                   int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    if (st.q[kQBig + parity * 8 + kQCount] == 0) return;
    big_worker_loop<kBigThreads, true>(cfg, st, lds_raw, UMc, CL, UM_out, parity, labels_out, db_n_out);
    if (blockIdx.x == 0 && threadIdx.x == 0) q_wait_done(st, st.q + kQBig + parity * 8);
}

// ---- Clouds of more than 1920 points (a context with ring * max_pts up to 4096: apply_DBscan itself has no limit,
//      Utils.py:250-291) ----------------------------------------------------------------------------------------------------
// 64 .. 128 leaves: the carve-up (up to ~0.5 MB) does not fit the LDS and lives in GLOBAL memory instead, one slab per worker
// (DevState::huge_scratch) -- the same dbscan_core / add_clusters, instantiated over pointers into that slab: the address
// space is the only difference (workgroup barriers order global memory inside a workgroup as they order the LDS: its waves
// share the CU's L1, stores write through), and the leaf-state mask of a position is MW = 4 words instead of one.  A chain
// of L2 round trips instead of LDS ones, several times slower per cloud: this is the path that makes such a context POSSIBLE
// (a scene that lost its tracks clusters its whole ring), not one the step is tuned around.  k_track puts these scenes on
// work list 2; one launch behind k_dbscan_big, only in contexts whose rings can hold such a cloud.
__global__ __launch_bounds__(kHugeThreads) void k_dbscan_huge(DevCfg cfg, DevState st, int UMc, int CL, int UM_out, int parity,
                                                              int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    DbLds L;
    db_hybrid_layout<true>(UMc, CL, lds_raw, st.huge_scratch + (size_t)blockIdx.x * st.huge_stride, &L, kHugeMW, nullptr);
    const int count = st.db_count[parity * 4 + 2];
    for (int w = blockIdx.x; w < count; w += gridDim.x) {
        const int s = st.db_list[(size_t)2 * cfg.n_scenes + w];
        if (cfg.seek_inner && !st.hdr[s].need_db) continue;  // cancelled by k_inner (uniform)
        spawn_scene<kHugeThreads, false, kHugeMW>(cfg, st, L, s, UMc, CL, UM_out, false, parity, labels_out, db_n_out);
        __syncthreads();  // the slab is reused by the next scene
    }
}

// ClusterTrack.seek_inner_clusters (Tracking.py:409-448) with its call site (Tracking.py:656) active, cfg.seek_inner:
// one launch between k_track and k_post, one workgroup per scene.  For every track whose associate_pointcloud ran
// this frame (k_track marks them), in list order:
//   * `cluster.point_num > DB_POINTS_THRES and spread.any() > DB_SPREAD_THRES` -- the second term compares a BOOL
//     (x-spread != 0) with the threshold, as the reference does;
//   * change_buffer_size(FB_FRAMES_BATCH_STATIC | FB_FRAMES_BATCH) -- permanent -- and add_frame(cluster.pointcloud): the
//     cloud k_track has just appended is appended a second time;
//   * apply_DBscan(effective_data, eps = DB_INNER_EPS) with the default min_samples; more than one cluster ->
//     _add_tracks([clusters[1]]) (Tracking.py:658-660): the track is appended BEFORE _update_all (k_post) and before
//     the frame's own DBSCAN trigger, which is re-evaluated here (`len(effective_tracks) < TR_MAX_TRACKS`).
// The per-scene layout of the Kalman kernels is forced for such contexts (hdr->n_upd is all k_post needs).
constexpr int kInnerThreads = 512;
__global__ __launch_bounds__(kInnerThreads) void k_inner(DevCfg cfg, DevState st, const int32_t *__restrict__ n_pts, int UMc,
                                                         int32_t *__restrict__ db_n_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int n = n_pts[s];
    int32_t *ib = st.inner_buf + (size_t)s * (kInnerHdr + st.inner_cap);
    if (tid < kInnerHdr) ib[tid] = 0;
    if (!frame_reaches_track(n, cfg.max_pts)) return;  // the frame never reached track()
    SceneHdr *hdr = st.hdr + s;
    int32_t *order = st.order + (size_t)s * cfg.t_cap;
    TrackRec *trk = st.trk + (size_t)s * cfg.t_cap;
    const int Tin = hdr->n_tracks;  // after _maintain_tracks: tracks with points are never removed and keep their order
    int T = Tin, calls = 0, stored = 0, err = 0;
    DbLds L;
    __syncthreads();
    for (int j = 0; j < Tin; j++) {
        const int slot = order[j];
        TrackRec *rec = trk + slot;
        const int inner = rec->inner;
        if (!(inner & kInnerTouched)) continue;  // uniform
        const double xspread = rec->maxv[0] - rec->minv[0];
        const double any = xspread != 0.0 ? 1.0 : 0.0;
        const bool go = rec->point_num > cfg.db_points_thres && any > cfg.db_spread_thres;
        int len = rec->ring_len, rn[MMW_RING_MAX], rs[MMW_RING_MAX];
#pragma unroll
        for (int k = 0; k < MMW_RING_MAX; k++) { rn[k] = rec->ring_n[k]; rs[k] = rec->ring_slot[k]; }
        const bool is_static = rec->is_static != 0;
        __syncthreads();  // everyone has read the record
        if (!go) {
            if (tid == 0) rec->inner = inner & 255;
            continue;
        }
        // ---- change_buffer_size + add_frame(cluster.pointcloud) ----
        const int size = is_static ? cfg.fb_frames_batch_static : cfg.ring - 1;  // FB_FRAMES_BATCH_STATIC | FB_FRAMES_BATCH
        const int src_slot = rs[len - 1], rows = rn[len - 1];  // the cloud associate_pointcloud appended
        while (len >= size && len > 0) {
            const int first = rs[0];
#pragma unroll
            for (int k = 1; k < MMW_RING_MAX; k++) if (k < len) { rs[k - 1] = rs[k]; rn[k - 1] = rn[k]; }
#pragma unroll
            for (int k = 0; k < MMW_RING_MAX; k++) if (k == len - 1) rs[k] = first;
            len--;
        }
        int dst_slot = rs[0];
#pragma unroll
        for (int k = 1; k < MMW_RING_MAX; k++) if (k == len) dst_slot = rs[k];
#pragma unroll
        for (int k = 0; k < MMW_RING_MAX; k++) if (k == len) rn[k] = rows;
        len++;
        double *ring = st.trk_ring + ((size_t)s * cfg.t_cap + slot) * cfg.ring * (size_t)cfg.ring_rows * 8;
        const int keep = min(rows, cfg.ring_rows);
        if (dst_slot != src_slot) {
            const double2 *a = reinterpret_cast<const double2 *>(ring + (size_t)src_slot * cfg.ring_rows * 8);
            double2 *b = reinterpret_cast<double2 *>(ring + (size_t)dst_slot * cfg.ring_rows * 8);
            for (int e = tid; e < keep * 4; e += kInnerThreads) b[e] = a[e];
        }
        if (tid == 0) {
            rec->ring_len = len;
#pragma unroll
            for (int k = 0; k < MMW_RING_MAX; k++) { rec->ring_n[k] = k < len ? rn[k] : 0; rec->ring_slot[k] = rs[k]; }
            rec->inner = size;
        }
        // ---- apply_DBscan(self.batch.effective_data, eps=DB_INNER_EPS) ----
        RowSrc src;
        const int big = 0x7fffffff;
        src.gb = ring;
        src.stride = (size_t)cfg.ring_rows * 8;
        src.slots = (unsigned)rs[0] | ((unsigned)rs[1] << 8) | ((unsigned)rs[2] << 16) | ((unsigned)rs[3] << 24);
        src.c1 = len > 1 ? rn[0] : big;
        src.c2 = len > 2 ? rn[0] + rn[1] : big;
        src.c3 = len > 3 ? rn[0] + rn[1] + rn[2] : big;
        int U = 0;
#pragma unroll
        for (int k = 0; k < MMW_RING_MAX; k++) if (k < len) U += rn[k];
        bool whole = true;
#pragma unroll
        for (int k = 0; k < MMW_RING_MAX; k++) if (k < len && rn[k] > cfg.ring_rows) whole = false;
        if (U > UMc || !whole) { err |= ERR_CAPACITY; continue; }  // a frame that was not stored whole, or more points than the BallTree holds
        __syncthreads();  // the copied rows are visible to the whole workgroup (this barrier is also a global-memory fence)
        {   // sklearn's input validation in front of the inner apply_DBscan (Utils.py:272-278): all 8 columns of the track's
            // ring rows -- an assigned point can carry a NaN / infinite doppler or peakVal (the gate only sees columns 0..5).
            // The reference's ValueError leaves track() in the middle of _associate_points_to_tracks: the scene is flagged,
            // this track's inner clustering does not run.
            const int nfb = cloud_nonfinite_bits(src, U);
            if (nfb) { err |= nf_error_of(nfb); continue; }
        }
        const bool tpp = U <= kInnerThreads;  // uniform
        db_lds_layout<true>(UMc, 2, tpp, lds_raw, &L);
        const int ncl = tpp ? dbscan_core<kInnerThreads, true>(cfg, L, src, U, UMc, cfg.db_inner_eps, cfg.db_min_samples, nullptr)
                            : dbscan_core<kInnerThreads, false>(cfg, L, src, U, UMc, cfg.db_inner_eps, cfg.db_min_samples, nullptr);
        // the call, for mmw_get_inner: rows and labels in call order
        if (calls < 16 && tid == 0) ib[2 + calls] = U;
        if (stored + U <= st.inner_cap) {
            for (int i = tid; i < U; i += kInnerThreads) ib[kInnerHdr + stored + i] = L.idx2[i];
            stored += U;
        }
        calls++;
        if (ncl > 1) {  // new_track_clusters = [track_clusters[1]]
            if (T + 1 > cfg.t_cap) { err |= ERR_CAPACITY; }
            else {
                __syncthreads();
                if (tid == 0) { L.misc[4] = hdr->next_uid; hdr->next_uid += 1; }
                __syncthreads();
                add_clusters<kInnerThreads>(cfg, st, L, src, s, U, 2, 1, 1, T);
                T++;
            }
        }
        __syncthreads();  // LDS and the scene's records are reused by the next track
    }
    if (tid == 0) {
        ib[0] = calls;
        ib[1] = stored;
        const int nd = hdr->need_db;
        if (T != Tin) {
            hdr->n_tracks = T;
            hdr->n_upd = T;   // _update_all covers the inner tracks as well
            if (T >= cfg.tr_max_tracks) {  // Tracking.py:693-697: apply_DBscan is not called this frame after all
                hdr->need_db = 0;
                if (db_n_out) db_n_out[s] = -1;
            }
        }
        if (nd & 2) {   // k_track left the verdict on a ring that holds a non-finite row to this re-evaluated trigger
            if (T < cfg.tr_max_tracks) {
                err |= nd >> 2;
                if (db_n_out) db_n_out[s] = kDbRaised;
            }
            hdr->need_db = 0;
        }
        if (err) atomicOr(&hdr->err, err);
    }
}

// Utils.apply_DBscan on caller-provided clouds: pts[S][max_n][8]
__global__ __launch_bounds__(256) void k_dbscan_only(DevCfg cfg, int UM, const double *__restrict__ pts,
                                                    const int32_t *__restrict__ n_all, int max_n, double eps,
                                                    int min_samples, int32_t *__restrict__ labels_out,
                                                    int32_t *__restrict__ ncl_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    DbLds L;
    db_lds_layout<true>(UM, 0, false, lds_raw, &L);
    const int s = blockIdx.x, tid = threadIdx.x;
    const int U = n_all[s];
    if (U <= 0 || U > UM) { if (tid == 0 && ncl_out) ncl_out[s] = 0; return; }
    RowSrc src;
    src.gb = pts + (size_t)s * max_n * 8;
    src.stride = 0;
    src.slots = 0;
    src.c1 = src.c2 = src.c3 = 0x7fffffff;
    if (const int nfb = cloud_nonfinite_bits(src, U)) {   // sklearn raises ValueError: no labels, n_clusters = -(error bit)
        if (tid == 0 && ncl_out) ncl_out[s] = -nf_error_of(nfb);
        return;
    }
    const int ncl = dbscan_core<256, false>(cfg, L, src, U, UM, eps, min_samples, nullptr);
    for (int i = tid; i < U; i += 256) labels_out[(size_t)s * max_n + i] = L.idx2[i];
    if (tid == 0 && ncl_out) ncl_out[s] = ncl;
}

// Utils.apply_DBscan on caller-provided clouds of more than 1920 points (mmw_dbscan): as k_dbscan_only, slab per workgroup
__global__ __launch_bounds__(kHugeThreads) void k_dbscan_only_huge(DevCfg cfg, DevState st, int UM, int n_clouds, const double *__restrict__ pts,
                                                                   const int32_t *__restrict__ n_all, int max_n, double eps, int min_samples,
                                                                   int32_t *__restrict__ labels_out, int32_t *__restrict__ ncl_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    DbLds L;
    db_hybrid_layout<true>(UM, 0, lds_raw, st.huge_scratch + (size_t)blockIdx.x * st.huge_stride, &L, kHugeMW, nullptr);
    const int tid = threadIdx.x;
    for (int s = blockIdx.x; s < n_clouds; s += gridDim.x) {
        const int U = n_all[s];
        if (U <= 0 || U > UM) { if (tid == 0 && ncl_out) ncl_out[s] = 0; continue; }
        RowSrc src;
        src.gb = pts + (size_t)s * max_n * 8;
        src.stride = 0;
        src.slots = 0;
        src.c1 = src.c2 = src.c3 = 0x7fffffff;
        if (const int nfb = cloud_nonfinite_bits(src, U)) {   // sklearn raises ValueError: no labels, n_clusters = -(error bit)
            if (tid == 0 && ncl_out) ncl_out[s] = -nf_error_of(nfb);
            continue;
        }
        const int ncl = dbscan_core<kHugeThreads, false, kHugeMW>(cfg, L, src, U, UM, eps, min_samples, nullptr);
        for (int i = tid; i < U; i += kHugeThreads) labels_out[(size_t)s * max_n + i] = L.idx2[i];
        if (tid == 0 && ncl_out) ncl_out[s] = ncl;
        __syncthreads();
    }
}

// ---- host side ---------------------------------------------------------------------------
static const int kClassUM[3] = {256, 768, 1920};

int dbscan_class_um(int cls, int UM) { return kClassUM[cls] < UM ? kClassUM[cls] : UM; }
size_t dbscan_lds_bytes(int cls, int UM, int t_cap, int min_samples)
{
    const int um = dbscan_class_um(cls, UM);
    return db_tree_end(um, db_class_cl(um, t_cap, min_samples), cls != 0);  // (k_dbscan_big carves either way per cloud)
}

static size_t post_lds_bytes(int UM, int t_cap, int min_samples, int waves = 4)
{
    const size_t upd = (size_t)waves * 4 * kUpdScratch * sizeof(double);
    const int um = dbscan_class_um(0, UM);
    const size_t db = post_worker_plan(um, db_class_cl(um, t_cap, min_samples)).bytes;
    return upd > db ? upd : db;
}

// capacity of the large-cloud kernels this step: no cloud has more than `u_bound` points (the caller knows how many frames the
// rings can hold so soon after a reset), none more than UM, and the BallTree emulation holds 1920
static int big_um(int UM, int u_bound)
{
    int um = u_bound < UM ? u_bound : UM;
    return um < kClassUM[2] ? um : kClassUM[2];
}
static size_t big_lds_bytes(int um, int cl, bool tpp_only) { return big_worker_plan(um, cl, tpp_only).bytes; }
// k_chain: the capacity of the large clouds (at least one slot per thread), + the pair-count scratch and the ticket
static int chain_um(int UM, int u_bound)
{
    const int um = big_um(UM, u_bound);
    return um < kBigThreads ? kBigThreads : um;
}
static size_t chain_lds_bytes(int um, int t_cap, int min_samples) { return chain_worker_plan(um, db_class_cl(um, t_cap, min_samples)).bytes; }

size_t dbscan_only_lds_bytes(int UM) { return only_plan(UM < kClassUM[2] ? UM : kClassUM[2]).bytes; }

hipError_t prepare_dbscan(int UM, int t_cap, int min_samples)
{
    const int bum = big_um(UM, UM);
    const size_t big = big_lds_bytes(bum, db_class_cl(bum, t_cap, min_samples), false);
    const size_t post = post_lds_bytes(UM, t_cap, min_samples) > big ? post_lds_bytes(UM, t_cap, min_samples) : big;  // (small contexts: the large clouds in k_post)
    const size_t c5 = chain_lds_bytes(kBigThreads, t_cap, min_samples), post512 = (c5 > big ? c5 : big) > post ? (c5 > big ? c5 : big) : post;   // (behind the fused step: 512-thread worker blocks)
    hipError_t e = set_dynamic_lds({{(const void *)k_post<9, 256>, post},
                                    {(const void *)k_post<6, 256>, post},
                                    {(const void *)k_post<9, 512>, post512},
                                    {(const void *)k_post<6, 512>, post512},
                                    {(const void *)k_dbscan_big, big},
                                    {(const void *)k_chain, chain_lds_bytes(chain_um(UM, UM), t_cap, min_samples)},
                                    {(const void *)k_dbscan_startup, big}});
    if (e != hipSuccess) return e;
    if (UM > kClassUM[2]) {   // the clouds of more than 1920 points: hot arrays in the LDS, the rest on slabs in global memory
        const size_t hot = huge_lds_bytes(UM, db_class_cl(UM, t_cap, min_samples));
        e = set_dynamic_lds({{(const void *)k_dbscan_huge, hot}, {(const void *)k_dbscan_only_huge, hot}});
        if (e != hipSuccess) return e;
    }
    return set_dynamic_lds({{(const void *)k_dbscan_only, dbscan_only_lds_bytes(UM)}});
}

int inner_um(const DevCfg &cfg)
{
    long long v = (long long)cfg.ring * cfg.ring_rows;
    if (v < 512) v = 512;  // (capacity only: the 512-thread build wants one exchange slot per thread)
    return (int)(v < 30 * 64 ? v : 30 * 64);  // the BallTree emulation holds <= 32 leaves
}
static size_t inner_lds_bytes(const DevCfg &cfg) { return inner_plan(inner_um(cfg)).bytes; }
hipError_t prepare_inner(const DevCfg &cfg)
{
    return hipFuncSetAttribute((const void *)k_inner, hipFuncAttributeMaxDynamicSharedMemorySize, (int)inner_lds_bytes(cfg));
}
size_t inner_lds_demand(const DevCfg &cfg) { return inner_lds_bytes(cfg); }
void launch_inner(const DevCfg &cfg, const DevState &st, const int32_t *n_pts, int32_t *db_n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_inner, dim3(cfg.n_scenes), dim3(kInnerThreads), inner_lds_bytes(cfg), stream, cfg, st, n_pts, inner_um(cfg), db_n);
}

// _update_all + the BallTree DBSCAN of the small clouds (work list 3)
void launch_post(const DevCfg &cfg, const DevState &st, const int32_t *n_pts, int UM, int u_bound, int parity, int epoch, int32_t *labels,
                 int32_t *db_n, hipStream_t stream)
{
    const int nq = kalman_waves_per_scene(cfg.tr_max_tracks);
    const int S = cfg.n_scenes, units = cfg.fused ? 0 : S * nq;  // (fused step: _update_all ran inside k_scene, only the DBSCAN workers are left)
    int G0 = S < 256 ? S : 256;
    const int umc = dbscan_class_um(0, UM), cl = db_class_cl(umc, cfg.t_cap, cfg.db_min_samples);
    size_t lds = post_lds_bytes(UM, cfg.t_cap, cfg.db_min_samples);
    // a small context's step is launch latency: its large clouds are taken here too and k_dbscan_big is not launched
    int umb = 0, clb = 0;
    if (S <= kSmallContextScenes && big_um(UM, u_bound) > kClassUM[0]) {
        umb = big_um(UM, u_bound);
        clb = db_class_cl(umb, cfg.t_cap, cfg.db_min_samples);
        const size_t big = big_lds_bytes(umb, clb, false);
        if (big > lds) lds = big;
        // (with that much LDS a CU holds one workgroup: workers + update units must stay one wave of workgroups)
        constexpr int kSmallContextWorkers = 64;  // (32 .. 128 measured equal)
        if (G0 > kSmallContextWorkers) G0 = kSmallContextWorkers;
    }
    if (units == 0) {
        // Behind the fused step only the DBSCAN workers are left: 512-THREAD blocks, as k_chain's -- a BallTree chain is ~40 us on
        // 512 threads against 45-60 on 256 (queries and the register sort network split two ways), and with the update gone nothing
        // in the launch wants two blocks per CU.  (For the contexts whose update runs here the same was measured and lost:
        // eight update waves that start and end together, profiles/NOTEBOOK.md round 5.)
        // (the 512-thread build wants one exchange slot per thread: the small clouds' carve-up holds at least 512 points, as k_chain's)
        const int umc5 = umc < kBigThreads ? kBigThreads : umc, cl5 = db_class_cl(umc5, cfg.t_cap, cfg.db_min_samples);
        const size_t c5 = chain_lds_bytes(umc5, cfg.t_cap, cfg.db_min_samples);
        if (c5 > lds) lds = c5;
        if (umb > 0 && umb < kBigThreads) {   // ... and so does the large clouds' (a context whose rings hold 257 .. 511 points)
            umb = kBigThreads;
            clb = db_class_cl(umb, cfg.t_cap, cfg.db_min_samples);
            const size_t b5 = big_lds_bytes(umb, clb, false);
            if (b5 > lds) lds = b5;
        }
        with_dx(cfg.dx, [&](auto DX) {
            mmw_launch(k_post<decltype(DX)::value, 512>, dim3(G0), dim3(512), lds, stream, cfg, st, n_pts, nq, G0, umc5, cl5, umb, clb, UM, parity, epoch, labels, db_n);
        });
        return;
    }
    const int upd_blocks = (units + 3) / 4;
    const dim3 grid(G0 + 1 + upd_blocks);  // workers | the schedule sort | _update_all
    with_dx(cfg.dx, [&](auto DX) {
        mmw_launch(k_post<decltype(DX)::value, 256>, grid, dim3(256), lds, stream, cfg, st, n_pts, nq, G0, umc, cl, umb, clb, UM, parity, epoch, labels, db_n);
    });
}

// The chain workers beside k_track and k_post (a second stream; see k_chain)
void launch_chain(const DevCfg &cfg, const DevState &st, int UM, int u_bound, int parity, int epoch, int32_t *labels, int32_t *db_n, hipStream_t side)
{
    // (2 / 4 / 8 / 12 / 16 workgroups, now that the pair counts run in k_track and only BallTree chains arrive: 0.2025 / 0.195 / 0.190 /
    //  0.189 / 0.190 ms per step in a 100-step window, 0.210 / 0.203 / 0.194 / 0.192 / 0.192 in a 150-step one: profiles/NOTEBOOK.md)
#ifdef MMW_STAMPS
    static const int want = getenv("MMW_CHAIN_BLOCKS") ? atoi(getenv("MMW_CHAIN_BLOCKS")) : kChainBlocks;  // diagnostic build only
#else
    const int want = kChainBlocks;
#endif
    const int um = chain_um(UM, u_bound), cl = db_class_cl(um, cfg.t_cap, cfg.db_min_samples);
    const int g = want < cfg.n_scenes ? want : cfg.n_scenes;
    hipLaunchKernelGGL(k_chain, dim3(g > 0 ? g : 1), dim3(kBigThreads), chain_lds_bytes(um, cfg.t_cap, cfg.db_min_samples), side, cfg, st, um, cl, UM,
                       parity, epoch, labels, db_n);
}

// The larger clouds, what the side-stream workers have not taken: k_dbscan_big (k_dbscan_startup in the first frames
// after a reset: 512-point clouds at most, two workgroups per CU -- 3.0 instead of 4.0 ms for frame 0 of 4096 scenes).
void launch_dbscan_big(const DevCfg &cfg, const DevState &st, int UM, int u_bound, int parity, int32_t *labels, int32_t *db_n, hipStream_t stream)
{
    const int um = big_um(UM, u_bound);
    if (kClassUM[0] >= um) return;  // no cloud can exceed the small class
    if (cfg.n_scenes <= kSmallContextScenes) return;  // k_post has taken them (launch_post)
    const int S = cfg.n_scenes, cl = db_class_cl(um, cfg.t_cap, cfg.db_min_samples);
    if (um <= kBigThreads && um < UM) {
        const size_t lds = big_lds_bytes(um, cl, true);
        int g = 256 * ((160u * 1024u) / lds >= 2 ? 2 : 1);
        if (g > S) g = S;
        mmw_launch(k_dbscan_startup, dim3(g), dim3(kBigThreads), lds, stream, cfg, st, um, cl, UM, parity, labels, db_n);
        return;
    }
    const int g = S < 256 ? S : 256;  // 176 VGPRs: one 512-thread workgroup per CU
    mmw_launch(k_dbscan_big, dim3(g), dim3(kBigThreads), big_lds_bytes(um, cl, false), stream, cfg, st, um, cl, UM, parity, labels, db_n);
}

void launch_dbscan_only(const DevCfg &cfg, const DevState &st, int UM, const double *pts, const int32_t *n, int max_n, double eps, int min_samples,
                        int32_t *labels, int32_t *ncl, hipStream_t stream)
{
    if (max_n > kClassUM[2]) {  // clouds the LDS cannot hold: slabs in global memory
        const int g = cfg.n_scenes < kHugeWorkers ? cfg.n_scenes : kHugeWorkers;
        hipLaunchKernelGGL(k_dbscan_only_huge, dim3(g), dim3(kHugeThreads), huge_lds_bytes(UM, 0), stream, cfg, st, UM, cfg.n_scenes, pts, n, max_n,
                           eps, min_samples, labels, ncl);
        return;
    }
    const int umk = UM < kClassUM[2] ? UM : kClassUM[2];  // (a context whose rings hold more: the LDS classes stop at 1920)
    hipLaunchKernelGGL(k_dbscan_only, dim3(cfg.n_scenes), dim3(256), dbscan_only_lds_bytes(umk), stream, cfg, umk, pts, n, max_n, eps, min_samples,
                       labels, ncl);
}

// the clouds of more than 1920 points (work list 2): contexts whose rings can hold one
int dbscan_huge_workers(int n_scenes) { return n_scenes < kHugeWorkers ? n_scenes : kHugeWorkers; }
size_t dbscan_huge_slab_bytes(int UM, int t_cap, int min_samples)
{
    if (UM <= kClassUM[2]) return 0;
    const size_t a = db_hybrid_layout<false>(UM, db_class_cl(UM, t_cap, min_samples), nullptr, nullptr, nullptr, kHugeMW, nullptr);
    return (a + 255) & ~(size_t)255;
}
void launch_dbscan_huge(const DevCfg &cfg, const DevState &st, int UM, int u_bound, int parity, int32_t *labels, int32_t *db_n, hipStream_t stream)
{
    if (UM <= kClassUM[2] || u_bound <= kClassUM[2]) return;  // no ring of this context can hold such a cloud (yet)
    const int cl = db_class_cl(UM, cfg.t_cap, cfg.db_min_samples);
    mmw_launch(k_dbscan_huge, dim3(dbscan_huge_workers(cfg.n_scenes)), dim3(kHugeThreads), huge_lds_bytes(UM, cl), stream, cfg, st, UM, cl, UM, parity,
               labels, db_n);
}

}  // namespace mmw
