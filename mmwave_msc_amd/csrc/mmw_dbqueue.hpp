// mmw_dbqueue.hpp -- how the DBSCAN workers get their clouds (the two queues k_track fills while it runs) and where each kind
// of worker keeps what in its dynamic LDS: one definition of either, shared by the kernels and their launchers
// (k_dbscan.hip).
#pragma once
#include "mmw_balltree.hpp"

namespace mmw {

// The two queues k_track fills WHILE IT RUNS (q[8p + ...] over list 0: the clouds of <= 256 points that can hold a
// cluster; q[kQBig + 8p + ...] over list 1: the clouds of more than 256 points) and their consumers.  An item is
// apply_DBscan + _add_tracks of one scene: 40-90 us of BallTree chain for a small cloud (after the exact pair count of the
// screen), 100-250 us for a large one.  The workgroups of k_chain take them on a second stream BESIDE k_track and k_post, so
// a chain sits in the shadow of the bulk kernels instead of behind them; the worker blocks of k_post (small) and
// k_dbscan_big (large) follow on the context's stream, take whatever is left and wait for the claimed items to finish --
// correctness never depends on k_chain having run.  `epoch` = this step's number: k_post raises q[kQStop] to it when it
// starts, i.e. when no more pushes can come.  Every wait is bounded.
#ifndef MMW_CHAIN_BLOCKS   // (scripts/chain_blocks.sh: diagnostic builds with another count)
#define MMW_CHAIN_BLOCKS 12
#endif
constexpr int kChainBlocks = MMW_CHAIN_BLOCKS;
// Waits that MUST succeed (an entry behind its count: a few instructions in the pushing workgroup; the end of a claimed item: one
// BallTree chain) are bounded by TIME, not by iterations -- the 100 MHz s_memrealtime counter; a slow clock or a profiler that
// serialises kernels must not turn into a spurious give-up: 0.2 s for an entry, 2 s for the end of the claimed items
constexpr unsigned long long kMustWaitTicks = 20000000ULL, kDoneWaitTicks = 200000000ULL;
// ... and how long a side-stream worker polls EMPTY queues before it leaves (~3 ms; k_post / k_dbscan_big take whatever comes
// later).  Short on purpose: should the context's stream ever sit behind a polling worker in one hardware queue -- two
// contexts whose streams share queues crosswise can do that, the probe only sees its own pair -- the damage is these 3 ms.
constexpr int kIdleLimit = 1 << 12;
// Polls are RELAXED device-scope atomic loads (served by the L2, no side effects): an ACQUIRE load invalidates the caches of
// the polling CU -- and the non-coherent lines of its XCD's L2 -- every time, and 64 pollers doing that made k_track, which
// runs beside them, 50 % slower.  One acquire fence follows a successful claim instead.
__device__ __forceinline__ int q_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void q_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }

// ---- the queue protocol: q = the three words of one queue of one parity (st.q + 8p for the small clouds over list 0,
//      st.q + kQBig + 8p for the large ones over list 1); one thread of the workgroup runs it ----------------------------------

// A ticket by atomicAdd, for the workers behind k_track (the step's pushes are complete): the ring index, or -1 -- a ticket
// past the count ends the block, and the counters are reset before their parity is used again.
__device__ __forceinline__ int q_claim_ticket(int32_t *q)
{
    const int h = atomicAdd(&q[kQHead], 1) & kQIdxMask;   // (tickets; the tag of the step in the upper bits: mmw_device.hpp)
    return h < q_load(&q[kQCount]) ? h : -1;
}

// (k_chain, beside k_track, claims by compare-and-swap on tag + index instead -- only when an entry is there, so a worker that gives
//  up never holds a ticket; that claim is written out in its loop: k_dbscan.hip.)

// The claimed ring entry -> its scene.  The entry follows its count by a few instructions in the pushing workgroup: a bounded
// wait; then -1, a sticky error (mmw_check) and the item counted as done so that nobody waits for it.
__device__ __forceinline__ int q_take_entry(const DevState &st, int32_t *q, int32_t *e)
{
    int v = 0;
    for (const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(); (v = q_load(e)) == 0 && __builtin_amdgcn_s_memrealtime() - t0 < kMustWaitTicks;) __builtin_amdgcn_s_sleep(2);
    if (v == 0) { atomicAdd(&st.q[kQTimeout], 1); atomicAdd(&q[kQDone], 1); return -1; }
    __hip_atomic_store(e, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    q_acquire();  // what the pushing workgroup stored for the scene is visible from here on
    return v - 1;
}

// The launch must not end before every claimed item is finished (a side-stream worker may still hold one): the next
// launches read what the spawn writes.  Bounded: ~2 s, then a sticky error.
__device__ __forceinline__ void q_wait_done(const DevState &st, const int32_t *q)
{
    const int want = q_load(&q[kQCount]);
    for (const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(); q_load(&q[kQDone]) < want && __builtin_amdgcn_s_memrealtime() - t0 < kDoneWaitTicks;) __builtin_amdgcn_s_sleep(8);
    if (q_load(&q[kQDone]) < want) atomicAdd(&st.q[kQTimeout], 1);
    q_acquire();
}

// ---- the workers' dynamic LDS: the BallTree carve-up (mmw_balltree.hpp) at offset 0, then what the worker itself needs.  Each
//      kind of worker has ONE plan: the kernel takes its offsets from it, the launcher its byte count --------------------------

// Scratch of the pair-count screen (cloud_pairs_prove_no_core, mmw_cloud.hpp) and the word(s) a worker loop hands its claim to the
// workgroup in.  (k_track and k_scene keep their own copy of the first four inside their work areas.)
struct ScreenScratch {
    float4 P4[256];
    int cnt[256];
    int flag[2];
    unsigned long long mm[3];
    int ticket[2];   // scene (, queue: k_chain)
    int spare[18];
};
static_assert(offsetof(ScreenScratch, P4) == 0 && offsetof(ScreenScratch, cnt) == 4096 && offsetof(ScreenScratch, flag) == 5120 &&
              offsetof(ScreenScratch, mm) == 5128 && offsetof(ScreenScratch, ticket) == 5152 && sizeof(ScreenScratch) == 5232,
              "the screen scratch: the offsets every worker has used, 5232 bytes reserved behind the carve-up");
constexpr size_t kTicketBytes = 16;   // a worker loop without the screen: its ticket word alone

// Where the tree's carve-up ends when a worker carves per cloud, thread-per-point or (strided_too) either way: the larger of the two
__host__ __device__ __forceinline__ size_t db_tree_end(int UM, int CL, bool strided_too)
{
    const size_t tpp = db_lds_layout<false>(UM, CL, true, nullptr, nullptr), strided = strided_too ? db_lds_layout<false>(UM, CL, false, nullptr, nullptr) : 0;
    return tpp > strided ? tpp : strided;
}
struct LdsPlan {
    size_t tree_end;   // ScreenScratch / the ticket word sit here
    size_t bytes;      // dynamic LDS of the launch
};
// k_post's worker blocks over the small clouds (chain_worker_loop, list 3): thread-per-point build, screen scratch
__host__ __device__ __forceinline__ LdsPlan post_worker_plan(int UMc, int CL)
{
    const size_t end = db_align16(db_tree_end(UMc, CL, false));
    return {end, end + sizeof(ScreenScratch)};
}
// the workers over the large clouds (big_worker_loop: k_dbscan_big, k_post in small contexts; tpp_only: k_dbscan_startup): ticket word
__host__ __device__ __forceinline__ LdsPlan big_worker_plan(int UMc, int CL, bool tpp_only)
{
    const size_t end = db_align16(db_tree_end(UMc, CL, !tpp_only));
    return {end, end + kTicketBytes};
}
// k_chain, and k_post's 512-thread worker blocks behind the fused step: both queues -- the large clouds' plan (its ticket word stays
// reserved), the screen scratch in place of the ticket
__host__ __device__ __forceinline__ LdsPlan chain_worker_plan(int UMc, int CL)
{
    const LdsPlan big = big_worker_plan(UMc, CL, false);
    return {big.tree_end, big.bytes + sizeof(ScreenScratch)};
}
// k_inner: the tree alone, either build per track
__host__ __device__ __forceinline__ LdsPlan inner_plan(int UMc) { const size_t end = db_tree_end(UMc, 2, true); return {end, end}; }
// k_dbscan_only: the tree alone, strided build, no spawn
__host__ __device__ __forceinline__ LdsPlan only_plan(int UMc) { const size_t end = db_lds_layout<false>(UMc, 0, false, nullptr, nullptr); return {end, end}; }
// k_dbscan_huge / k_dbscan_only_huge: the hot arrays of the hybrid carve-up (the others on the worker's slab in global memory)
constexpr int kHugeThreads = 512;
constexpr int kHugeMW = 4;       // <= 128 leaves
static_assert(MMW_RING_MAX * MMW_MAX_PTS_LIMIT <= 4096 && 2 * (MMW_RING_MAX * MMW_MAX_PTS_LIMIT / 30 + 1) <= 64 * 2 * kHugeMW, "the largest cloud: 12 position bits in the labelling's seed key, <= 128 leaves");
constexpr int kHugeWorkers = 64;
__host__ __device__ __forceinline__ size_t huge_lds_bytes(int UM, int CL)
{
    size_t hot = 0;
    db_hybrid_layout<false>(UM, CL, nullptr, nullptr, nullptr, kHugeMW, &hot);
    return hot;
}

// clusters a cloud of `um` points can hold (min_samples points each), capped by the track list
__host__ __device__ inline int db_class_cl(int um, int t_cap, int min_samples)
{
    const int cl = um / (min_samples > 0 ? min_samples : 1) + 1;
    return cl < t_cap ? cl : t_cap;
}

}  // namespace mmw
