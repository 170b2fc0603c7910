// mmw_evlog.hpp -- the per-scene EVENT LOG of the consumers that append events behind every sample call and hand them out on export
// (k_tripwire.hip, k_stance.hip): the ring, the words that say what was appended and what was handed out, and the three places that
// touch them -- the append of a sample call, the window an export hands out, the drain.  Registers only, no LDS, no atomics; a wave
// per scene (wave_scene, mmw_uidlist.hpp).  What an event carries beside its scene is the consumer's; the log only needs E::scene.
// (mmw_device.hpp includes this header for the struct.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmw {

// The log rule:
//   1. a scene's events are numbered from 0 in the order they were appended; event n lies at ring[n % depth], with the LOCAL scene
//      index.  `logged` counts the events ever appended, `taken` those ever handed out (or passed over, 3.).
//   2. a sample call appends its events behind `logged`.  Of more than `depth` events of ONE call only the newest `depth` are written,
//      so no entry has two writers in a launch; `logged` moves on by all of them.  An entry is written before `logged` lets anybody
//      read it, so a ring needs no clearing.
//   3. an export hands out the events first .. logged - 1, oldest first, with first = max(taken, logged - depth); the events between
//      `taken` and `first` were overwritten before it came and are counted as `lost`.
//   4. nothing is taken unless everything fits: an export whose rows or events do not fit the caller's buffers (k_pair_scan's
//      decision, totals[2]) writes neither buffer nor `taken`, and the next one hands out the same window -- or, after more samples, a
//      later one with more `lost`.
template <class E>
struct EventLog {
    int32_t depth;             // entries per scene, >= 1
    E *ring;                   // [S][depth]
    int32_t *logged, *taken;   // [S]
};

// 2., the plan of one sample call.  log0: `logged` as the call read it; head: the events lane 0 appends in front of the lanes' own
// (0 or 1); n_ev: the lanes' events, summed over the wave.  The event of ordinal n, log0 <= n < log0 + total, is stored to at(n) if
// keeps(n); otherwise it is one of those that the same call overwrites, and is dropped unbuilt.
template <class E>
struct LogAppend {
    E *ring;                   // the scene's
    unsigned depth;
    int log0, head, total, keep_from;
    // the ordinal of a lane's first event (the head's is log0): `at` = the wave-exclusive prefix of the lanes' event counts
    __device__ __forceinline__ int first(int at) const { return log0 + head + at; }
    __device__ __forceinline__ bool keeps(int n) const { return n >= keep_from; }
    __device__ __forceinline__ E &at(int n) const { return ring[(unsigned)n % depth]; }
};
template <class E>
__device__ __forceinline__ LogAppend<E> evlog_append(const EventLog<E> &g, int s, int log0, int head, int n_ev)
{
    const int total = head + n_ev;
    const int keep_from = log0 + max(total - g.depth, 0);
    const unsigned depth = (unsigned)g.depth;
    return LogAppend<E>{g.ring + (size_t)s * depth, depth, log0, head, total, keep_from};
}
// ... and its last store, behind the events'
template <class E>
__device__ __forceinline__ void evlog_commit(const EventLog<E> &g, int s, int lane, const LogAppend<E> &a)
{
    if (lane == 0 && a.total) g.logged[s] = a.log0 + a.total;
}

// 3., what an export hands out of a scene's log: events first .. first + n - 1, and how many were overwritten before it came.
struct LogWindow { int first, n, lost, logged; };
template <class E>
__device__ __forceinline__ LogWindow evlog_window(const EventLog<E> &g, int s)
{
    LogWindow w;
    w.logged = g.logged[s];
    const int taken = g.taken[s];
    w.first = max(taken, w.logged - g.depth);
    w.n = w.logged - w.first;
    w.lost = max(0, w.logged - g.depth - taken);
    return w;
}
// The count kernel of an export: the scene's two counts for k_pair_scan (off: ExportScratch::off), `rows` of the consumer's and the window's n.
template <class E>
__device__ __forceinline__ void evlog_count(const EventLog<E> &g, int32_t *off, int n_scenes, int s, int lane, int rows)
{
    if (lane == 0) {
        off[s] = rows;
        off[n_scenes + 1 + s] = evlog_window(g, s).n;
    }
}
// 4., the gate of the write kernel (totals: ExportScratch::totals; uniform over the launch) ...
__device__ __forceinline__ bool evlog_fits(const int32_t *totals) { return totals[2] != 0; }
// ... and the drain behind it: the lanes stride over the ring, oldest first, the scene index becomes the caller's, events[ev0 ..]
// is the scene's part of the buffer (its scanned offset); lane 0 stores `taken`.
template <class E>
__device__ __forceinline__ void evlog_drain(const EventLog<E> &g, int s, int lane, const LogWindow &w, E *__restrict__ events, int ev0, int scene_base)
{
    const unsigned depth = (unsigned)g.depth;
    const E *ring = g.ring + (size_t)s * depth;
    for (int k = lane; k < w.n; k += 64) {
        E e = ring[(unsigned)(w.first + k) % depth];
        e.scene += scene_base;
        events[ev0 + k] = e;
    }
    if (lane == 0) g.taken[s] = w.logged;
}

}  // namespace mmw
