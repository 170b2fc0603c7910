// mmw_uidlist.hpp -- what the by-uid consumers of the live-track list share (k_report.hip, k_zone.hip, k_trail.hip): the words that
// say whether a scene's uids are still the ones a consumer remembers, the remembered list itself, and the match of two unsorted uid
// lists held one entry per lane.  Registers only; a wave per scene, a lane per entry (t_cap <= 64).  (This lane's live uid is
// live_uid, beside live_tracks and live_slot in mmw_device.hpp, which includes this header for the two structs.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmw {

// Scene and lane of a wave-per-scene kernel: four scenes per 256-thread workgroup.  The wave index goes through readfirstlane, so s
// -- and everything indexed by it alone -- is scalar.
struct WaveScene { int s, lane; };
__device__ __forceinline__ WaveScene wave_scene()
{
    return WaveScene{(int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), (int)(threadIdx.x & 63)};
}

// The generation of every scene's uids, one pair of words per consumer.  mmw_reset / mmw_reset_scenes / mmw_restore bump `gen` of the
// scenes they touch (k_uid_rebase, k_scan.hip): uids restart there, so what the consumer remembers of the scene -- taken in
// generation `seen` -- names other tracks.  A consumer looks with rebased() and, once it has replaced what it remembered, settles.
struct UidGen {
    int32_t *gen;         // [S]
    int32_t *seen;        // [S] the generation the consumer's memory of the scene belongs to
    __device__ __forceinline__ bool rebased(int s) const { return gen[s] != seen[s]; }
    __device__ __forceinline__ void settle(int s, int lane) const { if (lane == 0) seen[s] = gen[s]; }
};

// The BASELINE: the uids that were live at a consumer's previous successful export, in effective_tracks order as it was then.
struct UidBaseline {
    int32_t *base_uid;    // [S][t_cap]
    int32_t *base_len;    // [S] ... and how many
    UidGen ug;
    __device__ __forceinline__ int len(int s, int t_cap) const { return min(base_len[s], t_cap); }
    // this lane's entry, -1 past the list (Tb = len)
    __device__ __forceinline__ int uid(int s, int t_cap, int lane, int Tb) const { return lane < Tb ? base_uid[(size_t)s * t_cap + lane] : -1; }
    // the current list (T entries, this lane's `cuid`) becomes the baseline; the caller settles the generation where it has to
    __device__ __forceinline__ void store(int s, int t_cap, int lane, int T, int cuid) const
    {
        if (lane < T) base_uid[(size_t)s * t_cap + lane] = cuid;
        if (lane == 0) base_len[s] = T;
    }
};

// Where the other list holds this lane's uid.  All 64 lanes call, ahead of any condition that only some lanes pass.  `key` is this
// lane's uid, `other` this lane's entry of the other list, n that list's length.  Returns the position k < n with other[k] == key,
// or -1.  Neither list is sorted, so entry k is broadcast and compared in every lane.  -1 is no uid: a lane past its list (key -1)
// finds nothing, a free entry (-1) matches nobody.  uids are unique inside a scene, so at most one position matches.
__device__ __forceinline__ int uid_find(int key, int other, int n)
{
    const bool has = key != -1;
    int at = -1;
    // (uniform.  k is scalar, so the broadcast is a v_readlane; as __shfl -- a ds_bpermute and a wait each round -- two finds in a row
    // made the report 0.8 us slower than the fused loop they replace, profiles/README.md)
    for (int k = 0; k < n; k++) {
        const int o = __builtin_amdgcn_readlane(other, k);
        at = (has && key == o) ? k : at;
    }
    return at;
}

}  // namespace mmw
