// mmw_uidlist.hpp -- what the by-uid consumers of the live-track list share (k_report.hip, k_zone.hip, k_trail.hip, k_tripwire.hip, k_stance.hip, k_heat.hip):
// the words that say whether a scene's uids are still the ones a consumer remembers, the remembered list itself (report, zones), the
// SLOT TABLE that keeps a word set per live uid from one sample call to the next (trails, tripwires, stance, heat), and the match of two unsorted
// uid lists held one entry per lane.  Registers only; a wave per scene, a lane per entry (t_cap <= 64).  (This lane's live uid is
// live_uid, beside live_tracks and live_slot in mmw_device.hpp, which includes this header for the structs.)
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

// The SLOT TABLE of a consumer that keeps words per live uid between its sample calls (trails: the ring and its totals; tripwires:
// the side word; stance: the class word and two times; heat: the last cell and its time).  A scene has t_cap slots; a slot belongs to one uid or is free, and which slot a uid has is not visible outside.
// Lane j of the scene's wave holds slot j's words, lane i track i's uid.  The slot rule of a sample call:
//   1. a uid of another generation owns nothing (the scene was rebased: every slot counts as free);
//   2. a slot whose uid is live is kept, every other slot is free;
//   3. the r-th newcomer, in live order, takes the r-th free slot -- one that was freed in this very call included;
//   4. a track lane writes its own slot's words, `owner` among them; a slot lane writes only the -1 of a slot that was freed and
//      NOT handed on.  No word has two writers.
// A slot table is taken in a generation, so it extends the generation words: what a consumer holds as `ug` is all of it.
struct UidSlots : UidGen {
    int32_t *ordinal;     // [S] sample calls that asked the scene since the consumer was enabled
    int32_t *owner;       // [S][t_cap] the slot's uid, -1 = free
};

// Steps 1 to 3.  All 64 lanes call, ahead of any condition that only some lanes pass (uid_find).  cuid: this lane's live uid (-1 past
// the T live tracks); raw_owner: this lane's slot's owner word as loaded (-1 past t_cap); rebased: the table's rebased(s).
struct UidSlotPick {
    int slot;             // this lane's TRACK's slot (-1: the lane has no track)
    bool fresh;           // ... which it takes in this call: its words start over
    bool release;         // this lane's SLOT was freed and not handed on: uid_slots_done stores its -1
};
__device__ __forceinline__ UidSlotPick uid_slots_pick(int cuid, int raw_owner, bool rebased, int T, int cap, int lane)
{
    const int owner = rebased ? -1 : raw_owner;   // (1.)
    // the two lists of the wave matched both ways: the slot of this lane's track or -1, and whether this lane's slot belongs to a live uid
    int slot = uid_find(cuid, owner, cap);
    const bool kept = uid_find(owner, cuid, T) >= 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool is_free = lane < cap && !kept;   // (2.)
    const unsigned long long free_b = __ballot(is_free);
    const bool fresh = lane < T && slot < 0;
    const unsigned long long new_b = __ballot(fresh);
    const int n_new = __popcll(new_b);
    if (fresh) {
        unsigned long long f = free_b;
        for (int r = __popcll(new_b & below); r > 0; r--) f &= f - 1ull;   // (divergent: drop the r lowest set bits)
        slot = f ? __ffsll((long long)f) - 1 : -1;   // (never -1: live tracks <= t_cap, so free slots >= newcomers)
    }
    // (this lane's slot, the k-th free one, goes to a newcomer if k < n_new; one that was free before needs no -1)
    return UidSlotPick{slot, fresh, is_free && __popcll(free_b & below) >= n_new && raw_owner != -1};
}

// The tail of a sample call, behind the track lanes' own stores: the released slot's -1, the generation settled, the scene's call
// ordinal (ord: what the call read of it) moved on.
__device__ __forceinline__ void uid_slots_done(const UidSlots &us, int s, int lane, size_t at, bool release, int ord)
{
    if (release) us.owner[at] = -1;   // (freed and not handed on)
    us.settle(s, lane);
    if (lane == 0) us.ordinal[s] = ord + 1;
}

}  // namespace mmw
