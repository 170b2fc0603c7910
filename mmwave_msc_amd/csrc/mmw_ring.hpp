// mmw_ring.hpp -- a track's ring as the exports read it after the step (k_cloud.hip, k_sample.hip).  The rings are slot-permuted:
// logical frame k (k-th oldest) lives in physical slot ring_slot[k] of the track's ring.  A track frame stores
// min(ring_n[k], ring_rows) rows; what the reference holds beyond that is `dropped`.
#pragma once

#include "mmw_device.hpp"

namespace mmw {

static_assert(MMW_RING_MAX == 4, "the frames of a ring are walked unrolled");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One ring as the copy sees it: frames, rows STORED per frame (oldest first; 0 past the ring's length), their physical slots.
struct Ring {
    int len, stored, dropped;
    int n[MMW_RING_MAX], phys[MMW_RING_MAX];
};
__device__ __forceinline__ int phys_slot(int logical, int stored_slot, int ring)
{
#ifdef MMW_MUTANT_CLOUD_IDENT_SLOTS   // (diagnostic build `make DIAG=cloudident DIAGFLAGS=-DMMW_MUTANT_CLOUD_IDENT_SLOTS`, never the
                                      //  product: the permutation ignored -- what tests/test_gpu_clouds.py's oracle comparison must catch)
    return logical % ring;
#else
    return (stored_slot & (MMW_RING_MAX - 1)) % ring;
#endif
}
__device__ __forceinline__ Ring track_ring(const DevCfg &cfg, const TrackRec *rec)
{
    Ring r;
    r.len = clampi(rec->ring_len, 0, cfg.ring);
    r.stored = r.dropped = 0;
#pragma unroll
    for (int k = 0; k < MMW_RING_MAX; k++) {
        const int nk = k < r.len ? max(rec->ring_n[k], 0) : 0;
        r.n[k] = min(nk, cfg.ring_rows);
        r.stored += r.n[k];
        r.dropped += nk - r.n[k];
        r.phys[k] = phys_slot(k, rec->ring_slot[k], cfg.ring);
    }
    return r;
}

}  // namespace mmw
