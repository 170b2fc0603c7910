// mmw_balltree.hpp -- apply_DBscan (Utils.py:250-291) with scikit-learn's BallTree semantics for one cloud on one workgroup
// (dbscan_core), its carve-up (DbLds), and TrackBuffer._add_tracks (Tracking.py:576-589, 697-703) behind it (spawn_scene):
// what every DBSCAN kernel (k_dbscan.hip) instantiates.
//
// Why a BallTree on a GPU: the reference hands sklearn a Python callable metric,
// sklearn answers with BallTree(leaf_size=30) over all 8 columns, and because the
// "distance" violates the triangle inequality the tree's prune / take-all
// shortcuts change the neighbour sets (13 % of queries differ from brute force on
// the synthetic scenes).  Bit-matching cluster ids therefore means reproducing the
// tree: split dimensions over 8 features, (value,index) median partition, ball
// centroids/radii, and the per-node PRUNE / ALL / leaf-TEST decision of
// BinaryTree._query_radius_single (sklearn/neighbors/_binary_tree.pxi.tp:1903-1980).
//
// Layout: x,y,z of the candidate points sit in LDS as fp64 SoA (indexed by point
// index); `idx` maps tree position -> point index so every node is a contiguous
// position range.  A query leaves a 2-bit state per leaf (64-bit mask per point); for
// clouds of <= 512 points it also records the neighbourhood itself as a bit row, and
// the labelling runs on the (transposed) bit matrix alone; larger clouds re-use the
// leaf states.  query_radius is walked one WAVE at a time (uniform node / level).
#pragma once
#include <cstddef>
#include "mmw_device.hpp"
#include "mmw_math.hpp"
#include "mmw_cloud.hpp"

namespace mmw {

// Diagnostic build only (make STAMPS=1): per-phase cycle sums of lane 0 into stats[20 + phase].
#ifdef MMW_STAMPS
#define DSTAMP(k)                                                                            \
    do {                                                                                     \
        if (threadIdx.x == 0 && dbg) {                                                       \
            const unsigned long long t_now = __builtin_amdgcn_s_memtime();                  \
            atomicAdd(&dbg[20 + (k)], t_now - t_prev);                                       \
            t_prev = t_now;                                                                  \
        }                                                                                    \
    } while (0)
#define DSTAMP_INIT unsigned long long t_prev = __builtin_amdgcn_s_memtime();
#else
#define DSTAMP(k)
#define DSTAMP_INIT
#endif

struct DbLds {
    double *X, *Y, *Z;             // [UM] by point index during the build, by tree position afterwards
    double *key;                   // [UM] split value by position (build) ...
    unsigned long long *mask;      // ... aliased: per-position leaf-state mask (query/label)
    int *idx;                      // [UM] position -> point index
    int *idx2;                     // [UM] partition target (build); labels by point index (output)
    int *lab;                      // [UM] labels by position
    int *front;                    // [UM]
    int *next;                     // [UM]
    unsigned char *core;           // [UM]
    unsigned char *leafpos;        // [UM] leaf number of a position
    int *nstart, *nend;            // [nodes+1]
    double *nsum;                  // [nodes][3]
    double *ncen;                  // [nodes][3]
    unsigned long long *nrad;      // [nodes] radius as raw bits (>= 0 so bit order == value order)
    unsigned long long *mm;        // [leaves/2][8][2] sortable min/max keys of the nodes of one level
    int *sdim;                     // [leaves/2]
    int *lbase;                    // [leaves/2] left-count scan value at node start
    int *blk;                      // [UM/64 + 1] block counts / prefixes
    int *misc;                     // [16]
    int *cnt;                      // [NB][CL+1] cluster member counting (spawn)
    int *cl_n, *cl_off;            // [CL+2]
    double *ccen;                  // [CL+1][6]
    double *fst;                   // [kFrontChunk][4] frontier staging of the labelling: mask bits, x, y, z
    unsigned long long *adj;       // [min(UM, kAdjMax)][W] + [4][8]: the eps-neighbourhoods of clouds of <= kAdjMax points as bit rows
                                   // (tree positions), then the frontier / reached / labelled / core sets of the labelling
};

__host__ __device__ inline size_t db_align16(size_t v) { return (v + 15) & ~(size_t)15; }

__host__ __device__ inline int db_pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

__host__ __device__ inline int db_levels(int U)
{
    // BinaryTree.__init__: n_levels = int(log2(max(1,(n-1)/leaf_size)) + 1)  (_binary_tree.pxi.tp:876-878)
    int n_levels = 1;
    while ((U - 1) >= kLeafSize * (1 << n_levels)) n_levels++;
    return n_levels;
}

// WRITE=false only sizes the layout (see k_track.hip: no null test on the private struct).
// ALL8 build: private copies of the per-node min/max keys (picked by lane & 7), merged after the atomics -- all
// lanes of a wave hitting the same sixteen LDS words serialise 64-fold
constexpr int kMmCopies = 8;
// (the 512-thread build of k_dbscan_big takes four: with eight its carve-up would cost a workgroup per CU)
__host__ __device__ inline int db_mm_copies(int UM) { return UM > 256 ? 4 : kMmCopies; }
constexpr int kFrontChunk = 32;
// Clouds of up to kAdjMax points keep their neighbourhoods as bit rows (query_radius writes them, dbscan_inner then works on
// bits alone): 32 KiB at 512 points, 8 KiB at 256.
constexpr int kAdjMax = 512;
// (the carve-up of the largest capacities, 1537 .. 1920 points, has room for 256-point rows only: 160 KiB of LDS)
__host__ __device__ inline int db_adj_cap(int UM) { return UM > 1536 ? 256 : (UM < kAdjMax ? UM : kAdjMax); }
// (rows are ((U + 63) / 64) | 1 words apart: an odd stride keeps the lanes of a wave, one row each, on different banks)
__host__ __device__ inline int db_adj_words(int UM)
{
    const int cap = db_adj_cap(UM);
    return cap * (((cap + 63) / 64) | 1) + 32;
}

// Transpose a 64 x 64 bit tile held one row per lane (bit c of lane i's word <-> bit i of lane c's word): six rounds of
// swapping the off-diagonal blocks with the partner lane.
__device__ __forceinline__ unsigned long long transpose64(unsigned long long x, int lane)
{
    unsigned long long m = 0x00000000FFFFFFFFULL;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, j), hi = __shfl_xor((unsigned)(x >> 32), j);
        const unsigned long long y = ((unsigned long long)hi << 32) | lo;
        x = (lane & j) == 0 ? (x & m) | ((y & m) << j) : (x & ~m) | ((y & ~m) >> j);
        m ^= m << (j >> 1);
    }
    return x;
}

// MW = 64-bit words of a position's leaf-state mask (two bits per leaf): 1 for the LDS-resident classes (<= 32 leaves, the mask
// lies over key[]), more for the clouds of more than 1920 points, whose carve-up lives in global memory (k_dbscan_huge).
__host__ __device__ inline int db_mask_words(int UM)
{
    const int leaves = 1 << (db_levels(UM) - 1);
    return (2 * leaves + 63) / 64 > 1 ? (2 * leaves + 63) / 64 : 1;
}
__host__ __device__ inline int db_front_stride(int MW) { return MW == 1 ? 4 : 4 + MW; }  // doubles per staged frontier entry: mask word 0, x, y, z, (mask words 1..)
template <bool WRITE>
__host__ __device__ __forceinline__ size_t db_lds_layout(int UM, int CL, bool all8, char *base, DbLds *L, int MW = 1)
{
    const int NB = (UM + 63) / 64;
    const int levels = db_levels(UM), nodes = (1 << levels) - 1, half = (1 << (levels - 1)) / 2 > 0 ? (1 << (levels - 1)) / 2 : 1;
    size_t off = 0;
#define CARVE(field, type, count)                       \
    if constexpr (WRITE) L->field = (type *)(base + off);  \
    off = db_align16(off + sizeof(type) * (size_t)(count));
    CARVE(X, double, UM)
    CARVE(Y, double, UM)
    CARVE(Z, double, UM)
    if constexpr (WRITE) L->mask = (unsigned long long *)(base + off);
    // (thread-per-point build: key[] / front[] are also the cross-wave exchange of the sort, one slot per THREAD -- 256
    // threads up to a capacity of 256 points, 512 wherever it is above, see db_mm_copies -- whatever the capacity: a context
    // whose ring holds fewer points than the kernel has threads still sorts over every thread slot.  With UM slots the
    // idle threads' keys ran over idx[] .. nend[] for rings of fewer than ~150 points: found by tests/test_gpu_fuzz.py)
    const int xslots = UM <= 256 ? 256 : (UM < 512 ? 512 : UM);
    CARVE(key, double, all8 ? xslots : db_pow2ceil(UM))   // (generic build: also the 64-bit half of the sort keys, one per slot)
    CARVE(idx, int, UM)
    CARVE(idx2, int, UM)
    CARVE(lab, int, UM)
    CARVE(front, int, all8 ? xslots : db_pow2ceil(UM))    // (generic build: the 32-bit half of the sort keys)
    CARVE(next, int, UM)
    CARVE(core, unsigned char, UM)
    CARVE(leafpos, unsigned char, UM)
    CARVE(nstart, int, nodes + 1)
    CARVE(nend, int, nodes + 1)
    CARVE(nsum, double, nodes * 3)
    CARVE(ncen, double, nodes * 3)
    CARVE(nrad, unsigned long long, nodes + 1)
    CARVE(mm, unsigned long long, half * 16 * (all8 ? db_mm_copies(UM) : 1))
    CARVE(sdim, int, half)
    CARVE(lbase, int, half)
    CARVE(blk, int, (NB + 1) > 64 ? (NB + 1) : 64)
    CARVE(misc, int, 16)
    CARVE(cnt, int, NB *(CL + 1))
    CARVE(cl_n, int, CL + 2)
    CARVE(cl_off, int, CL + 2)
    CARVE(ccen, double, (CL + 1) * 6)
    CARVE(fst, double, kFrontChunk * db_front_stride(MW))
    CARVE(adj, unsigned long long, db_adj_words(UM))
    if (MW > 1) { CARVE(mask, unsigned long long, (size_t)UM * MW) }
#undef CARVE
    return off;
}

// The carve-up of a cloud the LDS cannot hold (k_dbscan_huge): the arrays every phase hammers -- the three coordinate columns,
// the exchange slots of the level sort, the per-node min / max words of the build -- in the LDS (152 KB at 4096 points), all the
// others in a slab of global memory.  Returns the slab's bytes, *hot_bytes = the LDS bytes.  (generic build only: all8 = false)
template <bool WRITE>
__host__ __device__ __forceinline__ size_t db_hybrid_layout(int UM, int CL, char *hot, char *cold, DbLds *L, int MW, size_t *hot_bytes)
{
    const int NB = (UM + 63) / 64;
    const int levels = db_levels(UM), nodes = (1 << levels) - 1, half = (1 << (levels - 1)) / 2 > 0 ? (1 << (levels - 1)) / 2 : 1;
    size_t oh = 0, oc = 0;
#define HOT(field, type, count)                            \
    if constexpr (WRITE) L->field = (type *)(hot + oh);    \
    oh = db_align16(oh + sizeof(type) * (size_t)(count));
#define COLD(field, type, count)                           \
    if constexpr (WRITE) L->field = (type *)(cold + oc);   \
    oc = db_align16(oc + sizeof(type) * (size_t)(count));
    HOT(X, double, UM)
    HOT(Y, double, UM)
    HOT(Z, double, UM)
    HOT(key, double, db_pow2ceil(UM))
    HOT(front, int, db_pow2ceil(UM))
    HOT(mm, unsigned long long, half * 16)
    HOT(sdim, int, half)
    HOT(lbase, int, half)
    HOT(misc, int, 16)
    COLD(idx, int, UM)
    COLD(idx2, int, UM)
    COLD(lab, int, UM)
    COLD(next, int, UM)
    COLD(core, unsigned char, UM)
    COLD(leafpos, unsigned char, UM)
    COLD(nstart, int, nodes + 1)
    COLD(nend, int, nodes + 1)
    COLD(nsum, double, nodes * 3)
    COLD(ncen, double, nodes * 3)
    COLD(nrad, unsigned long long, nodes + 1)
    COLD(blk, int, (NB + 1) > 64 ? (NB + 1) : 64)
    COLD(cnt, int, NB *(CL + 1))
    COLD(cl_n, int, CL + 2)
    COLD(cl_off, int, CL + 2)
    COLD(ccen, double, (CL + 1) * 6)
    COLD(fst, double, kFrontChunk * db_front_stride(MW))
    COLD(adj, unsigned long long, db_adj_words(UM))
    COLD(mask, unsigned long long, (size_t)UM * (MW > 1 ? MW : 1))
#undef HOT
#undef COLD
    if (hot_bytes) *hot_bytes = oh;
    return oc;
}

__device__ __forceinline__ int node_of(const DbLds &L, int p, int level)
{
    int node = 0;
    for (int t = 0; t < level; t++) {
        const int s = L.nstart[node], e = L.nend[node];
        const int mid = s + (e - s) / 2;
        node = 2 * node + 1 + (p >= mid ? 1 : 0);
    }
    return node;
}

// ---- bitonic network over the NT thread slots of a workgroup, 96-bit keys (hi64, lo32) --------------------
// Partner exchange for distance J: DPP inside quads (J = 1, 2) and inside rows of 16 (J = 4, 8: the two row
// shifts, picked by the lane's bit J), ds_bpermute for 16 and 32, LDS + barriers across waves.
template <int J>
__device__ __forceinline__ unsigned xor_lane32(unsigned v, int lane)
{
    if constexpr (J == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    else if constexpr (J == 4 || J == 8) {
        const unsigned up = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + J, 0xF, 0xF, true);  // row_shl: lane i <- i + J
        const unsigned dn = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + J, 0xF, 0xF, true);  // row_shr: lane i <- i - J
        return (lane & J) ? dn : up;
    } else return (unsigned)__shfl_xor((int)v, J);
}

template <int K, int J, int NT>
__device__ __forceinline__ void bitonic_round(unsigned long long &hi64, unsigned &lo32, int tid, unsigned long long *xh, unsigned *xl)
{
    unsigned long long ph;
    unsigned pl;
    if constexpr (J >= 64) {
        xh[tid] = hi64; xl[tid] = lo32;
        __syncthreads();
        ph = xh[tid ^ J]; pl = xl[tid ^ J];
        __syncthreads();
    } else {
        const int lane = tid & 63;
        const unsigned a = xor_lane32<J>((unsigned)hi64, lane), b = xor_lane32<J>((unsigned)(hi64 >> 32), lane);
        ph = ((unsigned long long)b << 32) | a;
        pl = xor_lane32<J>(lo32, lane);
    }
    const bool up = (tid & K) == 0, lower = (tid & J) == 0;
    const bool pless = ph < hi64 || (ph == hi64 && pl < lo32);  // partner sorts before me
    if ((lower == up) ? pless : !pless) { hi64 = ph; lo32 = pl; }  // lower slot keeps the smaller one when ascending
}
template <int K, int J, int NT>
struct BitonicJ {
    static __device__ __forceinline__ void run(unsigned long long &h, unsigned &l, int tid, unsigned long long *xh, unsigned *xl)
    {
        bitonic_round<K, J, NT>(h, l, tid, xh, xl);
        if constexpr (J > 1) BitonicJ<K, J / 2, NT>::run(h, l, tid, xh, xl);
    }
};
template <int K, int NT>
struct BitonicK {
    static __device__ __forceinline__ void run(unsigned long long &h, unsigned &l, int tid, unsigned long long *xh, unsigned *xl)
    {
        BitonicJ<K, K / 2, NT>::run(h, l, tid, xh, xl);
        if constexpr (K < NT) BitonicK<K * 2, NT>::run(h, l, tid, xh, xl);
    }
};

// The fp32 screen of one leaf for this lane's query (see dbscan_core, query_radius): n <= 60 candidates whose fp32
// coordinates lie at xf / yf / zf (uniform addresses: LDS broadcasts), two per packed instruction.  Returns the bits of the
// candidates whose fp32 metric is <= lo ("inside" for certain); `amb` = those in (lo, hi] -- for the fp64 formula.  Each
// comparison lands in its word through the carry: v_cmp -> vcc, then word = 2 word + vcc in one v_addc.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned long long leaf_screen(const float *xf, const float *yf, const float *zf, int n, float px, float py, float pz,
                                                          float c, float zw, float lo, float hi, unsigned long long &amb)
{
    const f32x2 PX = {px, px}, PY = {py, py}, PZ = {pz, pz}, NC = {-c, -c}, ONE = {1.0f, 1.0f}, ZW = {zw, zw};
    unsigned in0 = 0u, no0 = 0u, in1 = 0u, no1 = 0u;
    auto metric2 = [&](const f32x2 bx, const f32x2 by, const f32x2 bz) {
        const f32x2 w = __builtin_elementwise_fma(PY + by, NC, ONE);
        const f32x2 dx = PX - bx, dy = PY - by, dz = PZ - bz;
        f32x2 D = dx * dx;
        D = __builtin_elementwise_fma(dy, dy, D);
        D = __builtin_elementwise_fma(dz * ZW, dz, D);
        return w * D;
    };
    // four candidates a round: their twelve coordinates are requested together (past the leaf's end: stray values, masked below)
    auto quad = [&](int k, unsigned &inw, unsigned &now) {
        const f32x2 bx0 = {xf[k], xf[k + 1]}, by0 = {yf[k], yf[k + 1]}, bz0 = {zf[k], zf[k + 1]};
        const f32x2 bx1 = {xf[k + 2], xf[k + 3]}, by1 = {yf[k + 2], yf[k + 3]}, bz1 = {zf[k + 2], zf[k + 3]};
        const f32x2 d0 = metric2(bx0, by0, bz0), d1 = metric2(bx1, by1, bz1);
        asm volatile("v_cmp_ge_f32 vcc, %6, %2\n\t"
                     "v_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %7, %2\n\t"
                     "v_addc_co_u32 %1, vcc, %1, %1, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %6, %3\n\t"
                     "v_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %7, %3\n\t"
                     "v_addc_co_u32 %1, vcc, %1, %1, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %6, %4\n\t"
                     "v_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %7, %4\n\t"
                     "v_addc_co_u32 %1, vcc, %1, %1, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %6, %5\n\t"
                     "v_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                     "v_cmp_ge_f32 vcc, %7, %5\n\t"
                     "v_addc_co_u32 %1, vcc, %1, %1, vcc"
                     : "+v"(inw), "+v"(now)
                     : "v"(d0.x), "v"(d0.y), "v"(d1.x), "v"(d1.y), "v"(lo), "v"(hi)
                     : "vcc");
    };
    n = __builtin_amdgcn_readfirstlane(n);  // (uniform by construction: scalar loop counters)
    const int n4 = (n + 3) & ~3, nA = n4 < 32 ? n4 : 32, nB = n4 - nA;
    for (int k = 0; k < nA; k += 4) quad(k, in0, no0);
    for (int k = 32; k < n4; k += 4) quad(k, in1, no1);
    // candidate k of a word that took m of them sits at bit m - 1 - k
    unsigned long long inb = nA > 0 ? (unsigned long long)(__brev(in0) >> (32 - nA)) : 0ULL;
    unsigned long long nob = nA > 0 ? (unsigned long long)(__brev(no0) >> (32 - nA)) : 0ULL;
    if (nB > 0) {
        inb |= (unsigned long long)(__brev(in1) >> (32 - nB)) << 32;
        nob |= (unsigned long long)(__brev(no1) >> (32 - nB)) << 32;
    }
    const unsigned long long valid = n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL);
    inb &= valid;
    amb = nob & ~inb & valid;
    return inb;
}

// The whole of DBSCAN.fit_predict for one cloud.  On return L.idx2[i] = label of
// point i (-1 noise) and the number of clusters is returned (uniform).
template <int NT, bool ALL8, int MW = 1>
__device__ __forceinline__ int dbscan_core(const DevCfg &cfg, const DbLds &L, const RowSrc src, int U, int UMc, double eps, int min_samples,
                                           unsigned long long *dbg, bool screened = false)
{
    DSTAMP_INIT
    (void)dbg;
    const int tid = threadIdx.x, lane = tid & 63;
    const double rw = cfg.db_range_weight, zw = cfg.db_z_weight;

    // ---- stage x,y,z in LDS (by point index); identity order.  ALL8 (U <= NT): thread i owns
    //      point i and keeps all 8 of its columns in registers for the whole tree build ----
    double f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0, f6 = 0, f7 = 0;
    int mypos = tid;  // ALL8: tree position of point `tid`
    if (ALL8) {
        if (tid < U) {
            const double2 *r2 = reinterpret_cast<const double2 *>(src.row(tid));
            const double2 a = r2[0], b = r2[1], c = r2[2], d = r2[3];
            f0 = a.x; f1 = a.y; f2 = b.x; f3 = b.y; f4 = c.x; f5 = c.y; f6 = d.x; f7 = d.y;
            L.X[tid] = f0; L.Y[tid] = f1; L.Z[tid] = f2;
            L.idx[tid] = tid;
            L.lab[tid] = -1;
            L.front[tid] = 0;
        }
    } else {
        for (int i = tid; i < U; i += NT) {
            const double *r = src.row(i);
            L.X[i] = r[0]; L.Y[i] = r[1]; L.Z[i] = r[2];
            L.idx[i] = i;
            L.lab[i] = -1;
        }
    }
    const int n_levels = db_levels(U);
    const int n_nodes = (1 << n_levels) - 1;
    if (tid == 0) { L.nstart[0] = 0; L.nend[0] = U; L.mm[0] = ~0ULL; L.mm[1] = 0ULL; L.misc[3] = 0; }
    __syncthreads();

    // ---- exact early exit: can ANY point reach min_samples tree-neighbours? ----
    // metric(a,b) = w_ab * E(a,b)^2 with E the weighted Euclidean norm sqrt(dx^2+dy^2+z_w*dz^2) (a true
    // norm for z_w >= 0) and w_ab = 1 - range_w*(ay+by)/2 >= wmin > 0 over the data's y range (node
    // centroids are means, so their y lies in that range too).  A BallTree neighbour q of p is either
    // leaf-tested, metric(p,q) <= eps => E(p,q)^2 <= eps/wmin, or taken with a whole node of centroid
    // c: metric(p,c) + radius <= eps with radius >= metric(c,q), so by the triangle inequality of E
    // E(p,q)^2 <= (sqrt(m(p,c)/wmin) + sqrt(m(c,q)/wmin))^2 <= 2*(m(p,c)+radius)/wmin <= 2*eps/wmin.
    // If no point has min_samples points (itself included) within E^2 <= 2*eps/wmin there is no core
    // point and every label is -1 -- exactly what sklearn returns -- and the tree is never built.
    // Steady-state rings of clutter end here.
    if (!screened && min_samples > 1 && zw >= 0.0 && eps >= 0.0) {
        double ylo = 1.7976931348623157e308, yhi = -1.7976931348623157e308;
        for (int i = tid; i < U; i += NT) {
            const double y = L.Y[i];
            ylo = y < ylo ? y : ylo;
            yhi = y > yhi ? y : yhi;
        }
        ylo = wave_min_d(ylo);
        yhi = wave_max_d(yhi);
        if (lane == 0 && ylo <= yhi) { atomicMin(&L.mm[0], sortable(ylo)); atomicMax(&L.mm[1], sortable(yhi)); }
        __syncthreads();
        const double ymin = unsortable(L.mm[0]), ymax = unsortable(L.mm[1]);
        const double wa = 1 - ymax * rw, wb = 1 - ymin * rw;
        const double wmin = wa < wb ? wa : wb;
        if (wmin > 0.0) {  // wave-uniform (same LDS values for every thread)
            const double R2 = 2.0 * (eps / wmin) * (1.0 + 1e-9);
            const int bparts = ALL8 ? (NT / U > 0 ? NT / U : 1) : 1;
            bool dense = false;
            if (!ALL8 || bparts == 1) {
                // the larger clouds: one dense point settles the question ("a core point is possible"), and a cloud
                // that holds a cluster has one within a few dozen candidates -- 64 at a time, then a look at the
                // flag the other threads may have raised
                for (int p = tid; p < U && !dense; p += NT) {
                    const double px = L.X[p], py = L.Y[p], pz = L.Z[p];
                    int c = 0;
                    for (int q0 = 0; q0 < U && !dense; q0 += 64) {
                        const int q1 = q0 + 64 < U ? q0 + 64 : U;
#pragma unroll 4
                        for (int q = q0; q < q1; q++) {
                            const double dx = px - L.X[q], dy = py - L.Y[q], dz = pz - L.Z[q];
                            c += ((dx * dx + dy * dy) + zw * (dz * dz) <= R2) ? 1 : 0;
                        }
                        if (c >= min_samples) { dense = true; L.misc[3] = 1; }
                        else if (L.misc[3] != 0) dense = true;
                    }
                }
            } else
            for (int t = tid; t < U * bparts; t += NT) {
                const int part = t / U, p = t - part * U;
                const double px = L.X[p], py = L.Y[p], pz = L.Z[p];
                int c = 0;
#pragma unroll 4
                for (int q = part; q < U; q += bparts) {
                    const double dx = px - L.X[q], dy = py - L.Y[q], dz = pz - L.Z[q];
                    c += ((dx * dx + dy * dy) + zw * (dz * dz) <= R2) ? 1 : 0;
                }
                if (bparts > 1) atomicAdd(&L.front[p], c);  // slices of one point add up in LDS
                else if (c >= min_samples) dense = true;
            }
            if (ALL8 && bparts > 1) {
                __syncthreads();
                if (tid < U && L.front[tid] >= min_samples) dense = true;
            }
            if (dense) L.misc[3] = 1;
            __syncthreads();
#ifdef MMW_STAMPS
            if (tid == 0 && dbg && L.misc[3] == 0) atomicAdd(&dbg[31], 1ULL);
#endif
            if (L.misc[3] == 0) {
                for (int i = tid; i < U; i += NT) L.idx2[i] = -1;
                __syncthreads();
                return 0;
            }
        }
    }

    auto feature = [&](int i, int f) -> double {
        if (f == 0) return L.X[i];
        if (f == 1) return L.Y[i];
        if (f == 2) return L.Z[i];
        return src.row(i)[f];
    };

    DSTAMP(0);
    // ---- _recursive_build, level by level (_binary_tree.pxi.tp:1040-1084) ----
    int *idx = L.idx, *idx2 = L.idx2;
    if (ALL8) {
        // Thread-per-point build: min/max by fire-and-forget LDS atomics, the median split by ONE bitonic sort
        // of the whole level, stable partition by ballots in lane (= point index) order.
        const int wave = tid >> 6;
        constexpr int MC = NT > 256 ? 4 : kMmCopies;  // == db_mm_copies(UMc): NT = 256 serves UMc <= 256, NT = 512 the larger class
        unsigned long long *xh = reinterpret_cast<unsigned long long *>(L.key);  // cross-wave exchange of the sort
        unsigned *xl = reinterpret_cast<unsigned *>(L.front);                     // (key[] / front[] are free here)
        unsigned char *leftflag = L.core;                                          // (free until the queries)
        int *posarr = L.next;   // point index -> tree position
        if (tid < U) posarr[tid] = tid;
        for (int level = 0; level + 1 < n_levels; level++) {
            const int first = (1 << level) - 1, nn = 1 << level;
            for (int e = tid; e < MC * nn * 16; e += NT) L.mm[e] = (e & 1) ? 0ULL : ~0ULL;
            __syncthreads();
            const bool act = tid < U;
            const int node = act ? node_of(L, mypos, level) : -1;
            if (act) {  // find_node_split_dim over all 8 features (_binary_tree.pxi.tp:598-645)
                unsigned long long *m = &L.mm[((lane & (MC - 1)) * nn + (node - first)) * 16];
                atomicMin(&m[0], sortable(f0)); atomicMax(&m[1], sortable(f0));
                atomicMin(&m[2], sortable(f1)); atomicMax(&m[3], sortable(f1));
                atomicMin(&m[4], sortable(f2)); atomicMax(&m[5], sortable(f2));
                atomicMin(&m[6], sortable(f3)); atomicMax(&m[7], sortable(f3));
                atomicMin(&m[8], sortable(f4)); atomicMax(&m[9], sortable(f4));
                atomicMin(&m[10], sortable(f5)); atomicMax(&m[11], sortable(f5));
                atomicMin(&m[12], sortable(f6)); atomicMax(&m[13], sortable(f6));
                atomicMin(&m[14], sortable(f7)); atomicMax(&m[15], sortable(f7));
            }
            __syncthreads();
            if (tid < nn * 16) {  // merge the private copies into copy 0
                unsigned long long v[MC];
#pragma unroll
                for (int q = 0; q < MC; q++) v[q] = L.mm[q * nn * 16 + tid];
                unsigned long long r = v[0];
#pragma unroll
                for (int q = 1; q < MC; q++) r = (tid & 1) ? (v[q] > r ? v[q] : r) : (v[q] < r ? v[q] : r);
                L.mm[tid] = r;
            }
            __syncthreads();
            DSTAMP(6);  // (diagnostic) min/max
            if (tid < nn) {
                double lo[8], hi[8];
#pragma unroll
                for (int f = 0; f < 8; f++) { lo[f] = unsortable(L.mm[(tid * 8 + f) * 2]); hi[f] = unsortable(L.mm[(tid * 8 + f) * 2 + 1]); }
                int jmax = 0;
                double best = 0;
#pragma unroll
                for (int f = 0; f < 8; f++) {
                    const double spread = hi[f] - lo[f];
                    if (spread > best) { best = spread; jmax = f; }
                }
                L.sdim[tid] = jmax;
            }
            __syncthreads();
            double kp = 0.0;
            int s = 0, e = 0;
            if (act) {
                const int sd = L.sdim[node - first];
                kp = sd == 0 ? f0 : sd == 1 ? f1 : sd == 2 ? f2 : sd == 3 ? f3 : sd == 4 ? f4 : sd == 5 ? f5 : sd == 6 ? f6 : f7;
                s = L.nstart[node];
                e = L.nend[node];
            }
            DSTAMP(7);  // (diagnostic) split dim + keys
            // partition_node_indices: the n_mid smallest under (value, index) go left
            // (_partition_nodes.pyx:35-39); both halves keep ascending point-index order.
            // Rank under (value, index) inside the node = position after sorting the whole level by
            // (node, value, index), minus the node's start (the nodes of a level are consecutive position
            // ranges in node order).  96-bit sort key: node(16) | order-preserving value bits(64) | point(16);
            // a bitonic network over the NT thread slots, cross-lane inside a wave, through LDS across waves.
            unsigned long long hi64 = ~0ULL;  // idle slots sort to the end
            unsigned lo32 = ~0u;
            if (act) {
                const unsigned long long sk = sortable(kp);
                hi64 = ((unsigned long long)node << 48) | (sk >> 16);
                lo32 = ((unsigned)(sk & 0xffffULL) << 16) | (unsigned)tid;
            }
            BitonicK<2, NT>::run(hi64, lo32, tid, xh, xl);
            if (hi64 != ~0ULL) {  // slot `tid` now holds the tid-th element of the level
                const int snode = (int)(hi64 >> 48), owner = (int)(lo32 & 0xffffu);
                const int ss = L.nstart[snode], ee = L.nend[snode];
                leftflag[owner] = (tid - ss) < (ee - ss) / 2 ? 1 : 0;
            }
            __syncthreads();
            const bool left = act && leftflag[tid] != 0;
            DSTAMP(8);  // (diagnostic) rank
            unsigned long long mine = 0;
            for (int nd = 0; nd < nn; nd++) {
                const unsigned long long b = __ballot(act && left && node == first + nd);
                if (node == first + nd) mine = b;
                if (lane == 0) L.blk[wave * nn + nd] = __popcll(b);
            }
            __syncthreads();
            int np = mypos;
            if (act) {
                int lc = __popcll(mine & lanemask_lt());  // lefts of my node with a smaller point index
                for (int w = 0; w < wave; w++) lc += L.blk[w * nn + (node - first)];
                const int nmid = (e - s) / 2;
                np = left ? s + lc : s + nmid + ((mypos - s) - lc);
                idx2[np] = tid;
                posarr[tid] = np;
            }
            if (tid < nn) {
                const int nd = first + tid, ss = L.nstart[nd], ee = L.nend[nd], nmid = (ee - ss) / 2;
                L.nstart[2 * nd + 1] = ss; L.nend[2 * nd + 1] = ss + nmid;
                L.nstart[2 * nd + 2] = ss + nmid; L.nend[2 * nd + 2] = ee;
            }
            DSTAMP(9);  // (diagnostic) partition
            mypos = np;
            { int *t = idx; idx = idx2; idx2 = t; }
            __syncthreads();
        }
    } else
    for (int level = 0; level + 1 < n_levels; level++) {
        const int first = (1 << level) - 1, nn = 1 << level;
        for (int e = tid; e < nn * 16; e += NT) L.mm[e] = (e & 1) ? 0ULL : ~0ULL;  // [node][f][0]=min key, [1]=max key
        __syncthreads();
        // find_node_split_dim over all 8 features (_binary_tree.pxi.tp:598-645)
        for (int p0 = 0; p0 < U; p0 += NT) {
            const int p = p0 + tid;
            const bool act = p < U;
            const int node = act ? node_of(L, p, level) : -1;
            const int nfirst = __builtin_amdgcn_readfirstlane(node);
            const bool uniform = __all(node == nfirst) != 0;  // wave-uniform
            const int i = act ? idx[p] : 0;
            const double *r = (!ALL8 && act) ? src.row(i) : nullptr;
#pragma unroll
            for (int f = 0; f < 8; f++) {
                double v = 0.0;
                if (act) v = ALL8 ? feature(i, f) : r[f];
                if (uniform) {
                    if (nfirst >= 0) {
                        const double mn = wave_min_d(v), mx = wave_max_d(v);
                        if (lane == 0) {
                            atomicMin(&L.mm[((nfirst - first) * 8 + f) * 2], sortable(mn));
                            atomicMax(&L.mm[((nfirst - first) * 8 + f) * 2 + 1], sortable(mx));
                        }
                    }
                } else if (act) {
                    atomicMin(&L.mm[((node - first) * 8 + f) * 2], sortable(v));
                    atomicMax(&L.mm[((node - first) * 8 + f) * 2 + 1], sortable(v));
                }
            }
        }
        __syncthreads();
        if (tid < nn) {
            int jmax = 0;
            double best = 0;
            for (int f = 0; f < 8; f++) {
                const double spread = unsortable(L.mm[(tid * 8 + f) * 2 + 1]) - unsortable(L.mm[(tid * 8 + f) * 2]);
                if (spread > best) { best = spread; jmax = f; }
            }
            L.sdim[tid] = jmax;
        }
        __syncthreads();
        DSTAMP(6);  // (diagnostic) min/max + split dim
        // partition_node_indices: the n_mid smallest under (value, index) go left
        // (_partition_nodes.pyx:35-39); both halves keep ascending point-index order.
        // Rank inside the node = slot after sorting the whole level by (node, value, point index), minus the
        // node's start (see the ALL8 branch).  Here the 96-bit keys live in LDS, one slot per position, and the
        // bitonic network runs over them: every thread owns pairs (i, i + j), so one barrier per round.
        {
            unsigned long long *xh = reinterpret_cast<unsigned long long *>(L.key);
            unsigned *xl = reinterpret_cast<unsigned *>(L.front);
            unsigned char *leftflag = L.core;  // by point index (free until the queries)
            const int Upad = db_pow2ceil(U);
            if (Upad <= NT && db_pow2ceil(UMc) >= NT) {  // (the exchange arrays hold pow2ceil(UMc) slots)
                // one slot per thread: the register network of the ALL8 build (cross-lane inside a wave, LDS only
                // for partner distances >= 64) -- 6 exchange rounds through LDS instead of 45 for 512 slots
                unsigned long long h = ~0ULL;  // padding sorts to the end
                unsigned l = ~0u;
                if (tid < U) {
                    const int node = node_of(L, tid, level), i = idx[tid];
                    const unsigned long long sk = sortable(feature(i, L.sdim[node - first]));
                    h = ((unsigned long long)node << 48) | (sk >> 16);
                    l = ((unsigned)(sk & 0xffffULL) << 16) | (unsigned)i;
                }
                BitonicK<2, NT>::run(h, l, tid, xh, xl);
                if (tid < U) {  // slot tid holds the tid-th element of the level
                    const int snode = (int)(h >> 48), owner = (int)(l & 0xffffu);
                    const int ss = L.nstart[snode], ee = L.nend[snode];
                    leftflag[owner] = (tid - ss) < (ee - ss) / 2 ? 1 : 0;
                }
                __syncthreads();
            } else {
            for (int p = tid; p < Upad; p += NT) {
                unsigned long long h = ~0ULL;  // padding sorts to the end
                unsigned l = ~0u;
                if (p < U) {
                    const int node = node_of(L, p, level), i = idx[p];
                    const unsigned long long sk = sortable(feature(i, L.sdim[node - first]));
                    h = ((unsigned long long)node << 48) | (sk >> 16);
                    l = ((unsigned)(sk & 0xffffULL) << 16) | (unsigned)i;
                }
                xh[p] = h; xl[p] = l;
            }
            __syncthreads();
            for (int k = 2; k <= Upad; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < Upad / 2; t += NT) {
                        const int i = 2 * j * (t / j) + (t % j), q = i + j;
                        const unsigned long long ah = xh[i], bh = xh[q];
                        const unsigned al = xl[i], bl = xl[q];
                        const bool b_first = bh < ah || (bh == ah && bl < al);  // element q sorts before element i
                        if (b_first == ((i & k) == 0)) { xh[i] = bh; xl[i] = bl; xh[q] = ah; xl[q] = al; }
                    }
                    __syncthreads();
                }
            for (int t = tid; t < U; t += NT) {  // slot t holds the t-th element of the level
                const int snode = (int)(xh[t] >> 48), owner = (int)(xl[t] & 0xffffu);
                const int ss = L.nstart[snode], ee = L.nend[snode];
                leftflag[owner] = (t - ss) < (ee - ss) / 2 ? 1 : 0;
            }
            __syncthreads();
            }
        }
        DSTAMP(8);  // (diagnostic) keys + rank
        const int NBLK = (U + 63) / 64;
        for (int p0 = 0; p0 < U; p0 += NT) {
            const int p = p0 + tid;
            const bool left = p < U && L.core[idx[p]] != 0;
            const unsigned long long b = __ballot(left);
            if (p0 + (tid & ~63) < U && lane == 0) L.blk[(p0 + tid) >> 6] = __popcll(b);
            // stash (rank of p among the lefts of its 64-block) | left flag in lab[] (restored to -1 below)
            if (p < U) L.lab[p] = __popcll(b & lanemask_lt()) | (left ? 0x40000000 : 0);
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int b = 0; b < NBLK; b++) { const int t = L.blk[b]; L.blk[b] = run; run += t; }
        }
        __syncthreads();
        for (int p = tid; p < U; p += NT) {  // scan value at node starts
            const int node = node_of(L, p, level);
            if (p == L.nstart[node]) L.lbase[node - first] = L.blk[p >> 6] + (L.lab[p] & 0x3fffffff);
        }
        __syncthreads();
        for (int p = tid; p < U; p += NT) {
            const int node = node_of(L, p, level);
            const int s = L.nstart[node], e = L.nend[node], nmid = (e - s) / 2;
            const int lb = L.blk[p >> 6] + (L.lab[p] & 0x3fffffff) - L.lbase[node - first];  // lefts in [s, p)
            const bool left = (L.lab[p] & 0x40000000) != 0;
            const int np = left ? s + lb : s + nmid + ((p - s) - lb);
            idx2[np] = idx[p];
        }
        __syncthreads();
        for (int p = tid; p < U; p += NT) L.lab[p] = -1;
        if (tid < nn) {
            const int node = first + tid, s = L.nstart[node], e = L.nend[node], nmid = (e - s) / 2;
            L.nstart[2 * node + 1] = s; L.nend[2 * node + 1] = s + nmid;
            L.nstart[2 * node + 2] = s + nmid; L.nend[2 * node + 2] = e;
        }
        { int *t = idx; idx = idx2; idx2 = t; }
        __syncthreads();
        DSTAMP(9);  // (diagnostic) partition
    }

    DSTAMP(1);
    // ---- init_node: centroids (leaf sums in ascending index order, parents = left + right)
    //      and radii (_ball_tree.pyx.tp:84-144) ----
    const int leaf0 = (1 << (n_levels - 1)) - 1, n_leaves = 1 << (n_levels - 1);
    for (int t = tid; t < n_leaves * 3; t += NT) {
        const int node = leaf0 + t / 3, c = t % 3;
        const double *col = c == 0 ? L.X : (c == 1 ? L.Y : L.Z);
        double acc = 0.0;
        int p = L.nstart[node];
        const int pe = L.nend[node];
        for (; p + 8 <= pe; p += 8) {  // (index loads, then value loads, then the adds in index order)
            int ii[8];
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) ii[u] = idx[p + u];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = col[ii[u]];
#pragma unroll
            for (int u = 0; u < 8; u++) acc += v[u];
        }
        for (; p < pe; p++) acc += col[idx[p]];
        L.nsum[node * 3 + c] = acc;
    }
    for (int p = tid; p < U; p += NT) L.leafpos[p] = (unsigned char)(node_of(L, p, n_levels - 1) - leaf0);
    for (int e = tid; e < n_nodes; e += NT) L.nrad[e] = 0ULL;
    __syncthreads();
    for (int level = n_levels - 2; level >= 0; level--) {
        const int first = (1 << level) - 1, nn = 1 << level;
        for (int t = tid; t < nn * 3; t += NT) {
            const int node = first + t / 3, c = t % 3;
            L.nsum[node * 3 + c] = L.nsum[(2 * node + 1) * 3 + c] + L.nsum[(2 * node + 2) * 3 + c];
        }
        __syncthreads();
    }
    for (int t = tid; t < n_nodes * 3; t += NT) {
        const int node = t / 3;
        L.ncen[t] = L.nsum[t] / (double)(L.nend[node] - L.nstart[node]);
    }
    // From here on x,y,z are addressed by TREE POSITION (leaf ranges become contiguous reads):
    // permute the three columns in place (every by-index read above is complete: barrier in the loop).
    if (ALL8) {
        __syncthreads();
        if (tid < U) { L.X[mypos] = f0; L.Y[mypos] = f1; L.Z[mypos] = f2; }
    } else {
        for (int c = 0; c < 3; c++) {
            double *col = c == 0 ? L.X : (c == 1 ? L.Y : L.Z);
            __syncthreads();
            for (int p = tid; p < U; p += NT) L.key[p] = col[idx[p]];
            __syncthreads();
            for (int p = tid; p < U; p += NT) col[p] = L.key[p];
        }
    }
    // fp32 copies of the coordinates by tree position, for the screen in front of the leaf tests of query_radius (below): in
    // the three arrays that are dead between the build and the labelling -- the spare one of idx / idx2, next, lab (the
    // labelling's -1 are written again behind the queries) -- and the extents the screen's error bound needs
    float *XF = reinterpret_cast<float *>(idx2), *YF = reinterpret_cast<float *>(L.next), *ZF = reinterpret_cast<float *>(L.lab);
    if constexpr (MW > 1) {
        // (the clouds of more than 1920 points, db_hybrid_layout: those three are in global memory there, while the exchange slots of
        //  the level sort -- key[] and front[], in the LDS, dead after the build; the masks have their own array -- hold exactly
        //  three fp32 columns)
        XF = reinterpret_cast<float *>(L.key);
        YF = XF + UMc;
        ZF = reinterpret_cast<float *>(L.front);
    }
    if (tid == 0) { L.mm[0] = ~0ULL; L.mm[1] = 0ULL; L.mm[2] = 0ULL; }
    __syncthreads();
    double ext_lo = 1.7976931348623157e308, ext_hi = -1.7976931348623157e308, ext_m = 0.0;
    for (int p0 = 0; p0 < U; p0 += NT) {
        const int p = p0 + tid;
        const bool act = p < U;
        const int i = act ? p : 0;
        const double px = L.X[i], py = L.Y[i], pz = L.Z[i];
        if (act) {
            XF[p] = (float)px; YF[p] = (float)py; ZF[p] = (float)pz;
            ext_lo = py < ext_lo ? py : ext_lo;
            ext_hi = py > ext_hi ? py : ext_hi;
            const double ax = fabs(px), ay = fabs(py), az = fabs(pz);
            double am = ax > ay ? ax : ay;
            am = am > az ? am : az;
            ext_m = am > ext_m ? am : ext_m;   // (a NaN coordinate never enters: its comparisons are false in fp32 as in fp64)
        }
        int node = 0;
        for (int level = 0; level < n_levels; level++) {
            double d = act ? alt_dist(L.ncen[node * 3], L.ncen[node * 3 + 1], L.ncen[node * 3 + 2], px, py, pz, rw, zw) : 0.0;
            if (!(d > 0.0)) d = 0.0;
            const int nfirst = __builtin_amdgcn_readfirstlane(act ? node : -1);
            const bool uniform = __all((act ? node : -1) == nfirst) != 0;
            if (uniform) {
                const double mx = wave_max_d(d);
                if (lane == 0 && nfirst >= 0) atomicMax(&L.nrad[nfirst], (unsigned long long)__double_as_longlong(mx));
            } else if (act) {
                atomicMax(&L.nrad[node], (unsigned long long)__double_as_longlong(d));
            }
            if (level + 1 < n_levels) {
                const int s = L.nstart[node], e = L.nend[node];
                node = 2 * node + 1 + (p >= s + (e - s) / 2 ? 1 : 0);
            }
        }
    }
    ext_lo = wave_min_d(ext_lo);
    ext_hi = wave_max_d(ext_hi);
    ext_m = wave_max_d(ext_m);
    if (lane == 0 && ext_lo <= ext_hi) {
        atomicMin(&L.mm[0], sortable(ext_lo));
        atomicMax(&L.mm[1], sortable(ext_hi));
        atomicMax(&L.mm[2], (unsigned long long)__double_as_longlong(ext_m));
    }
    __syncthreads();

    DSTAMP(2);
    // ---- BallTree.query_radius(X, eps) for every point (_binary_tree.pxi.tp:1903-1980) ----
    const int lbits = n_levels - 1;
    // NearestNeighbors._fit with algorithm="auto" (sklearn/neighbors/_base.py:622-633): DBSCAN leaves n_neighbors at its default
    // of 5, and `n_neighbors >= n_samples // 2` answers clouds of 1 .. 11 points by BRUTE FORCE -- the exact pairwise metric
    // `<= eps` (_base.py:1054-1081, 1221-1250), no tree: the root (the only node of so small a cloud) is a TEST leaf for every
    // query, never PRUNE, never taken whole.  (Reachable with DB_MIN_SAMPLES_MIN <= 11; the no-core-point screens bound a
    // superset of either neighbourhood.)
    const bool brute = (U >> 1) <= kSkNeighbors;  // uniform
    // The leaf tests -- "is metric(p, q) <= eps" for every point q of a leaf some query of the wave reached: nine tenths of
    // this phase, 14 fp64 operations each -- go through an fp32 SCREEN first: the same formula on the fp32 copies, two
    // candidates per packed instruction, decides every pair whose fp32 value is further than E from eps; the few in between
    // are computed in fp64 as before.  E bounds |metric_fp32 - metric_fp64| for all pairs whose coordinate differences are
    // within R, R^2 = 4 max(eps, 1) / (wmin min(1, z_w)) (beyond R the metric is >= 4 max(eps, 1) and its fp32 value within
    // 15 % of it: "out" either way), from |coordinates| <= M and y in [ymin, ymax] (u = 2^-23, twice the unit roundoff; a
    // difference is off by <= 2Mu + 2u|d|, its square by <= 4RMu + 6uR^2, the weight by <= 12cMu + 4u, c = |range_w| / 2),
    // doubled.  Clouds whose extents make E useless (or the far-pair argument void) skip the screen: the decisions -- and with
    // them counts, rows, labels -- are those of the fp64 formula in every case.
    float scr_lo = 0.f, scr_hi = 0.f;
    bool use_scr = false;
    {
        const double ymin = unsortable(L.mm[0]), ymax = unsortable(L.mm[1]), M = __longlong_as_double((long long)L.mm[2]);
        const double wa = 1 - ymax * rw, wb = 1 - ymin * rw, wmin = wa < wb ? wa : wb;
        const double u = 1.0 / 8388608.0, c = 0.5 * fabs(rw), mz = zw < 1.0 ? zw : 1.0, e1 = eps > 1.0 ? eps : 1.0;
        if (wmin > 0.0 && zw >= 1.0 / 1024.0 && eps > 0.0 && L.mm[0] != ~0ULL) {
            const double R2 = 4.0 * e1 / (wmin * mz), R = sqrt(R2), Wm = 1.0 + 2.0 * c * M, Dm = (2.0 + zw) * R2;
            const double dD = (2.0 + zw) * (4.0 * R * M * u + 6.0 * u * R2) + 4.0 * u * Dm, dw = 12.0 * c * M * u + 4.0 * u;
            const double E = 2.0 * (Wm * dD + Dm * dw + 2.0 * u * Wm * Dm) + eps * (1.0 / 4194304.0);
            if (M <= 65536.0 * R && dw <= 0.1 * wmin && E < 0.25 * (eps < 1.0 ? eps : 1.0)) {
                use_scr = true;
#ifdef MMW_MUTANT_NO_MARGIN   // (mutation check of tests/test_gpu_parity.py::test_dbscan_pairs_at_the_threshold_vs_oracle: never the product)
                scr_lo = scr_hi = (float)eps;
#else
                scr_lo = (float)(eps - E);
                scr_hi = (float)(eps + E);
#endif
            }
        }
    }
    // A WAVE walks the tree as one: its 64 queries are neighbours in the tree (one or two leaves), so the nodes any of them
    // needs are nearly the nodes each of them needs -- and with node and level uniform every branch below is taken by
    // the whole wave, the candidates of a leaf are read once (one LDS broadcast per coordinate) and the distance block runs
    // on full lanes.  (One thread walking alone per query left the SIMDs ~25 % busy: every lane at its own node.)  Per lane:
    // `alive` bit l = "the walk reached this level's node through DESCEND states of mine".  The per-lane visit order is the
    // order of the private walk, so masks, counts and rows are the same.
    // Spare waves (thread-per-point build, U <= NT / 2) share the queries: slice `qpart` of `qparts` takes every qparts-th
    // candidate of a TEST leaf; counts meet in an LDS counter.
    const int Wq = (U + 63) >> 6;  // waves that hold one query each per lane
    const int qparts = ALL8 ? ((NT >> 6) / Wq > 0 ? (NT >> 6) / Wq : 1) : 1;
    int *qcount = L.front;
    // Clouds of <= kAdjMax points also record WHICH points are within eps: row p of L.adj, one bit per tree position, set
    // exactly where the labelling below would find "q in query_radius(p)" (a node taken whole: its range; a tested leaf:
    // the points that passed).  dbscan_inner then never touches a coordinate again.
    const bool use_adj = U <= db_adj_cap(UMc);  // uniform
    const int W = (U + 63) >> 6, WS = W | 1;
    unsigned long long *adj = L.adj;
    if (use_adj)
        for (int e = tid; e < U * WS + 32; e += NT) adj[e] = 0ULL;
    if (ALL8 && qparts > 1)
        for (int p = tid; p < U; p += NT) qcount[p] = 0;
    if (use_adj || (ALL8 && qparts > 1)) __syncthreads();
    {
        const int wv = tid >> 6;
        const int qpart = __builtin_amdgcn_readfirstlane(ALL8 ? wv / Wq : 0);  // (uniform per wave)
        const int pbase = ALL8 ? (wv - qpart * Wq) * 64 : wv * 64;
        const int pstep = ALL8 ? U : NT;                           // (thread-per-point build: one batch)
        for (int pb = pbase; pb < U && qpart < qparts; pb += pstep) {
            const int p = pb + lane;
            const bool act = p < U;
            const double px = L.X[act ? p : 0], py = L.Y[act ? p : 0], pz = L.Z[act ? p : 0];
            const float pxf = (float)px, pyf = (float)py, pzf = (float)pz, cf = (float)(0.5 * rw), zwf = (float)zw;
            unsigned long long m[MW];
#pragma unroll
            for (int w = 0; w < MW; w++) m[w] = 0ULL;
            int count = 0, node = 0, level = 0;  // node, level: uniform
            unsigned alive = 1u;
            for (;;) {
                int state = 0;  // 0 prune (or not mine), 1 all, 2 leaf test, 3 descend
                if (act && ((alive >> level) & 1u)) {
                    const double d = alt_dist(px, py, pz, L.ncen[node * 3], L.ncen[node * 3 + 1], L.ncen[node * 3 + 2], rw, zw);
                    const double rad = __longlong_as_double((long long)L.nrad[node]);
                    const double t = d - rad;
                    const double lb = t > 0 ? t : 0, ub = d + rad;
                    if (brute) state = 2;   // (one node: level == lbits == 0)
                    else if (lb > eps) state = 0;
                    else if (ub <= eps) state = 1;
                    else if (level == lbits) state = 2;
                    else state = 3;
                }
                // (the same LDS words for every lane: scalar from here on, the loops below are uniform)
                const int s = __builtin_amdgcn_readfirstlane(L.nstart[node]), e = __builtin_amdgcn_readfirstlane(L.nend[node]);
                if (state == 1 || state == 2) {
                    const int span = 1 << (lbits - level);
                    const int fl = (node + 1 - (1 << level)) * span;
                    const unsigned long long pat = state == 1 ? 0x5555555555555555ULL : 0xAAAAAAAAAAAAAAAAULL;
                    if constexpr (MW == 1) {
                        const unsigned long long sel = span == 32 ? ~0ULL : ((1ULL << (2 * span)) - 1ULL);
                        m[0] |= (pat & sel) << (2 * fl);
                    } else {
#pragma unroll
                        for (int w = 0; w < MW; w++) {  // bits [2 fl, 2 fl + 2 span) of the mask, word by word
                            const int lo = 2 * fl - 64 * w, hi = lo + 2 * span;
                            if (hi > 0 && lo < 64) {
                                const int a = lo < 0 ? 0 : lo, b = hi > 64 ? 64 : hi;
                                const unsigned long long sel = b - a == 64 ? ~0ULL : (((1ULL << (b - a)) - 1ULL) << a);
                                m[w] |= pat & sel;
                            }
                        }
                    }
                }
                if (state == 1 && qpart == 0) {
                    count += e - s;
                    if (use_adj)
                        for (int w = s >> 6; w <= (e - 1) >> 6; w++) {
                            const int lo = (s > w * 64 ? s : w * 64) - w * 64, hi = (e < w * 64 + 64 ? e : w * 64 + 64) - w * 64;
                            const unsigned long long bits = (hi == 64 ? ~0ULL : ((1ULL << hi) - 1ULL)) & ~((1ULL << lo) - 1ULL);
                            atomicOr(&adj[p * WS + w], bits);
                        }
                }
                if (level == lbits && __any(state == 2)) {
                    // (a leaf holds at most 2 * leaf_size = 60 points: one word of bits relative to its start, two row words)
                    // (spare waves: slice `qpart` of the leaf; everything here is uniform but the lane's own state and bits)
                    const int n = e - s, per = (n + qparts - 1) / qparts;
                    const int a = __builtin_amdgcn_readfirstlane(qpart * per < n ? qpart * per : n), b = a + per < n ? a + per : n;
                    unsigned long long bits = 0ULL, amb_all = b - a >= 64 ? ~0ULL : ((1ULL << (b - a)) - 1ULL);
                    if (use_scr && b > a) bits = leaf_screen(XF + s + a, YF + s + a, ZF + s + a, b - a, pxf, pyf, pzf, cf, zwf, scr_lo, scr_hi, amb_all);
                    unsigned long long amb = state == 2 ? amb_all : 0ULL;  // (the lanes that do not test this leaf drop their bits below)
                    while (amb) {  // what the screen left open (without it: every candidate): the fp64 formula
                        const int k = __ffsll((long long)amb) - 1;
                        amb &= amb - 1ULL;
                        const int q = s + a + k;
                        if (alt_dist(px, py, pz, L.X[q], L.Y[q], L.Z[q], rw, zw) <= eps) bits |= 1ULL << k;
                    }
                    bits <<= a;
                    if (state == 2) {
                        count += __popcll(bits);
                        if (use_adj) {
                            const int w0 = s >> 6, lo = s & 63;
                            const unsigned long long b0 = bits << lo, b1 = lo ? bits >> (64 - lo) : 0ULL;
                            if (b0) atomicOr(&adj[p * WS + w0], b0);
                            if (b1) atomicOr(&adj[p * WS + w0 + 1], b1);
                        }
                    }
                }
                if (__any(state == 3)) {
                    alive = (alive & ~(2u << level)) | (state == 3 ? 2u << level : 0u);
                    node = 2 * node + 1;
                    level++;
                    continue;
                }
                while (node != 0 && (node & 1) == 0) { node = (node - 1) >> 1; level--; }  // climb while right child
                if (node == 0) break;
                node++;  // left child -> its sibling
            }
            if (act) {
                // the key[] buffer is dead after the build: it now holds the masks
                if (qpart == 0) {
#pragma unroll
                    for (int w = 0; w < MW; w++) L.mask[(size_t)p * MW + w] = m[w];
                }
                if (qparts > 1) atomicAdd(&qcount[p], count);
                else L.core[p] = count >= min_samples ? 1 : 0;
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < U; p += NT) L.lab[p] = -1;  // (held the fp32 z column during the queries)
    if (qparts > 1)
        for (int p = tid; p < U; p += NT) L.core[p] = qcount[p] >= min_samples ? 1 : 0;
    __syncthreads();

    DSTAMP(3);
    // ---- dbscan_inner (sklearn/cluster/_dbscan_inner.pyx): clusters seeded in ascending
    //      point index; frontier expansion instead of the DFS stack (same labels) ----
    int n_clusters = 0;
    int *front = L.front, *next = L.next;
    if (use_adj) {
        // Bit-set form.  The rows are transposed first (row q then says WHO has q in its neighbourhood: the distance itself
        // is symmetric, bit for bit, but the rows are not -- the tree takes whole nodes by a bound that is no true triangle
        // inequality for this weighted distance -- so a cluster is what its seed reaches along rows of cores, in seed
        // order, exactly dbscan_inner's; a union-find would not do).  One round of the expansion is then,
        // per unlabelled point, a few ANDs of its row with the frontier set F and a ballot: no atomics, one barrier.
        unsigned long long *F0 = adj + U * WS, *F1 = F0 + 8;
        {
            const int wave = tid >> 6, nw = NT >> 6;
            int pair = 0;
            for (int a = 0; a < W; a++)
                for (int b = a; b < W; b++, pair++) {
                    if (pair % nw != wave) continue;  // (uniform per wave)
                    const int ra = a * 64 + lane, rb = b * 64 + lane;
                    unsigned long long x = ra < U ? adj[ra * WS + b] : 0ULL;             // tile (a, b)
                    unsigned long long y = (a != b && rb < U) ? adj[rb * WS + a] : 0ULL;  // tile (b, a)
                    x = transpose64(x, lane);
                    if (a != b) y = transpose64(y, lane);
                    if (a == b) { if (ra < U) adj[ra * WS + a] = x; }
                    else {
                        if (rb < U) adj[rb * WS + a] = x;
                        if (ra < U) adj[ra * WS + b] = y;
                    }
                }
        }
        __syncthreads();
        for (;;) {
            if (tid == 0) L.misc[0] = 0x7fffffff;
            __syncthreads();
            {
                int best = 0x7fffffff;
                for (int p = tid; p < U; p += NT)
                    if (L.core[p] && L.lab[p] < 0) { const int k = idx[p] * 4096 + p; best = k < best ? k : best; }
                for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(best, o); best = t < best ? t : best; }
                if (lane == 0 && best != 0x7fffffff) atomicMin(&L.misc[0], best);
            }
            __syncthreads();
            const int seedkey = L.misc[0];
            if (seedkey == 0x7fffffff) break;
            __syncthreads();
            const int sp = seedkey & 4095;
            if (tid < 8) F0[tid] = (sp >> 6) == tid ? 1ULL << (sp & 63) : 0ULL;
            if (tid == 0) L.lab[sp] = n_clusters;
            __syncthreads();
            unsigned long long *Fc = F0, *Fn = F1;
            for (;;) {
                for (int p0 = 0; p0 < U; p0 += NT) {
                    const int p = p0 + tid;
                    bool hit = false;
                    if (p < U && L.lab[p] < 0) {
                        unsigned long long acc = 0ULL;
                        for (int w = 0; w < W; w++) acc |= adj[p * WS + w] & Fc[w];
                        hit = acc != 0ULL;
                    }
                    if (hit) L.lab[p] = n_clusters;
                    const unsigned long long hb = __ballot(hit && L.core[p]);
                    if (lane == 0 && p < U) Fn[p >> 6] = hb;  // (whole words: a wave's points share one)
                }
                __syncthreads();
                unsigned long long any = 0ULL;
                for (int w = 0; w < W; w++) any |= Fn[w];  // (uniform: the same LDS words for every thread)
                if (!any) break;
                { unsigned long long *t = Fc; Fc = Fn; Fn = t; }
            }
            n_clusters++;
        }
    } else
    for (;;) {
        if (tid == 0) L.misc[0] = 0x7fffffff;
        __syncthreads();
        {
            int best = 0x7fffffff;
            for (int p = tid; p < U; p += NT)
                if (L.core[p] && L.lab[p] < 0) { const int k = idx[p] * 4096 + p; best = k < best ? k : best; }
            for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(best, o); best = t < best ? t : best; }
            if (lane == 0 && best != 0x7fffffff) atomicMin(&L.misc[0], best);
        }
        __syncthreads();
        const int seedkey = L.misc[0];
        if (seedkey == 0x7fffffff) break;
        __syncthreads();
        if (tid == 0) { const int sp = seedkey & 4095; L.lab[sp] = n_clusters; front[0] = sp; L.misc[2] = 0; }
        __syncthreads();
        int fcount = 1;
        while (fcount > 0) {
            // The frontier goes through a contiguous staging array, kFrontChunk points at a time: every thread
            // then reads the same addresses (LDS broadcast) that depend on nothing it loaded before, so one
            // round trip brings four entries instead of a position load followed by four dependent gathers.
            for (int f0 = 0; f0 < fcount; f0 += kFrontChunk) {
                const int fc = fcount - f0 < kFrontChunk ? fcount - f0 : kFrontChunk;
                if (f0 > 0) __syncthreads();  // the previous chunk has been consumed
                constexpr int FS = MW == 1 ? 4 : 4 + MW;  // (db_front_stride)
                if (tid < fc) {
                    const int pp = front[f0 + tid];
                    L.fst[tid * FS + 0] = __longlong_as_double((long long)L.mask[(size_t)pp * MW]);
                    L.fst[tid * FS + 1] = L.X[pp];
                    L.fst[tid * FS + 2] = L.Y[pp];
                    L.fst[tid * FS + 3] = L.Z[pp];
#pragma unroll
                    for (int w = 1; w < MW; w++) L.fst[tid * FS + 3 + w] = __longlong_as_double((long long)L.mask[(size_t)pp * MW + w]);
                }
                __syncthreads();
                for (int q = tid; q < U; q += NT) {
                    if (L.lab[q] >= 0) continue;
                    const int lq = L.leafpos[q];
                    const double qx = L.X[q], qy = L.Y[q], qz = L.Z[q];
                    bool hit = false;
                    for (int f = 0; f < fc && !hit; f += 4) {
                        double4 en[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const double2 *e2 = reinterpret_cast<const double2 *>(L.fst + (f + u < fc ? f + u : f) * FS);
                            const double2 a = e2[0], b = e2[1];
                            en[u] = make_double4(a.x, a.y, b.x, b.y);
                            if constexpr (MW > 1) {  // the mask word this point's leaf lies in
                                if ((lq >> 5) != 0) en[u].x = L.fst[(f + u < fc ? f + u : f) * FS + 3 + (lq >> 5)];
                            }
                        }
                        // leaf states first: most (point, frontier point) pairs are PRUNE, and a wave's 64 points
                        // sit in one or two leaves, so the distance block below is skipped by whole waves
                        int stt[4];
                        bool test = false;
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            stt[u] = (int)(((unsigned long long)__double_as_longlong(en[u].x) >> (2 * (lq & 31))) & 3ULL);
                            hit = hit || stt[u] == 1;
                            test = test || stt[u] == 2;
                        }
                        if (test && !hit) {
#pragma unroll
                            for (int u = 0; u < 4; u++)
                                if (stt[u] == 2 && alt_dist(en[u].y, en[u].z, en[u].w, qx, qy, qz, rw, zw) <= eps) hit = true;
                        }
                    }
                    if (hit) {
                        L.lab[q] = n_clusters;
                        if (L.core[q]) next[atomicAdd(&L.misc[2], 1)] = q;
                    }
                }
            }
            __syncthreads();
            fcount = L.misc[2];
            __syncthreads();
            if (tid == 0) L.misc[2] = 0;
            { int *t = front; front = next; next = t; }
            __syncthreads();
        }
        n_clusters++;
    }
    DSTAMP(4);
    // labels by point index: scatter into whichever of the two index buffers is free,
    // the caller always finds them in L.idx2
    int *labi = (idx == L.idx) ? L.idx2 : L.idx;
    for (int p = tid; p < U; p += NT) labi[idx[p]] = L.lab[p];
    __syncthreads();
    if (labi != L.idx2) {
        for (int i = tid; i < U; i += NT) L.idx2[i] = labi[i];
        __syncthreads();
    }
    return n_clusters;
}

// Tracking.py:697-703 for the scenes of one size class: apply_DBscan on the global ring,
// batch.clear(), _add_tracks.
__device__ __forceinline__ void finish_scene_stats(const DevState &st, int s, int U, int ncl)
{
    if (st.stats) {  // algorithmic bytes: ring rows in, labels out, new track records + ring rows out
        unsigned long long *sl = stats_slot(st, s);
        atomicAdd(&sl[1], (unsigned long long)(64 * U + 4 * U) + (unsigned long long)ncl * (sizeof(TrackRec) + 64ULL * 64ULL));
        atomicAdd(&sl[3], 1ULL);
        atomicAdd(&sl[4], (unsigned long long)U);
        atomicAdd(&sl[7], (unsigned long long)ncl);
    }
}

// _add_tracks (Tracking.py:576-589) for `nspawn` clusters of the cloud dbscan_core has just labelled: cluster c is
// the set of points with label lab0 + c (rows keep input order, Utils.py:285-287); its track is appended at list
// position T0 + c.  All threads of the workgroup call; L.misc[4] holds the first creation ordinal.
template <int NT>
__device__ __forceinline__ void add_clusters(const DevCfg &cfg, const DevState &st, const DbLds &L, const RowSrc src, int s, int U, int CL,
                                             int lab0, int nspawn, int T0)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int *labi = L.idx2;
    // members of every cluster in ascending point index
    const int NB = (U + 63) / 64, CLS = CL + 1;
    for (int i0 = 0; i0 < U; i0 += NT) {
        const int i = i0 + tid;
        const int cls_i = (i < U) ? labi[i] - lab0 : -1;
        const int b = i >> 6;
        if (i0 + (tid & ~63) < U) {
            unsigned long long mine = 0;
            for (int c = 0; c < nspawn; c++) {
                const unsigned long long bal = __ballot(cls_i == c);
                if (cls_i == c) mine = bal;
                if (lane == 0) L.cnt[b * CLS + c] = __popcll(bal);
            }
            if (i < U) L.lab[i] = __popcll(mine & lanemask_lt());  // rank inside its 64-block
        }
    }
    __syncthreads();
    for (int c = tid; c < nspawn; c += NT) {
        int run = 0;
        for (int b = 0; b < NB; b++) { const int t = L.cnt[b * CLS + c]; L.cnt[b * CLS + c] = run; run += t; }
        L.cl_n[c] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int c = 0; c < nspawn; c++) { L.cl_off[c] = run; run += L.cl_n[c]; }
        L.cl_off[nspawn] = run;
    }
    __syncthreads();
    int *memb = L.front;  // free after labelling
    for (int i = tid; i < U; i += NT) {
        const int c = labi[i] - lab0;
        if (c >= 0 && c < nspawn) memb[L.cl_off[c] + L.cnt[(i >> 6) * CLS + c] + L.lab[i]] = i;
    }
    __syncthreads();
    int32_t *order = st.order + (size_t)s * cfg.t_cap;
    TrackRec *trk = st.trk + (size_t)s * cfg.t_cap;
    // PointCluster stats (Tracking.py:120-136): sequential mean in row order
    for (int t = tid; t < nspawn * 6; t += NT) {
        const int c = t / 6, m = t % 6;
        const int n = L.cl_n[c], off = L.cl_off[c];
        TrackRec *rec = trk + order[T0 + c];
        // (rows come from the ring -- the LDS x,y,z are in tree-position order by now --: eight loads in
        //  flight per round trip, the sum itself stays sequential in row order)
        double sum = 0.0, mn = 0.0, mx = 0.0;
        int r = 0;
        for (; r + 8 <= n; r += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = src.row(memb[off + r + u])[m];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                sum += v[u];
                mn = (r + u == 0 || v[u] < mn) ? v[u] : mn;
                mx = (r + u == 0 || v[u] > mx) ? v[u] : mx;
            }
        }
        for (; r < n; r++) {
            const double v = src.row(memb[off + r])[m];
            sum += v;
            mn = (r == 0 || v < mn) ? v : mn;
            mx = (r == 0 || v > mx) ? v : mx;
        }
        const double cen = sum / (double)n;
        L.ccen[c * 6 + m] = cen;
        rec->centroid[m] = cen;
        rec->minv[m] = mn;
        rec->maxv[m] = mx;
    }
    __syncthreads();
    // ClusterTrack.__init__ / KalmanState.__init__ (Tracking.py:87-97, 210-230)
    for (int c = 0; c < nspawn; c++) {
        const int slot = order[T0 + c];
        TrackRec *rec = trk + slot;
        const int n = L.cl_n[c], off = L.cl_off[c];
        for (int e = tid; e < 81; e += NT) {
            const int i = e / 9, k = e % 9;
            rec->P[e] = (i == k && i < cfg.dx) ? 1.0 * cfg.kf_p_init : 0.0;
        }
        for (int e = tid; e < 36; e += NT) rec->gd[e] = (e / 6 == e % 6) ? 1.0 * cfg.kf_group_disp_est_init : 0.0;
        for (int e = tid; e < 9; e += NT) rec->x[e] = e < 6 ? L.ccen[c * 6 + e] : 0.0;
        for (int e = tid; e < 6; e += NT) rec->spread[e] = 0.0;
        for (int e = tid; e < MMW_NKP; e += NT) rec->kp[e] = st.default_posture[e];
        if (tid == 0) {
            const double v3 = L.ccen[c * 6 + 3], v4 = L.ccen[c * 6 + 4], v5 = L.ccen[c * 6 + 5];
            rec->is_static = sqrt((v3 * v3 + v4 * v4) + v5 * v5) < cfg.tr_vel_thres ? 1 : 0;
            rec->point_num = n;
            rec->n_est = 0.0;
            rec->lifetime = 0.0;
            rec->ring_len = 1;
            rec->uid = L.misc[4] + c;
            rec->inner = cfg.ring;  // a fresh BatchedData: size FB_FRAMES_BATCH + 1, associate_pointcloud has not run on it
            for (int k = 0; k < MMW_RING_MAX; k++) { rec->ring_slot[k] = k; rec->ring_n[k] = 0; }
            rec->ring_n[0] = n;
        }
        const int keep = min(n, cfg.ring_rows);
        double *dst = st.trk_ring + (((size_t)s * cfg.t_cap + slot) * cfg.ring + 0) * (size_t)cfg.ring_rows * 8;
        for (int e = tid; e < keep * 8; e += NT) dst[e] = src.row(memb[off + (e >> 3)])[e & 7];
    }
}

template <int NT, bool ALL8, int MW = 1>
__device__ __forceinline__ void spawn_scene(const DevCfg &cfg, const DevState &st, const DbLds &L, int s, int UMc, int CL, int UM_out,
                                            bool screened, int parity, int32_t *__restrict__ labels_out, int32_t *__restrict__ db_n_out)
{
    const int tid = threadIdx.x;
    SceneHdr *hdr = st.hdr + s;
    const int U = hdr->db_u;
    const RowSrc src = ring_rows_of(cfg, st, hdr, s);
    __syncthreads();  // every thread has read the header before anyone rewrites it below
    const int ncl = dbscan_core<NT, ALL8, MW>(cfg, L, src, U, UMc, cfg.db_eps, cfg.db_min_samples, stats_slot(st, s), screened);
    const int *labi = L.idx2;
    if (labels_out)
        for (int i = tid; i < U; i += NT) labels_out[(size_t)s * UM_out + i] = labi[i];
    if (tid == 0) {
        if (db_n_out) db_n_out[s] = U;
        hdr->need_db = 0;
        finish_scene_stats(st, s, U, ncl);
    }
    if (ncl == 0) return;

    // ---- batch.clear() (Tracking.py:53-58) + _add_tracks (Tracking.py:576-589) ----
    const int T0 = hdr->n_tracks;
    int nspawn = ncl;
    int err = 0;
    if (T0 + ncl > cfg.t_cap || ncl > CL) { nspawn = min(max(cfg.t_cap - T0, 0), CL); err |= ERR_CAPACITY; }
    __syncthreads();
    if (tid == 0) {
        hdr->g_len = 0;
        for (int k = 0; k < MMW_RING_MAX; k++) hdr->g_n[k] = 0;
        hdr->n_tracks = T0 + nspawn;
        if (nspawn > 0) {  // the next k_predict takes the new tracks T0.. from here (the older ones from the update lists)
            const int pos = atomicAdd(&st.spc_count[parity], 1);
            st.spc_list[((size_t)parity * cfg.n_scenes + pos) * 2] = s;
            st.spc_list[((size_t)parity * cfg.n_scenes + pos) * 2 + 1] = T0;
        }
        L.misc[4] = hdr->next_uid;
        hdr->next_uid += nspawn;
        if (err) atomicOr(&hdr->err, err);
    }
    add_clusters<NT>(cfg, st, L, src, s, U, CL, 0, nspawn, T0);
}

}  // namespace mmw
