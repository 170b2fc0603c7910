// mmw_scene_table.hpp -- the per-scene tables of the C-ABI (mmw_set_zones / mmw_get_zones, mmw_set_tripwires / mmw_get_tripwires, mmw_set_stance_rules / mmw_get_stance_rules,
// mmw_set_heat_grids / mmw_get_heat_grids):
// one allocation, one check of a set call's arguments, one way a new table reaches the device, one getter.  Host code only; the
// state is SceneTable (mmw_ctx.hpp).  What differs between the tables comes from the caller: the names the messages speak with,
// the check of one entry and what the device reads of it.
#pragma once

#include "mmw_ctx.hpp"

// `fn` the entry the messages speak for, `counts` / `entries` its two array arguments
struct SceneTableNames { const char *fn, *counts, *entries; };

// The table and its mirrors, every scene at 0 entries (the device block is NOT cleared: a first set call writes all of it, an owner
// whose kernels may run before one clears it).  On failure `tb` is as never allocated.
template <class T>
int scene_table_alloc(mmw_ctx *c, T &tb, const char *fn)
{
    const size_t S = c->dc.n_scenes;
    if (hipMalloc((void **)&tb.d_tab, T::bytes(S)) != hipSuccess) {
        tb.d_tab = nullptr;
        return fail(c, MMW_E_HIP, "%s: hipMalloc(%zu B) failed", fn, T::bytes(S));
    }
    tb.h_entries.assign(S * T::kMax, typename T::entry{});
    tb.h_counts.assign(S, 0);
    return MMW_OK;
}

template <class T>
void scene_table_free(T &tb)
{
    if (tb.d_tab) hipFree(tb.d_tab);
    tb = T();
}

// Every check of a set call, before anything changes: n entries, entry i for scene scenes[i] (scenes == NULL: scene i) with counts[i]
// of the MAX entries at entries[i * MAX].  check(i, s, z, q) looks at entry z of list entry i (scene s) and returns what fail returned.
template <class T, class Check>
int scene_table_check(mmw_ctx *c, const SceneTableNames &nm, const int32_t *scenes, int32_t n, const int32_t *counts, const typename T::entry *entries, Check check)
{
    const int S = c->dc.n_scenes;
    if (n < 0 || n > S) return fail(c, MMW_E_ARG, "%s: n = %d, the context has %d scenes", nm.fn, n, S);
    if (n > 0 && (!counts || !entries)) return fail(c, MMW_E_ARG, "%s: %s is NULL with n = %d", nm.fn, !counts ? nm.counts : nm.entries, n);
    std::vector<char> listed((size_t)S, 0);
    for (int i = 0; i < n; i++) {
        const int s = scenes ? scenes[i] : i;
        if (s < 0 || s >= S) return fail(c, MMW_E_ARG, "%s: entry %d names scene %d, the context has %d scenes", nm.fn, i, s, S);
        if (listed[s]) return fail(c, MMW_E_ARG, "%s: entry %d names scene %d a second time", nm.fn, i, s);
        listed[s] = 1;
        if (counts[i] < 0 || counts[i] > T::kMax)
            return fail(c, MMW_E_ARG, "%s: entry %d (scene %d) has %s = %d, outside 0 .. %d", nm.fn, i, s, nm.counts, counts[i], T::kMax);
        for (int z = 0; z < counts[i]; z++) MMW_TRY(check(i, s, z, entries[(size_t)i * T::kMax + z]));
    }
    return MMW_OK;
}

// A checked set call takes effect.  The new table is put together on the host (from a copy of the mirrors: a failure leaves them as
// they were) and travels as ONE copy, ordered on the context's stream: what was queued before this call reads the old table.  The
// listed scenes' flags ride behind it, for the generation bump of the owner's word `gen` alone and for whatever else `behind(flags)`
// launches on them.  conv(e) is what the device reads of a caller's entry.
template <class T, class Conv, class Behind>
int scene_table_send(mmw_ctx *c, T &tb, const char *fn, const int32_t *scenes, int32_t n, const int32_t *counts, const typename T::entry *entries, Conv conv,
                     int32_t *gen, Behind behind)
{
    using E = typename T::entry;
    const size_t S = (size_t)c->dc.n_scenes, M = T::kMax;
    std::vector<E> next = tb.h_entries;
    std::vector<int32_t> next_n = tb.h_counts;
    std::vector<char> stage(T::bytes(S), 0);
    typename T::dev_entry *dev = reinterpret_cast<typename T::dev_entry *>(stage.data());
    int32_t *st_n = reinterpret_cast<int32_t *>(stage.data() + T::table_bytes(S)), *st_flags = st_n + S;
    for (int i = 0; i < n; i++) {
        const size_t s = scenes ? scenes[i] : i;
        next_n[s] = counts[i];
        st_flags[s] = 1;
        for (size_t z = 0; z < M; z++) next[s * M + z] = (int)z < counts[i] ? entries[(size_t)i * M + z] : E{};
    }
    for (size_t s = 0; s < S; s++)
        for (int z = 0; z < next_n[s]; z++) dev[s * M + z] = conv(next[s * M + z]);
    memcpy(st_n, next_n.data(), sizeof(int32_t) * S);
    hipError_t e = hipMemcpyAsync(tb.d_tab, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_uid_rebase((int)S, tb.flags(S), UidGens{{gen, nullptr, nullptr, nullptr}}, c->stream);
        behind(tb.flags(S));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (`stage` is pageable and goes away)
    if (e != hipSuccess) return fail(c, MMW_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    tb.h_entries.swap(next);
    tb.h_counts.swap(next_n);
    return MMW_OK;
}

// The mirrors into the caller's arrays (either may be NULL); all zero while the table is not allocated.
template <class T>
void scene_table_get(const T &tb, size_t S, int32_t *counts, typename T::entry *entries)
{
    const size_t nb = S * sizeof(int32_t), eb = S * T::kMax * sizeof(typename T::entry);
    if (counts) { if (tb.d_tab) memcpy(counts, tb.h_counts.data(), nb); else memset(counts, 0, nb); }
    if (entries) { if (tb.d_tab) memcpy(entries, tb.h_entries.data(), eb); else memset(entries, 0, eb); }
}
