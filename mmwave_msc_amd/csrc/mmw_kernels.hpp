// mmw_kernels.hpp -- every host-callable launcher and sizing function of the k_*.hip files, declared ONCE: the kernel file
// that defines one includes this header (the compiler checks the definition against it), and so do the api_*.hip files.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmw.h"

namespace mmw {
struct DevCfg;     // mmw_device.hpp (the CNN's kernel files do without it)
struct DevState;
struct ReportState;
struct ZoneState;
struct TrailState;
struct TripState;
struct StanceState;
struct HeatState;
struct UartState;
struct UartLog;
struct ExportScratch;
// k_track.hip, k_kalman.hip, k_scene.hip: the step
size_t track_lds_bytes(const DevCfg &c);
hipError_t prepare_track(const DevCfg &cfg);
void launch_predict(const DevCfg &cfg, const DevState &st, const int32_t *n_pts, const double *dt, int parity, hipStream_t stream);
void launch_track(const DevCfg &cfg, const DevState &st, const void *pts, bool f32, const int32_t *n_pts, const double *dt, int32_t *assoc, int32_t *db_n, int32_t *db_labels, int UM, int parity, hipStream_t stream);
size_t scene_lds_bytes(const DevCfg &c);
hipError_t prepare_scene(const DevCfg &cfg);
void launch_scene(const DevCfg &cfg, const DevState &st, const void *pts, bool f32, const int32_t *n_pts, const double *dt, int32_t *assoc, int32_t *db_n, int32_t *db_labels, int UM, int parity, hipStream_t stream);
// k_dbscan.hip
void launch_post(const DevCfg &cfg, const DevState &st, const int32_t *n_pts, int UM, int u_bound, int parity, int epoch, int32_t *labels, int32_t *db_n, hipStream_t stream);
void launch_chain(const DevCfg &cfg, const DevState &st, int UM, int u_bound, int parity, int epoch, int32_t *labels, int32_t *db_n, hipStream_t side);
size_t dbscan_lds_bytes(int cls, int UM, int t_cap, int min_samples);
size_t dbscan_only_lds_bytes(int UM);
hipError_t prepare_dbscan(int UM, int t_cap, int min_samples);
void launch_dbscan_big(const DevCfg &cfg, const DevState &st, int UM, int u_bound, int parity, int32_t *labels, int32_t *db_n, hipStream_t stream);
hipError_t prepare_inner(const DevCfg &cfg);
size_t inner_lds_demand(const DevCfg &cfg);
int inner_um(const DevCfg &cfg);
void launch_inner(const DevCfg &cfg, const DevState &st, const int32_t *n_pts, int32_t *db_n, hipStream_t stream);
int dbscan_huge_workers(int n_scenes);
size_t dbscan_huge_slab_bytes(int UM, int t_cap, int min_samples);
void launch_dbscan_huge(const DevCfg &cfg, const DevState &st, int UM, int u_bound, int parity, int32_t *labels, int32_t *db_n, hipStream_t stream);
void launch_dbscan_only(const DevCfg &cfg, const DevState &st, int UM, const double *pts, const int32_t *n, int max_n, double eps, int min_samples, int32_t *labels, int32_t *ncl, hipStream_t stream);
// k_misc.hip
// (sites: the context's site table while one is in use -- the kernels' SITE = true instantiations --, else nullptr: the plain kernels)
void launch_normalize(const DevCfg &cfg, const mmw_scene_site *sites, const void *raw, bool f32, const int32_t *n_raw, double *out, int32_t *n_out, hipStream_t st);
void launch_normalize_tlv(const DevCfg &cfg, const mmw_scene_site *sites, const uint8_t *packets, long long packets_bytes, const long long *tlv_offset, double half_bins, double doppler_res, double *out, int32_t *n_out, hipStream_t st);
void launch_feat_scan(const DevCfg &cfg, const DevState &s, int32_t *row_off, hipStream_t st);
void launch_feat_count(const DevCfg &cfg, const DevState &s, int32_t *row_off, hipStream_t st);
// k_feat_models.hip: behind launch_feat_count, the offsets model by model (map: dev [S]; groups: dev [16] = totals[8] | bases[8])
void launch_feat_scan_models(int S, int n_models, int none_off, const int32_t *map, int32_t *row_off, int32_t *groups, hipStream_t st);
void launch_features(const DevCfg &cfg, const mmw_scene_site *sites, const DevState &s, const int32_t *row_off, float *feat, int32_t *owner, int32_t *uid, int cap, hipStream_t st, const int32_t *n_in = nullptr, int32_t *total_out = nullptr, const int32_t *gen = nullptr, int32_t *gen_snap = nullptr);
void launch_set_kp_uid(const DevCfg &cfg, const DevState &s, const float *kp, const int32_t *owner, const int32_t *uid, int n_rows, hipStream_t st, const int32_t *gen = nullptr, const int32_t *gen_snap = nullptr);
void launch_format_frames(const DevCfg &cfg, const double *frames, const int32_t *counts, const double *ref, float *feat, int B, hipStream_t st);
void launch_set_kp(const DevCfg &cfg, const DevState &s, const float *kp, const int32_t *owner, int n_rows, hipStream_t st, const int32_t *dev_rows = nullptr);
void launch_export(const DevCfg &cfg, const DevState &s, mmw_track_record *out, int cap, hipStream_t st);
void launch_table(const DevCfg &cfg, const mmw_scene_site *sites, const DevState &s, mmw_track_summary *out, int slots, int base, hipStream_t st);
void launch_reset(const DevCfg &cfg, const DevState &s, const int32_t *flags, int32_t *kp_gen, hipStream_t st);
void launch_probe_wait(int32_t *w, int slot, int polls, hipStream_t st);
void launch_probe_set(int32_t *w, hipStream_t st);
void launch_pop_frame(const DevCfg &cfg, const DevState &s, const int32_t *flags, hipStream_t st);
void launch_clear_errors(const DevCfg &cfg, const DevState &s, const int32_t *flags, int bits, hipStream_t st);
void launch_set_batch_size(const DevCfg &cfg, const DevState &s, const int32_t *flags, int new_size, hipStream_t st);
// k_scan.hip: the scan step of the live-track exports below -- two count arrays to offsets, totals and the capacity decision
void launch_pair_scan(int S, int32_t *off, int32_t *totals, int cap0, int cap1, hipStream_t st);
// ... and the generation bump of those that remember uids (report, zones, trails, tripwires, stance, heat): every non-null word, for the scenes flagged
// (flags: dev [S] or nullptr = every scene)
struct UidGens { static constexpr int kMax = 5; int32_t *gen[kMax]; };
void launch_uid_rebase(int n_scenes, const int32_t *flags, const UidGens &gens, hipStream_t st);
// k_report.hip: the live-track report
void launch_report_baseline(const DevCfg &cfg, const DevState &s, const ReportState &rp, hipStream_t st);
void launch_report(const DevCfg &cfg, const mmw_scene_site *sites, const DevState &s, const ReportState &rp, mmw_track_report *rows, int cap_rows, mmw_track_event *events, int cap_events, int scene_base, hipStream_t st);
// k_cloud.hip: the live tracks' point clouds (mode: MMW_CLOUD_POINTS / MMW_CLOUD_ROWS, | MMW_CLOUD_UNASSIGNED)
void launch_clouds(const DevCfg &cfg, const DevState &s, const ExportScratch &sc, mmw_cloud_track *dir, int cap_tracks, void *out, int cap_points, int mode, int scene_base, hipStream_t st);
// k_skeleton.hip: the live tracks' room-frame skeletons (mode: MMW_SKEL_ALL / MMW_SKEL_DRAWN)
void launch_skeletons(const DevCfg &cfg, const DevState &s, const ExportScratch &sc, mmw_skeleton *out, int cap, int mode, int scene_base, hipStream_t st);
// k_zone.hip: zone occupancy
void launch_zones(const DevCfg &cfg, const DevState &s, const ZoneState &zs, mmw_zone_row *rows, int cap_rows, mmw_zone_event *events, int cap_events, int scene_base, hipStream_t st);
// k_trail.hip: track trails (flags: dev [S] or nullptr = every scene; t: dev [S] or nullptr = the scenes' call ordinals)
void launch_trail_sample(const DevCfg &cfg, const DevState &s, const TrailState &ts, const int32_t *flags, const double *t, hipStream_t st);
void launch_trails(const DevCfg &cfg, const DevState &s, const TrailState &ts, mmw_trail_track *dir, int cap_tracks, mmw_trail_point *points, int cap_points, int max_per_track, int scene_base, hipStream_t st);
// k_tripwire.hip: tripwires (flags, t as launch_trail_sample's; launch_tripwire_zero: the flagged scenes' counters and marks, flags: dev [S])
void launch_tripwire_zero(int n_scenes, const int32_t *flags, const TripState &ts, hipStream_t st);
void launch_tripwire_sample(const DevCfg &cfg, const DevState &s, const TripState &ts, const int32_t *flags, const double *t, hipStream_t st);
void launch_tripwires(const DevCfg &cfg, const TripState &ts, mmw_tripwire_row *rows, int cap_rows, mmw_tripwire_event *events, int cap_events, int scene_base, hipStream_t st);
// k_stance.hip: the stance watch (flags, t as launch_trail_sample's; launch_stance_zero: the flagged scenes' counters and marks, flags: dev [S])
void launch_stance_zero(int n_scenes, const int32_t *flags, const StanceState &ss, hipStream_t st);
void launch_stance_sample(const DevCfg &cfg, const DevState &s, const StanceState &ss, const int32_t *flags, const double *t, hipStream_t st);
void launch_stance(const DevCfg &cfg, const StanceState &ss, mmw_stance_row *rows, int cap_rows, mmw_stance_event *events, int cap_events, int scene_base, hipStream_t st);
// k_heat.hip: the dwell heat maps (flags, t as launch_trail_sample's; launch_heat_zero: the flagged scenes' cells and scene words, flags: dev [S];
// launch_heat: scene_flags dev [S] or nullptr = every scene, mode MMW_HEAT_KEEP / MMW_HEAT_CLEAR)
void launch_heat_zero(int n_scenes, const int32_t *flags, const HeatState &hs, hipStream_t st);
void launch_heat_sample(const DevCfg &cfg, const DevState &s, const HeatState &hs, const int32_t *flags, const double *t, hipStream_t st);
void launch_heat(const DevCfg &cfg, const HeatState &hs, mmw_heat_row *rows, int cap_rows, mmw_heat_cell *cells, int cap_cells, const int32_t *scene_flags, int mode, int scene_base, hipStream_t st);
// k_uart.hip: the device-resident radar readers (log: the radar log while it is enabled -- k_uart_read's LOG = true instantiations --, else nullptr)
void launch_uart_read(const DevCfg &cfg, const mmw_scene_site *sites, const UartState &us, const UartLog *log, const uint8_t *chunks, const long long *chunk_off, long long chunks_bytes, const int32_t *flags, double now, double *out, int32_t *n_out, double *dt_out, int32_t *status, uint32_t *frame_number, hipStream_t st);
void launch_uart_set_time(const DevCfg &cfg, const UartState &us, const int32_t *flags, double t, hipStream_t st);
// k_uart_log.hip: the radar log's export (scene_flags: dev [S] or nullptr = every scene)
void launch_uart_log(const DevCfg &cfg, const UartState &us, const UartLog &log, const ExportScratch &sc, mmw_uart_frame *dir, int cap_frames, mmw_uart_object *rows, int cap_rows, const int32_t *scene_flags, int frame_select, int scene_base, hipStream_t st);
// k_sample.hip: the training samples (mode: MMW_SAMPLE_BLOCK / MMW_SAMPLE_INPUT, | MMW_SAMPLE_ABSOLUTE; sites as k_features'; scene_flags: dev [S] or nullptr)
void launch_samples(const DevCfg &cfg, const mmw_scene_site *sites, const DevState &s, const ExportScratch &sc, mmw_sample_entry *dir, int cap_samples, void *out, int mode, const int32_t *scene_flags, int scene_base, hipStream_t st);
// k_mars.hip, k_dense.hip, k_dense2.hip: the posture CNN
void launch_mars_conv(const float *feat, const float *w1, const float *b1, const float *w2, const float *b2, float *out, int B, hipStream_t stream, const int32_t *dev_rows = nullptr);
// k_mars2d.hip: the Conv2D pair of the single-frame model (define_CNN) in fp32; dev_rows as launch_mars_conv's
void launch_mars_conv2d(const float *feat, const float *w1, const float *b1, const float *w2, const float *b2, float *out, int B, hipStream_t stream, const int32_t *dev_rows = nullptr);
// ... and the fp32 conv pair of either model: launch_mars_conv for frames = 3, launch_mars_conv2d for frames = 1
void launch_mars_conv_f32(int frames, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2, float *out, int B, hipStream_t stream, const int32_t *dev_rows = nullptr);
void launch_range_gather(const float *feat, int32_t *list, int n, int per, int cap, float *small, int32_t *range_flag, hipStream_t stream);
void launch_range_scatter(const float *kp_small, const int32_t *list, float *kp, int cap, int nout, int n, hipStream_t stream);
// Dense-1's tile plan (k_dense.hip): bands of 256 rows per instantiation -- 256 x 192 tiles, 256 x 128 tiles, 128 x 128 half tiles
struct Dense1Plan { int bands192, bands128, bands_half; };
Dense1Plan mars_dense1_plan(int rows_padded, int N, int n_cu);
int mars_dense1_cus(int dev);
int launch_mars_dense1(const void *a2, long long lda, const void *w2, long long ldw, const float *bias, float *out, int rows_padded, int K, int N, hipStream_t stream);
int launch_mars_head_small(const float *act, long long lda, const float *w1, long long ldw, const float *bias1, const float *w2, const float *bias2, float *hidden, float *kp, int n_rows, int K, int N1, int NOUT, hipStream_t stream, const int32_t *dev_rows = nullptr);
int launch_mars_conv16(int nz, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2, void *out16, long long ld_out, int B, int32_t *range_flag, int32_t *sample_flags, hipStream_t stream);
void launch_mars_dense2(const float *hidden, long long ldh, const float *w2, const float *bias2, float *kp, int n_rows, int K, hipStream_t stream);
void launch_split_weights(const float *w, long long ldw, void *w16, long long ld16, int n, int k, int32_t *range_flag, hipStream_t stream);
void launch_range_check(const float *a, long long count, int32_t *range_flag, hipStream_t stream);
// k_snapshot.hip
void launch_snap_size(const DevCfg &cfg, const DevState &st, const int32_t *sel, int n, mmw_snapshot_entry *dir, unsigned long long *bytes, unsigned long long base, hipStream_t stream);
void launch_snap_pack(const DevCfg &cfg, const DevState &st, const int32_t *sel, int n, const mmw_snapshot_entry *dir, char *blob, int max_tracks, hipStream_t stream);
void launch_snap_check(const DevCfg &cfg, const char *blob, const mmw_snapshot_entry *dir, int n, int src_ring_rows, int32_t *bad, hipStream_t stream);
void launch_snap_restore(const DevCfg &cfg, const DevState &st, const char *blob, const mmw_snapshot_entry *dir, const int32_t *dst, const int32_t *flags, int n, int max_tracks, int src_ring_rows, int32_t *kp_gen, hipStream_t stream);
}  // namespace mmw
