"""ctypes binding of libmmw_hip.so (C-ABI declared in include/mmw.h).

There is deliberately no fallback: if the HIP library is missing or cannot be
loaded, importing the compute path raises.  `build()` compiles it in-tree with
hipcc for gfx950 (no GPU needed to compile).

This module is the one Python mirror of the header, in three tables that tests/test_abi.py holds to it:
  constants    every integer `#define MMW_X` is the module attribute `X` -- the `MMW_` prefix dropped (`MMW_OK` alone keeps it);
  ABI_STRUCTS  C struct name -> its one Python definition: a numpy dtype for the structs the library fills arrays of, a
               ctypes.Structure for those Python builds one value of and passes by pointer;
  sig          entry name -> (restype, argtypes); `EXPORTS` is its key list.
A new entry family adds its rows to all three.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("MMW_LIB_NAME", "libmmw_hip.so"))  # MMW_LIB_NAME: diagnostic builds only
CSRC = os.path.join(_HERE, "csrc")
RING_MAX = 4
NKP = 57
MAX_PTS_LIMIT, TRACK_CAP_LIMIT = 1024, 64   # the largest max_pts / track_cap of mmw_create

MMW_OK = 0
E_ARG, E_SINGULAR, E_DIVZERO, E_CAPACITY, E_HIP, E_NODEVICE, E_NONFINITE = -1, -2, -3, -4, -5, -6, -7
DB_RAISED = -2     # MMW_DB_RAISED: db_n of a scene whose apply_DBscan call of the frame raised (E_NONFINITE)
ERRBIT_SINGULAR, ERRBIT_DIVZERO, ERRBIT_CAPACITY, ERRBIT_BADCOUNT, ERRBIT_NONFINITE_NAN, ERRBIT_NONFINITE_INF = 1, 2, 4, 8, 16, 32
K_TRACK, K_DBSCAN, K_FEATURES, K_NORMALIZE, K_TABLE, K_PREDICT, K_POST, K_COUNT = range(8)
RANGE_FIXUP_CAP = 64               # out-of-range samples one call of the posture chain repairs in fp32
RANGE_FIXUP_SCRATCH = 2226944      # bytes of device scratch mmw_mars_range_fixup* takes (the header's expression, evaluated)
POSTURE_MODELS_MAX = 8             # models one mmw_posture_attach_models call takes
POSTURE_NONE = -1                  # MMW_POSTURE_NONE: the map entry of a scene no model estimates
EXPORT_TICKETS = 4                 # kTickets (csrc/mmw_ctx.hpp): `*_async` calls of one export that may be outstanding; the
                                   # one-call form of each export (mmw_report, mmw_clouds, ...) uses the last ticket itself
REPORT_TICKETS = CLOUD_TICKETS = SKEL_TICKETS = ZONE_TICKETS = TRAIL_TICKETS = TRIPWIRE_TICKETS = STANCE_TICKETS = HEAT_TICKETS = UART_LOG_TICKETS = SAMPLE_TICKETS = EXPORT_TICKETS   # (the names callers know)

EMPTY_FRAME = -1   # MMW_EMPTY_FRAME (include/mmw.h)
BAD_FRAME = -3     # MMW_BAD_FRAME: n_out of mmw_normalize_tlv for a TLV body it refused to decode
UART_NONE, UART_POINTS, UART_PACKET = 0, 1, 2   # MMW_UART_*: what mmw_parse_uart_cap found
UART_OVERFLOW, UART_RAISED, UART_SKIPPED, UART_BADCHUNK = 3, 4, 5, 6   # ... and the other outcomes of mmw_uart_read (status, low byte)
UART_CHUNK_DROPPED = 256                        # MMW_UART_CHUNK_DROPPED: bit 8 of that status
UART_BUFFER = 32768                             # MMW_UART_BUFFER: the reference's maxBufferSize


class MmwPostureModel(C.Structure):
    """struct mmw_posture_model (include/mmw.h): device pointers of define_CNN_3D's (or, for the *_frames entries with frames = 1,
    define_CNN's) weights, BatchNormalization folded."""
    _fields_ = [("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p),
                ("dense1_w", C.c_void_p), ("dense1_ld", C.c_int64), ("dense1_b", C.c_void_p), ("dense2_w", C.c_void_p),
                ("dense2_b", C.c_void_p)]

    @classmethod
    def of(cls, conv1_w, conv1_b, conv2_w, conv2_b, dense1_w, dense1_b, dense2_w, dense2_b, dense1_ld):
        """From the eight device pointers (weight, bias of each layer in turn) and Dense-1's leading dimension in floats."""
        return cls(conv1_w, conv1_b, conv2_w, conv2_b, dense1_w, dense1_ld, dense1_b, dense2_w, dense2_b)


class MmwUartCfg(C.Structure):
    """struct mmw_uart_cfg (include/mmw.h): the scales ReadIWR14xx.__parseConfigFile derives from the radar .cfg."""
    _fields_ = [("range_idx_to_meters", C.c_double), ("doppler_resolution_mps", C.c_double),
                ("num_doppler_bins", C.c_int32), ("reserved", C.c_int32)]


class MmwConfig(C.Structure):
    """struct mmw_config (include/mmw.h) -- mirrors the reference constants.py."""
    _fields_ = [
        ("fb_frames_batch", C.c_int32), ("db_min_samples", C.c_int32), ("tr_max_tracks", C.c_int32),
        ("kf_enable_est", C.c_int32), ("model_min_input", C.c_int32), ("dim_x", C.c_int32),
        ("ring_rows", C.c_int32), ("track_cap", C.c_int32),
        ("db_z_weight", C.c_double), ("db_range_weight", C.c_double), ("db_eps", C.c_double),
        ("tr_lifetime_dynamic", C.c_double), ("tr_lifetime_static", C.c_double), ("tr_vel_thres", C.c_double),
        ("tr_gate", C.c_double), ("kf_q_std", C.c_double), ("kf_p_init", C.c_double),
        ("kf_group_disp_est_init", C.c_double), ("kf_a_n", C.c_double), ("kf_est_pointnum", C.c_double),
        ("kf_spread_lim", C.c_double * 6), ("kf_a_spr", C.c_double), ("intensity_mu", C.c_double),
        ("intensity_std", C.c_double), ("s_height", C.c_double), ("tilt_cos", C.c_double), ("tilt_sin", C.c_double),
        ("default_posture", C.c_float * NKP),
        ("kalman_dense_min_units", C.c_int32), ("seek_inner", C.c_int32), ("db_points_thres", C.c_int32),
        ("fb_frames_batch_static", C.c_int32), ("chain_side_stream", C.c_int32),
        ("db_spread_thres", C.c_double), ("db_inner_eps", C.c_double),
        ("m_x", C.c_double), ("m_y", C.c_double), ("m_z", C.c_double),
        ("v_screen_fade_size_max", C.c_double), ("v_screen_fade_size_min", C.c_double), ("v_screen_fade_weight", C.c_double),
        ("fused_step", C.c_int32), ("reserved_", C.c_int32),
    ]


SITE_FIELDS = ("s_height", "tilt_cos", "tilt_sin", "intensity_mu", "intensity_std", "m_x", "m_y", "m_z",
               "v_screen_fade_size_max", "v_screen_fade_size_min", "v_screen_fade_weight")
# struct mmw_scene_site (include/mmw.h): the eleven values of mmw_config that describe a scene's installation -- sensor mounting,
# intensity scale, window / monitoring point -- and one reserved double that must be 0
SITE_DTYPE = np.dtype([(f, "f8") for f in SITE_FIELDS] + [("reserved_", "f8")], align=True)   # 12 x f8 = 96 bytes

SNAP_MAGIC = b"MMWSNAP"   # MMW_SNAP_MAGIC (8 bytes with the terminating 0)
SNAP_VERSION = 1
SNAP_SCENE_HDR_BYTES = 64
SNAP_TRACK_BYTES = 1504


class MmwSnapshotHeader(C.Structure):
    """struct mmw_snapshot_header (include/mmw.h): the head of a scene snapshot."""
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("total_bytes", C.c_uint64),
                ("n_scenes", C.c_int32), ("entry_bytes", C.c_int32), ("max_pts", C.c_int32), ("ring", C.c_int32),
                ("ring_rows", C.c_int32), ("dim_x", C.c_int32), ("track_cap", C.c_int32), ("reserved_", C.c_int32),
                ("config", MmwConfig)]


class MmwSnapshotEntry(C.Structure):
    """struct mmw_snapshot_entry (include/mmw.h): one scene of a snapshot's directory."""
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64), ("n_tracks", C.c_int32), ("g_len", C.c_int32),
                ("max_g_rows", C.c_int32), ("max_trk_rows", C.c_int32), ("err", C.c_int32), ("ring_size", C.c_int32),
                ("reserved_", C.c_int32 * 2)]


class MmwSnapshotInfo(C.Structure):
    """struct mmw_snapshot_info (include/mmw.h): what mmw_snapshot_inspect fills in."""
    _fields_ = [("header", MmwSnapshotHeader), ("entries", C.c_void_p)]


TRACK_DTYPE = np.dtype(
    [
        ("x", "f8", (9,)), ("P", "f8", (9, 9)), ("centroid", "f8", (6,)), ("min_vals", "f8", (6,)),
        ("max_vals", "f8", (6,)), ("spread_est", "f8", (6,)), ("group_disp_est", "f8", (6, 6)),
        ("n_est", "f8"), ("lifetime", "f8"), ("point_num", "i4"), ("is_static", "i4"), ("ring_len", "i4"),
        ("ring_n", "i4", (RING_MAX,)), ("uid", "i4"), ("keypoints", "f4", (NKP,)),
    ],
    align=True,
)
SUMMARY_DTYPE = np.dtype(
    [("scene", "i4"), ("slot", "i4"), ("alive", "i4"), ("is_static", "i4"), ("point_num", "i4"),
     ("lifetime", "f4"), ("x", "f4", (9,)), ("centroid", "f4", (6,)), ("keypoints", "f4", (NKP,)),
     ("fade_x", "f4"), ("fade_z", "f4"), ("fade_size", "f4")],
    align=True,
)
# struct mmw_track_report / mmw_track_event (include/mmw.h): the live-track report's rows (324 bytes, no padding) and events
TRACK_REPORT_DTYPE = np.dtype(
    [("scene", "i4"), ("slot", "i4"), ("uid", "i4"), ("flags", "i4"), ("point_num", "i4"), ("lifetime", "f4"),
     ("x", "f4", (9,)), ("centroid", "f4", (6,)), ("fade_x", "f4"), ("fade_z", "f4"), ("fade_size", "f4"),
     ("keypoints", "f4", (NKP,))],
    align=True,
)
TRACK_EVENT_DTYPE = np.dtype([("scene", "i4"), ("uid", "i4"), ("kind", "i4"), ("slot", "i4")], align=True)
REPORT_STATIC, REPORT_BORN = 1, 2             # MMW_REPORT_*: bits of mmw_track_report.flags
EV_BORN, EV_GONE, EV_REBASED = 1, 2, 3        # MMW_EV_*: mmw_track_event.kind

# struct mmw_cloud_track / mmw_cloud_point (include/mmw.h): the directory entries (32 bytes) and points (16 bytes) of mmw_clouds_*
CLOUD_TRACK_DTYPE = np.dtype([("scene", "i4"), ("slot", "i4"), ("uid", "i4"), ("first", "i4"), ("count", "i4"), ("frames", "i4"),
                              ("newest", "i4"), ("dropped", "i4")], align=True)
CLOUD_POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("track", "i4")], align=True)
CLOUD_POINTS, CLOUD_ROWS, CLOUD_UNASSIGNED = 0, 1, 2   # MMW_CLOUD_*: the mode of mmw_clouds_* (UNASSIGNED is a flag bit)

# struct mmw_uart_frame / mmw_uart_object (include/mmw.h): the directory entries (32 bytes) and detObj rows (48 bytes) of mmw_uart_log_*
UART_FRAME_DTYPE = np.dtype([("scene", "i4"), ("frame_number", "u4"), ("first", "i4"), ("count", "i4"), ("t", "f8"), ("q_format", "i4"),
                             ("reserved_", "i4")], align=True)
UART_OBJECT_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("z", "f8"), ("doppler", "f8"), ("peak_val", "f8"), ("range", "f8")], align=True)

# struct mmw_sample_entry (include/mmw.h): the directory entries (48 bytes, no padding) of mmw_samples_*
SAMPLE_ENTRY_DTYPE = np.dtype([("scene", "i4"), ("uid", "i4"), ("frames", "i4"), ("reserved", "i4"), ("rows", "i4", (3,)), ("cut", "i4"),
                               ("centroid", "f8", (2,))], align=True)
SAMPLE_BLOCK, SAMPLE_INPUT, SAMPLE_ABSOLUTE = 0, 1, 2   # MMW_SAMPLE_*: the mode of mmw_samples_* (ABSOLUTE is a flag bit)
SAMPLE_BLOCK_SHAPE, SAMPLE_INPUT_SHAPE = (192, 5), (8, 8, 5)   # float64 / float32 per sample

# struct mmw_skeleton (include/mmw.h): one live track's room-frame skeleton of mmw_skeletons_* (256 bytes, no padding)
SKEL_JOINTS, SKEL_BONES = 19, 18
SKELETON_DTYPE = np.dtype([("scene", "i4"), ("slot", "i4"), ("uid", "i4"), ("row", "i4"), ("flags", "i4"), ("gap", "f4"),
                           ("joint", "f4", (SKEL_JOINTS, 3)), ("reserved_", "i4")], align=True)
SKEL_SKIPPED = 1                              # MMW_SKEL_SKIPPED: bit 0 of mmw_skeleton.flags
SKEL_ALL, SKEL_DRAWN = 0, 1                   # MMW_SKEL_*: the mode of mmw_skeletons_*
SKEL_CLASS_NAMES = ("blue", "green", "red")   # mmw_skeleton_tables' joint classes as the reference's colour names

# struct mmw_zone / mmw_zone_row / mmw_zone_event (include/mmw.h): a scene's zones (48 bytes each), and the rows (32 bytes) and
# events (24 bytes) of mmw_zones_*
ZONES_MAX = 16                                # MMW_ZONES_MAX: zones per scene
ZONE_FIELDS = ("x0", "x1", "y0", "y1", "margin", "id")
ZONE_DTYPE = np.dtype([("x0", "f8"), ("x1", "f8"), ("y0", "f8"), ("y1", "f8"), ("margin", "f8"), ("id", "i4"), ("reserved_", "i4")], align=True)
ZONE_ROW_DTYPE = np.dtype([("scene", "i4"), ("zone", "i4"), ("id", "i4"), ("count", "i4"), ("count_static", "i4"), ("entered", "i4"),
                           ("left", "i4"), ("reserved_", "i4")], align=True)
ZONE_EVENT_DTYPE = np.dtype([("scene", "i4"), ("uid", "i4"), ("kind", "i4"), ("zone", "i4"), ("id", "i4"), ("slot", "i4")], align=True)
ZEV_ENTER, ZEV_LEAVE, ZEV_REBASED = 1, 2, 3   # MMW_ZEV_*: mmw_zone_event.kind

# struct mmw_trail_track / mmw_trail_point (include/mmw.h): the directory entries (40 bytes) and points (24 bytes) of mmw_trails_*
TRAIL_DEPTH_MAX = 256                         # MMW_TRAIL_DEPTH_MAX: samples a trail's ring holds at the most
TRAIL_STATIC, TRAIL_UPDATED = 1, 2            # MMW_TRAIL_*: bits of mmw_trail_point.flags
TRAIL_TRACK_DTYPE = np.dtype([("scene", "i4"), ("slot", "i4"), ("uid", "i4"), ("first", "i4"), ("count", "i4"), ("total", "i4"),
                              ("t_first", "f8"), ("travelled", "f8")], align=True)
TRAIL_POINT_DTYPE = np.dtype([("t", "f8"), ("x", "f4"), ("y", "f4"), ("z", "f4"), ("flags", "i4")], align=True)

# struct mmw_tripwire / mmw_tripwire_row / mmw_tripwire_event (include/mmw.h): a scene's wires (48 bytes each), and the rows (32 bytes)
# and events (32 bytes) of mmw_tripwires_*
TRIPWIRES_MAX = 16                            # MMW_TRIPWIRES_MAX: wires per scene
TRIPWIRE_LOG_MAX = 4096                       # MMW_TRIPWIRE_LOG_MAX: events a scene's log holds at the most
TRIPWIRE_FIELDS = ("ax", "ay", "bx", "by", "margin", "id")
TRIPWIRE_DTYPE = np.dtype([("ax", "f8"), ("ay", "f8"), ("bx", "f8"), ("by", "f8"), ("margin", "f8"), ("id", "i4"), ("reserved_", "i4")], align=True)
TRIPWIRE_ROW_DTYPE = np.dtype([("scene", "i4"), ("wire", "i4"), ("id", "i4"), ("forward", "i4"), ("backward", "i4"), ("d_forward", "i4"),
                               ("d_backward", "i4"), ("lost", "i4")], align=True)
TRIPWIRE_EVENT_DTYPE = np.dtype([("scene", "i4"), ("uid", "i4"), ("kind", "i4"), ("wire", "i4"), ("id", "i4"), ("slot", "i4"), ("t", "f8")], align=True)
TW_FORWARD, TW_BACKWARD, TW_REBASED = 1, 2, 3   # MMW_TW_*: mmw_tripwire_event.kind

# struct mmw_stance_rule / mmw_stance_row / mmw_stance_event (include/mmw.h): a scene's rule (64 bytes), and the rows (48 bytes) and
# events (32 bytes) of mmw_stance_*
STANCE_RULES_MAX = 1                          # MMW_STANCE_RULES_MAX: rules per scene
STANCE_LOG_MAX = 4096                         # MMW_STANCE_LOG_MAX: events a scene's log holds at the most
STANCE_UNKNOWN, STANCE_UPRIGHT, STANCE_LOW, STANCE_LYING = 0, 1, 2, 3   # MMW_STANCE_*: the classes (mmw_stance_event.from / .to)
STANCE_CLASS_NAMES = ("unknown", "upright", "low", "lying")
STANCE_FIELDS = ("h_stand", "h_lie", "margin", "fall_window", "long_lie", "max_gap", "id")
STANCE_DEFAULTS = dict(h_stand=1.2, h_lie=0.5, margin=0.1, fall_window=1.5, long_lie=30.0, max_gap=0.5, id=0)
STANCE_RULE_DTYPE = np.dtype([("h_stand", "f8"), ("h_lie", "f8"), ("margin", "f8"), ("fall_window", "f8"), ("long_lie", "f8"), ("max_gap", "f8"),
                              ("id", "i4"), ("reserved_", "i4"), ("pad_", "i4", (2,))], align=True)
STANCE_ROW_DTYPE = np.dtype([("scene", "i4"), ("id", "i4"), ("upright", "i4"), ("low", "i4"), ("lying", "i4"), ("unknown", "i4"), ("falls", "i4"),
                             ("d_falls", "i4"), ("long_lies", "i4"), ("d_long_lies", "i4"), ("lost", "i4"), ("reserved_", "i4")], align=True)
STANCE_EVENT_DTYPE = np.dtype([("scene", "i4"), ("uid", "i4"), ("kind", "i4"), ("from", "i4"), ("to", "i4"), ("slot", "i4"), ("t", "f8")], align=True)
SEV_CHANGE, SEV_FALL, SEV_LONG_LIE, SEV_REBASED = 1, 2, 3, 4   # MMW_SEV_*: mmw_stance_event.kind

# struct mmw_heat_grid / mmw_heat_row / mmw_heat_cell (include/mmw.h): a scene's grid (48 bytes), and the rows (48 bytes) and cells
# (24 bytes) of mmw_heat_*
HEAT_CELLS_MAX = 4096                         # MMW_HEAT_CELLS_MAX: cells a scene's grid has at the most
HEAT_GRIDS_MAX = 1                            # MMW_HEAT_GRIDS_MAX: grids per scene
HEAT_KEEP, HEAT_CLEAR = 0, 1                  # MMW_HEAT_*: the mode of mmw_heat_*
HEAT_FIELDS = ("x0", "y0", "cell", "max_gap", "nx", "ny", "id")
HEAT_GRID_DTYPE = np.dtype([("x0", "f8"), ("y0", "f8"), ("cell", "f8"), ("max_gap", "f8"), ("nx", "i4"), ("ny", "i4"), ("id", "i4"),
                            ("reserved_", "i4")], align=True)
HEAT_ROW_DTYPE = np.dtype([("scene", "i4"), ("id", "i4"), ("nx", "i4"), ("ny", "i4"), ("first", "i4"), ("count", "i4"), ("calls", "i4"),
                           ("outside", "i4"), ("t_first", "f8"), ("t_last", "f8")], align=True)
HEAT_CELL_DTYPE = np.dtype([("scene", "i4"), ("cell", "i4"), ("samples", "i4"), ("visits", "i4"), ("dwell", "f8")], align=True)


# C struct name in include/mmw.h -> its Python mirror; every `typedef struct mmw_*` but the opaque mmw_ctx.  Field names are the
# header's own throughout, so a mirror needs no second spelling beside it.
ABI_STRUCTS = {
    "mmw_config": MmwConfig, "mmw_track_record": TRACK_DTYPE, "mmw_track_summary": SUMMARY_DTYPE, "mmw_scene_site": SITE_DTYPE,
    "mmw_posture_model": MmwPostureModel, "mmw_track_report": TRACK_REPORT_DTYPE, "mmw_track_event": TRACK_EVENT_DTYPE,
    "mmw_cloud_track": CLOUD_TRACK_DTYPE, "mmw_cloud_point": CLOUD_POINT_DTYPE, "mmw_skeleton": SKELETON_DTYPE,
    "mmw_zone": ZONE_DTYPE, "mmw_zone_row": ZONE_ROW_DTYPE, "mmw_zone_event": ZONE_EVENT_DTYPE,
    "mmw_trail_track": TRAIL_TRACK_DTYPE, "mmw_trail_point": TRAIL_POINT_DTYPE,
    "mmw_tripwire": TRIPWIRE_DTYPE, "mmw_tripwire_row": TRIPWIRE_ROW_DTYPE, "mmw_tripwire_event": TRIPWIRE_EVENT_DTYPE,
    "mmw_stance_rule": STANCE_RULE_DTYPE, "mmw_stance_row": STANCE_ROW_DTYPE, "mmw_stance_event": STANCE_EVENT_DTYPE,
    "mmw_heat_grid": HEAT_GRID_DTYPE, "mmw_heat_row": HEAT_ROW_DTYPE, "mmw_heat_cell": HEAT_CELL_DTYPE,
    "mmw_snapshot_header": MmwSnapshotHeader, "mmw_snapshot_entry": MmwSnapshotEntry, "mmw_snapshot_info": MmwSnapshotInfo,
    "mmw_uart_cfg": MmwUartCfg, "mmw_uart_frame": UART_FRAME_DTYPE, "mmw_uart_object": UART_OBJECT_DTYPE,
    "mmw_sample_entry": SAMPLE_ENTRY_DTYPE,
}


def _signatures():
    """Entry name -> (restype, argtypes) of every function include/mmw.h declares."""
    vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
    i32, i32p, i64p = C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    f64p = C.POINTER(C.c_double)
    cfgp = C.POINTER(MmwConfig)
    return {
        "mmw_config_default": (C.c_int, [cfgp]),
        "mmw_create": (C.c_int, [cfgp, i32, i32, i32, vpp]),
        "mmw_destroy": (C.c_int, [vp]),
        "mmw_last_error": (C.c_char_p, [vp]),
        "mmw_reset": (C.c_int, [vp]),
        "mmw_set_stream": (C.c_int, [vp, vp]),
        "mmw_pop_frame": (C.c_int, [vp, vp]),
        "mmw_synchronize": (C.c_int, [vp]),
        "mmw_stream_wait": (C.c_int, [vp, vp]),
        "mmw_wait_stream": (C.c_int, [vp, vp]),
        "mmw_get_dims": (C.c_int, [vp, i32p, i32p, i32p, i32p, i32p]),
        "mmw_dev_alloc": (C.c_int, [vp, C.c_size_t, vpp]),
        "mmw_dev_free": (C.c_int, [vp, vp]),
        "mmw_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "mmw_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "mmw_normalize": (C.c_int, [vp, vp, vp, vp, vp]),
        "mmw_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "mmw_step_host": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "mmw_step_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "mmw_frame_host": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mmw_frame_posture_host": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mmw_attach_posture": (C.c_int, [vp, vp]),
        "mmw_normalize_f32": (C.c_int, [vp, vp, vp, vp, vp]),
        "mmw_dbscan": (C.c_int, [vp, vp, vp, i32, C.c_double, i32, vp, vp]),
        "mmw_features": (C.c_int, [vp, vp, vp, i32, i32p]),
        "mmw_set_keypoints": (C.c_int, [vp, vp, vp, i32]),
        "mmw_features_async": (C.c_int, [vp, vp, vp, vp, i32, i32]),
        "mmw_features_wait": (C.c_int, [vp, i32, i32p]),
        "mmw_set_keypoints_uid": (C.c_int, [vp, vp, vp, vp, i32]),
        "mmw_set_keypoints_ticket": (C.c_int, [vp, vp, vp, vp, i32, i32]),
        "mmw_get_inner": (C.c_int, [vp, vp, vp, vp, i32]),
        "mmw_set_batch_size": (C.c_int, [vp, vp, i32]),
        "mmw_set_batch_frame": (C.c_int, [vp, i32, vp, i32]),
        "mmw_check": (C.c_int, [vp]),
        "mmw_get_num_tracks": (C.c_int, [vp, vp]),
        "mmw_get_tracks": (C.c_int, [vp, vp, i32]),
        "mmw_get_batch_ring": (C.c_int, [vp, vp, vp]),
        "mmw_get_track_ring_frame": (C.c_int, [vp, i32, i32, i32, vp, i32p]),
        "mmw_get_batch_ring_frame": (C.c_int, [vp, i32, i32, vp, i32p]),
        "mmw_track_table": (C.c_int, [vp, vp, i32, i32]),
        "mmw_profile_enable": (C.c_int, [vp, i32]),
        "mmw_profile_reset": (C.c_int, [vp]),
        "mmw_profile_get": (C.c_int, [vp, i32, f64p, i64p]),
        "mmw_kernel_name": (C.c_char_p, [i32]),
        "mmw_version": (C.c_char_p, []),
        "mmw_stats_get": (C.c_int, [vp, vp]),
        "mmw_stats_reset": (C.c_int, [vp]),
        "mmw_diag_queue": (C.c_int, [vp, vp]),
        "mmw_side_workers": (C.c_int, [vp]),
        "mmw_step_kind": (C.c_int, [vp]),
        "mmw_kalman_layout": (C.c_int, [vp]),
        "mmw_streams_concurrent": (C.c_int, [vp, vp, vp]),
        "mmw_reset_scenes": (C.c_int, [vp, vp]),
        "mmw_get_errors": (C.c_int, [vp, vp]),
        "mmw_clear_errors": (C.c_int, [vp, vp, i32]),
        "mmw_set_chain_side_stream": (C.c_int, [vp, i32]),
        "mmw_stats_get_ext": (C.c_int, [vp, vp]),
        "mmw_mars_conv3d": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32]),
        "mmw_mars_conv_split": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, C.c_int64, i32, vp, vp]),
        "mmw_mars_range_fixup": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]),
        "mmw_mars_dense1_split": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, vp, vp, i32, i32, i32]),
        "mmw_mars_dense1_plan": (C.c_int, [i32, i32, vp]),
        "mmw_mars_head_small": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp, i32, i32, i32]),
        "mmw_parse_uart": (C.c_int, [vp, C.c_size_t, vp, vp, vp, i32, vp, vp, vp, vp]),
        "mmw_parse_uart_cap": (C.c_int, [vp, C.c_size_t, C.c_size_t, vp, vp, vp, i32, vp, vp, vp, vp]),
        "mmw_find_tlv": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp]),
        "mmw_normalize_tlv": (C.c_int, [vp, vp, C.c_size_t, vp, vp, vp, vp]),
        "mmw_format_frames": (C.c_int, [vp, vp, vp, vp, vp, i32]),
        "mmw_snapshot_size": (C.c_int, [vp, vp, i32, C.POINTER(C.c_size_t)]),
        "mmw_snapshot": (C.c_int, [vp, vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "mmw_restore": (C.c_int, [vp, vp, C.c_size_t, vp, i32]),
        "mmw_snapshot_inspect": (C.c_int, [vp, C.c_size_t, C.POINTER(MmwSnapshotInfo)]),
        "mmw_set_sites": (C.c_int, [vp, vp, i32, vp]),
        "mmw_get_sites": (C.c_int, [vp, vp]),
        "mmw_clear_sites": (C.c_int, [vp]),
        "mmw_has_sites": (C.c_int, [vp]),
        "mmw_posture_attach": (C.c_int, [vp, vp, i32]),
        "mmw_estimate_posture": (C.c_int, [vp, i32p]),
        "mmw_posture_range": (C.c_int, [vp, i32p]),
        "mmw_mars_dense2": (C.c_int, [vp, vp, C.c_int64, vp, vp, vp, i32, i32]),
        "mmw_mars_split_weights": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, i32, i32, vp]),
        "mmw_report_enable": (C.c_int, [vp, i32]),
        "mmw_report_async": (C.c_int, [vp, vp, i32, vp, i32, i32, i32]),
        "mmw_report_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_report": (C.c_int, [vp, vp, i32, vp, i32, i32, i32p, i32p]),
        "mmw_clouds_async": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32]),
        "mmw_clouds_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_clouds": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32p, i32p]),
        "mmw_skeletons_async": (C.c_int, [vp, vp, i32, i32, i32, i32]),
        "mmw_skeletons_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_skeletons": (C.c_int, [vp, vp, i32, i32, i32, i32p, i32p]),
        "mmw_skeleton_tables": (C.c_int, [C.POINTER(i32p), C.POINTER(i32p)]),
        "mmw_set_zones": (C.c_int, [vp, vp, i32, vp, vp]),
        "mmw_get_zones": (C.c_int, [vp, vp, vp]),
        "mmw_clear_zones": (C.c_int, [vp]),
        "mmw_has_zones": (C.c_int, [vp]),
        "mmw_zones_async": (C.c_int, [vp, vp, i32, vp, i32, i32, i32]),
        "mmw_zones_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_zones": (C.c_int, [vp, vp, i32, vp, i32, i32, i32p, i32p]),
        "mmw_trails_enable": (C.c_int, [vp, i32]),
        "mmw_trails_sample": (C.c_int, [vp, vp, vp]),
        "mmw_trails_async": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32]),
        "mmw_trails_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_trails": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32p, i32p]),
        "mmw_tripwires_enable": (C.c_int, [vp, i32]),
        "mmw_set_tripwires": (C.c_int, [vp, vp, i32, vp, vp]),
        "mmw_get_tripwires": (C.c_int, [vp, vp, vp]),
        "mmw_tripwires_sample": (C.c_int, [vp, vp, vp]),
        "mmw_tripwires_async": (C.c_int, [vp, vp, i32, vp, i32, i32, i32]),
        "mmw_tripwires_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_tripwires": (C.c_int, [vp, vp, i32, vp, i32, i32, i32p, i32p]),
        "mmw_stance_enable": (C.c_int, [vp, i32]),
        "mmw_set_stance_rules": (C.c_int, [vp, vp, i32, vp, vp]),
        "mmw_get_stance_rules": (C.c_int, [vp, vp, vp]),
        "mmw_stance_sample": (C.c_int, [vp, vp, vp]),
        "mmw_stance_async": (C.c_int, [vp, vp, i32, vp, i32, i32, i32]),
        "mmw_stance_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_stance": (C.c_int, [vp, vp, i32, vp, i32, i32, i32p, i32p]),
        "mmw_heat_enable": (C.c_int, [vp, i32]),
        "mmw_set_heat_grids": (C.c_int, [vp, vp, i32, vp, vp]),
        "mmw_get_heat_grids": (C.c_int, [vp, vp, vp]),
        "mmw_heat_sample": (C.c_int, [vp, vp, vp]),
        "mmw_heat_async": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, i32, i32]),
        "mmw_heat_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_heat": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, i32, i32p, i32p]),
        "mmw_uart_open": (C.c_int, [vp, vp, i32, C.c_double]),
        "mmw_uart_close": (C.c_int, [vp]),
        "mmw_uart_read": (C.c_int, [vp, vp, vp, C.c_size_t, vp, C.c_double, vp, vp, vp, vp, vp]),
        "mmw_uart_get_state": (C.c_int, [vp, i32, vp, i32p, f64p]),
        "mmw_uart_set_state": (C.c_int, [vp, i32, vp, i32, C.c_double]),
        "mmw_uart_set_time": (C.c_int, [vp, vp, C.c_double]),
        "mmw_uart_log_enable": (C.c_int, [vp, i32]),
        "mmw_uart_log_async": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, i32, i32]),
        "mmw_uart_log_wait": (C.c_int, [vp, i32, i32p, i32p]),
        "mmw_uart_log": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, i32, i32p, i32p]),
        "mmw_samples_async": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, i32]),
        "mmw_samples_wait": (C.c_int, [vp, i32, i32p]),
        "mmw_samples": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, i32p]),
        "mmw_mars_conv2d": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32]),
        "mmw_mars_range_fixup_frames": (C.c_int, [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]),
        "mmw_posture_attach_frames": (C.c_int, [vp, vp, i32, i32]),
        "mmw_attach_posture_frames": (C.c_int, [vp, vp, i32]),
        "mmw_posture_attach_models": (C.c_int, [vp, vp, i32, i32, vp, i32]),
        "mmw_posture_set_scene_models": (C.c_int, [vp, vp, i32, vp]),
        "mmw_posture_get_scene_models": (C.c_int, [vp, vp]),
        "mmw_posture_group_rows": (C.c_int, [vp, vp, i32p]),
        "mmw_posture_owners": (C.c_int, [vp, vp, i32, i32p]),
    }


sig = _signatures()
EXPORTS = list(sig)


def skeleton_tables():
    """mmw_skeleton_tables (host only, no GPU): (connections int32[18, 2] -- the bones as joint index pairs, in the order the
    reference draws them --, joint_class int32[19]: 0 blue, 1 green, 2 red = the head)."""
    conn, cls = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    rc = load().mmw_skeleton_tables(C.byref(conn), C.byref(cls))
    if rc:
        raise MmwError(rc, "mmw_skeleton_tables")
    return (np.ctypeslib.as_array(conn, (SKEL_BONES, 2)).astype(np.int32), np.ctypeslib.as_array(cls, (SKEL_JOINTS,)).astype(np.int32))


_lib = None


class MmwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmmw_hip error {code}: {msg}")
        self.code = code


# The exceptions the reference's track() can raise on this path, as subclasses of BOTH MmwError and the reference's type, so
# that `except ValueError:` / `except np.linalg.LinAlgError:` around a drop-in TrackBuffer.track() keeps working:
#   sklearn's input validation in apply_DBscan (Utils.py:272-278)      -> ValueError
#   np.linalg.inv / det on a singular 6x6 (Tracking.py:556-560, filterpy) -> numpy.linalg.LinAlgError
#   (N_est - 1) * N == 0 in _get_Rc (Tracking.py:310-312)              -> ZeroDivisionError
class MmwNonFinite(MmwError, ValueError):
    pass


class MmwSingular(MmwError, np.linalg.LinAlgError):
    pass


class MmwDivZero(MmwError, ZeroDivisionError):
    pass


def error_for(code, msg) -> MmwError:
    cls = {E_NONFINITE: MmwNonFinite, E_SINGULAR: MmwSingular, E_DIVZERO: MmwDivZero}.get(code, MmwError)
    return cls(code, msg)


def last_error(ctx=None) -> str:
    """mmw_last_error: the message of the last failed call on `ctx`, or (None) of the last failed call that had no context."""
    return (load().mmw_last_error(ctx) or b"").decode()


def check(rc, ctx=None):
    """The one way a C-ABI status becomes an exception."""
    if rc != 0:
        raise error_for(rc, last_error(ctx))


def source_hash() -> str:
    """First 16 hex digits of the SHA-256 over csrc/*.hip, csrc/*.hpp (byte order of their names) and include/mmw.h:
    what csrc/Makefile compiles into mmw_version().  The sources travel with the package, so a library built from other
    sources -- a stale .so with a newer mtime, one copied in from another checkout -- is recognisable."""
    import hashlib
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp")))
    h = hashlib.sha256()
    for p in [os.path.join(CSRC, f) for f in names] + [os.path.join(os.path.dirname(_HERE), "include", "mmw.h")]:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def built_hash(path: str = None):
    """The src:<hash> a built library carries, read from the file (no dlopen); None if absent or unhashed."""
    import re
    path = path or LIB_PATH
    if not os.path.isfile(path):
        return None
    with open(path, "rb") as fh:
        m = re.search(rb"\(gfx950\) src:([0-9a-f]{16})", fh.read())
    return m.group(1).decode() if m else None


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree (hipcc --offload-arch=gfx950) unless the one present was built from exactly
    these sources (mmw_version()'s hash, not file times)."""
    if force or built_hash() != source_hash():
        subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=subprocess.DEVNULL)
        if built_hash() != source_hash():
            raise RuntimeError(f"{LIB_PATH}: built, but its source hash {built_hash()} is not {source_hash()}")
    return LIB_PATH


def _preload_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's, different file).
    Two HIP runtimes in one process cannot both own the GPU ("No HIP GPUs are available" in
    whichever comes second), so when torch is installed we bind to ITS runtime up front --
    without importing torch -- and torch later finds the same object already mapped."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        p = os.path.join(libdir, name)
        if os.path.isfile(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load():
    """Load libmmw_hip.so and declare every prototype.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_hip_runtime()
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950).  mmwave_msc_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.mmw_version.restype = C.c_char_p
    ver = (L.mmw_version() or b"").decode()
    if os.path.isdir(CSRC) and not ver.endswith("src:" + source_hash()):
        raise ImportError(
            f"{LIB_PATH} reports {ver!r} but the sources beside it hash to {source_hash()}: it was built from other "
            "sources.  Rebuild it: `python -c 'import __graft_entry__ as g; g.build()'`.")
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def default_config(**overrides) -> MmwConfig:
    cfg = MmwConfig()
    load().mmw_config_default(C.byref(cfg))
    apply_overrides(cfg, overrides)
    return cfg


def apply_overrides(cfg: MmwConfig, overrides: dict):
    for k, v in overrides.items():
        if k == "kf_spread_lim":
            for i in range(6):
                cfg.kf_spread_lim[i] = float(v[i])
        elif k == "default_posture":
            for i in range(NKP):
                cfg.default_posture[i] = float(v[i])
        elif k == "s_tilt":
            ang = np.radians(v)  # Utils.py:315
            cfg.tilt_cos, cfg.tilt_sin = float(np.cos(ang)), float(np.sin(ang))
        else:
            if not hasattr(cfg, k):
                raise AttributeError(f"mmw_config has no field {k!r}")
            setattr(cfg, k, v)
    return cfg


def make_sites(cfg: MmwConfig, n: int, **columns) -> np.ndarray:
    """SITE_DTYPE[n]: n sites that start as `cfg`'s own values.  Each keyword is a site field (SITE_FIELDS) given as a scalar or a
    length-n array, or `s_tilt` in degrees -- turned into tilt_cos / tilt_sin per element the way apply_overrides does for a
    config (np.cos(np.radians(.)), Utils.py:315), which is what makes a site bit-equal to a context created with that S_TILT."""
    sites = np.zeros(int(n), SITE_DTYPE)
    for f in SITE_FIELDS:
        sites[f] = getattr(cfg, f)
    for k, v in columns.items():
        col = np.asarray(v, np.float64)
        if col.ndim > 1 or (col.ndim == 1 and col.shape[0] != sites.shape[0]):
            raise ValueError(f"make_sites: {k} must be a scalar or have length {sites.shape[0]}, not shape {col.shape}")
        if k == "s_tilt":
            # element by element, as apply_overrides does for one config (a vectorised np.cos need not round like the scalar call)
            ang = [np.radians(float(a)) for a in np.broadcast_to(col, sites.shape)]
            sites["tilt_cos"], sites["tilt_sin"] = [float(np.cos(a)) for a in ang], [float(np.sin(a)) for a in ang]
        elif k in SITE_FIELDS:
            sites[k] = col
        else:
            raise AttributeError(f"mmw_scene_site has no field {k!r}")
    return sites


def make_zones(per_scene):
    """(n_zones int32[n], zones ZONE_DTYPE[n, ZONES_MAX]) for `mmw_set_zones` from one list per scene of up to ZONES_MAX zones, each
    a dict with keys of ZONE_FIELDS (`margin` and `id` may be left out: 0, and the zone's index) or a tuple
    (x0, x1, y0, y1[, margin[, id]]).  Entries past a scene's zones stay zero."""
    per_scene = list(per_scene)
    n_zones = np.zeros(len(per_scene), np.int32)
    zones = np.zeros((len(per_scene), ZONES_MAX), ZONE_DTYPE)
    for i, zs in enumerate(per_scene):
        zs = list(zs)
        if len(zs) > ZONES_MAX:
            raise ValueError(f"make_zones: scene entry {i} has {len(zs)} zones, at most {ZONES_MAX} fit")
        n_zones[i] = len(zs)
        for k, z in enumerate(zs):
            if isinstance(z, dict):
                unknown = set(z) - set(ZONE_FIELDS)
                if unknown:
                    raise AttributeError(f"mmw_zone has no field {sorted(unknown)[0]!r}")
                vals = [z[f] for f in ZONE_FIELDS[:4]] + [z.get("margin", 0.0), z.get("id", k)]
            else:
                z = tuple(z)
                if not 4 <= len(z) <= 6:
                    raise ValueError(f"make_zones: a zone is (x0, x1, y0, y1[, margin[, id]]), not {len(z)} values")
                vals = list(z) + [0.0, k][len(z) - 4:]
            for f, v in zip(ZONE_FIELDS, vals):
                zones[i, k][f] = v
    return n_zones, zones


def make_tripwires(per_scene):
    """(n_wires int32[n], wires TRIPWIRE_DTYPE[n, TRIPWIRES_MAX]) for `mmw_set_tripwires` from one list per scene of up to
    TRIPWIRES_MAX wires, each a dict with keys of TRIPWIRE_FIELDS (`margin` and `id` may be left out: 0, and the wire's index) or a
    tuple (ax, ay, bx, by[, margin[, id]]).  Entries past a scene's wires stay zero."""
    per_scene = list(per_scene)
    n_wires = np.zeros(len(per_scene), np.int32)
    wires = np.zeros((len(per_scene), TRIPWIRES_MAX), TRIPWIRE_DTYPE)
    for i, ws in enumerate(per_scene):
        ws = list(ws)
        if len(ws) > TRIPWIRES_MAX:
            raise ValueError(f"make_tripwires: scene entry {i} has {len(ws)} wires, at most {TRIPWIRES_MAX} fit")
        n_wires[i] = len(ws)
        for k, w in enumerate(ws):
            if isinstance(w, dict):
                unknown = set(w) - set(TRIPWIRE_FIELDS)
                if unknown:
                    raise AttributeError(f"mmw_tripwire has no field {sorted(unknown)[0]!r}")
                vals = [w[f] for f in TRIPWIRE_FIELDS[:4]] + [w.get("margin", 0.0), w.get("id", k)]
            else:
                w = tuple(w)
                if not 4 <= len(w) <= 6:
                    raise ValueError(f"make_tripwires: a wire is (ax, ay, bx, by[, margin[, id]]), not {len(w)} values")
                vals = list(w) + [0.0, k][len(w) - 4:]
            for f, v in zip(TRIPWIRE_FIELDS, vals):
                wires[i, k][f] = v
    return n_wires, wires


def make_stance_rules(per_scene):
    """(n_rules int32[n], rules STANCE_RULE_DTYPE[n, STANCE_RULES_MAX]) for `mmw_set_stance_rules` from one list per scene of zero or
    one rule, a dict with keys of STANCE_FIELDS or a tuple (h_stand, h_lie, margin, fall_window, long_lie, max_gap, id) cut short
    anywhere; what is left out is STANCE_DEFAULTS' (`id`: 0).  An entry without a rule stays zero."""
    per_scene = list(per_scene)
    n_rules = np.zeros(len(per_scene), np.int32)
    rules = np.zeros((len(per_scene), STANCE_RULES_MAX), STANCE_RULE_DTYPE)
    for i, rs in enumerate(per_scene):
        rs = list(rs)
        if len(rs) > STANCE_RULES_MAX:
            raise ValueError(f"make_stance_rules: scene entry {i} has {len(rs)} rules, at most {STANCE_RULES_MAX} fits")
        n_rules[i] = len(rs)
        for k, r in enumerate(rs):
            if isinstance(r, dict):
                unknown = set(r) - set(STANCE_FIELDS)
                if unknown:
                    raise AttributeError(f"mmw_stance_rule has no field {sorted(unknown)[0]!r}")
                vals = [r.get(f, STANCE_DEFAULTS[f]) for f in STANCE_FIELDS]
            else:
                r = tuple(r)
                if len(r) > len(STANCE_FIELDS):
                    raise ValueError(f"make_stance_rules: a rule is (h_stand, h_lie, margin, fall_window, long_lie, max_gap, id) or its head, not {len(r)} values")
                vals = list(r) + [STANCE_DEFAULTS[f] for f in STANCE_FIELDS[len(r):]]
            for f, v in zip(STANCE_FIELDS, vals):
                rules[i, k][f] = v
    return n_rules, rules


def make_heat_grids(per_scene):
    """(n_grids int32[n], grids HEAT_GRID_DTYPE[n, HEAT_GRIDS_MAX]) for `mmw_set_heat_grids` from one list per scene of zero or one
    grid, a dict with keys of HEAT_FIELDS (`max_gap` and `id` may be left out: +inf, and 0) or a tuple
    (x0, y0, cell, max_gap, nx, ny[, id]).  An entry without a grid stays zero."""
    per_scene = list(per_scene)
    n_grids = np.zeros(len(per_scene), np.int32)
    grids = np.zeros((len(per_scene), HEAT_GRIDS_MAX), HEAT_GRID_DTYPE)
    for i, gs in enumerate(per_scene):
        gs = list(gs)
        if len(gs) > HEAT_GRIDS_MAX:
            raise ValueError(f"make_heat_grids: scene entry {i} has {len(gs)} grids, at most {HEAT_GRIDS_MAX} fits")
        n_grids[i] = len(gs)
        for k, g in enumerate(gs):
            if isinstance(g, dict):
                unknown = set(g) - set(HEAT_FIELDS)
                if unknown:
                    raise AttributeError(f"mmw_heat_grid has no field {sorted(unknown)[0]!r}")
                vals = [g["x0"], g["y0"], g["cell"], g.get("max_gap", float("inf")), g["nx"], g["ny"], g.get("id", 0)]
            else:
                g = tuple(g)
                if not 6 <= len(g) <= 7:
                    raise ValueError(f"make_heat_grids: a grid is (x0, y0, cell, max_gap, nx, ny[, id]), not {len(g)} values")
                vals = list(g) + [0][len(g) - 6:]
            for f, v in zip(HEAT_FIELDS, vals):
                grids[i, k][f] = v
    return n_grids, grids
