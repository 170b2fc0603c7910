"""The training sample of mmw_samples_* (include/mmw.h) restated in numpy over a track's ring frames and its centroid: what
preprocessing.py:192-220 saves (relative_coordinates + format_batched_frames, Utils.py:437-465, 523-548) and what
format_mmwave_to_npy makes of it (format_single_frame_mode(np.float32(block), mean, std, 1, fuse=True), Utils.py:551-572), with
np.argsort's open tie order fixed as the stable sort of the reference's array gives it.  tests/test_sample_exports.py pins both
functions to the repository's utils; tests/test_gpu_samples.py compares the kernels with them."""
import numpy as np

FRAMES, ROWS, COLS = 3, 64, (0, 1, 2, 6, 7)


def block_of(frames, centroid=None) -> np.ndarray:
    """(192, 5) float64: `frames` = the ring oldest first, each (n, 8); centroid None = MMW_SAMPLE_ABSOLUTE."""
    frames = [np.asarray(f, np.float64).reshape(-1, 8) for f in frames]
    if len(frames) > FRAMES:
        raise ValueError(f"{len(frames)} frames do not fit the 3 x 64 row block")
    out = np.zeros((FRAMES * ROWS, len(COLS)))
    for j, fr in enumerate(reversed(frames)):              # newest first
        rows = fr[:ROWS][:, list(COLS)].copy()
        if centroid is not None:
            rows[:, 0] = rows[:, 0] - float(centroid[0])    # fp64; the other columns have 0 subtracted: unchanged
            rows[:, 1] = rows[:, 1] - float(centroid[1])
        out[j * ROWS: j * ROWS + len(rows)] = rows          # pad rows and absent frames stay true zeros
    return out


def input_of(block, mean, std) -> np.ndarray:
    """(8, 8, 5) float32 of a (192, 5) block: rows 0..63, one rounding to fp32, the intensity by two fp32 operations, all-zero
    rows behind the others as true zeros, stable argsort on x."""
    b = np.asarray(block, np.float64)[:ROWS].astype(np.float32)
    b[:, 4] = (b[:, 4] - np.float32(mean)) / np.float32(std)
    keep = np.any(b != 0, axis=1)
    frame = np.zeros((ROWS, 5), np.float32)
    frame[: int(keep.sum())] = b[keep]
    return frame[np.argsort(frame[:, 0], kind="stable")].reshape(8, 8, 5)


def entry_of(scene, uid, ring_n, centroid, dtype) -> np.ndarray:
    """The directory entry: ring_n = rows the reference holds per frame, oldest first."""
    e = np.zeros((), dtype)
    rn = [int(v) for v in ring_n]
    e["scene"], e["uid"], e["frames"] = scene, uid, len(rn)
    e["rows"][: len(rn)] = rn[::-1]
    e["cut"] = sum(max(0, v - ROWS) for v in rn)
    e["centroid"] = np.asarray(centroid, np.float64)[:2]
    return e


def is_sample(n_tracks, lifetime0, ring_n) -> bool:
    """preprocessing.py:192-194 on effective_tracks[0]: there is one, the frame updated it, its effective_data is not empty."""
    return n_tracks > 0 and lifetime0 == 0 and sum(int(v) for v in ring_n) > 0
