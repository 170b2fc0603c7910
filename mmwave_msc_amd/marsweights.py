"""The MARS models' facts without torch (train.py:33-106): their dimensions (model_dims), which model a set of Keras weights is
(frames_of), seeded random weights in Keras' tensor shapes and the one BatchNormalization fold (fold_keras_weights) -- numpy only:
the CPU-side tools (the oracle's child processes of bench_e2e.oracle_reference, fixture generators) and the torch-free C-ABI
path import this without paying for `import torch`; mars.MarsCNN and train.MarsTrainNet take their sizes and tensors from here."""
from typing import NamedTuple

import numpy as np

N_KEYPOINTS = 57   # 19 joints x (x, y, z)  (preprocessing.py:377)
BN_EPS = 1e-3      # Keras' BatchNormalization default


class ModelDims(NamedTuple):
    frames: int     # 3 = define_CNN_3D (train.py:71-106), 1 = define_CNN (train.py:33-68)
    per: int        # floats of one feature tensor
    flat: int       # floats the conv pair hands Dense-1 (Keras' Flatten)
    hidden: int     # Dense-1's outputs
    taps: int       # positions of a conv kernel
    kernel: tuple   # ... and its spatial shape
    input: tuple    # one sample's shape, channels last


def model_dims(frames: int) -> ModelDims:
    """The model of `frames` frames per sample.  For 3 and 1 -- the models the HIP library serves -- per / flat / hidden / taps are
    cnn_dims() of csrc/mmw_ctx.hpp; any other count is a Conv3D model of that depth with define_CNN_3D's hidden layer (torch path)."""
    frames = int(frames)
    three_d = frames > 1
    depth = frames if three_d else 1
    return ModelDims(frames, depth * 8 * 8 * 5, depth * 64 * 32, 512 * (3 if three_d else 1), 27 if three_d else 9,
                     (3, 3, 3) if three_d else (3, 3), (depth, 8, 8, 5) if three_d else (8, 8, 5))


def frames_of(w: dict) -> int:
    """Which model Keras-convention weights are: Conv3D kernels -> the depth Dense-1's input width implies, Conv2D kernels -> 1."""
    three_d = np.asarray(w["conv1_w"]).ndim == 5
    return np.asarray(w["dense1_w"]).shape[0] // model_dims(1).flat if three_d else 1


def random_keras_weights(seed: int = 0, frames: int = 3) -> dict:
    """Seeded random weights with Keras shapes (Glorot-like scales, non-trivial BN stats)."""
    rng = np.random.default_rng(seed)
    d = model_dims(frames)
    k, flat, hidden = d.kernel, d.flat, d.hidden

    def glorot(shape, fan_in, fan_out):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)

    rf = d.taps
    w = {
        "conv1_w": glorot(k + (5, 16), rf * 5, rf * 16), "conv1_b": rng.normal(0, 0.05, 16).astype(np.float32),
        "conv2_w": glorot(k + (16, 32), rf * 16, rf * 32), "conv2_b": rng.normal(0, 0.05, 32).astype(np.float32),
        "bn1_gamma": rng.uniform(0.5, 1.5, 32).astype(np.float32), "bn1_beta": rng.normal(0, 0.1, 32).astype(np.float32),
        "bn1_mean": rng.normal(0.2, 0.1, 32).astype(np.float32), "bn1_var": rng.uniform(0.05, 0.5, 32).astype(np.float32),
        "dense1_w": glorot((flat, hidden), flat, hidden), "dense1_b": rng.normal(0, 0.05, hidden).astype(np.float32),
        "bn2_gamma": rng.uniform(0.5, 1.5, hidden).astype(np.float32), "bn2_beta": rng.normal(0, 0.1, hidden).astype(np.float32),
        "bn2_mean": rng.normal(0.2, 0.1, hidden).astype(np.float32), "bn2_var": rng.uniform(0.05, 0.5, hidden).astype(np.float32),
        "dense2_w": glorot((hidden, N_KEYPOINTS), hidden, N_KEYPOINTS), "dense2_b": rng.normal(0, 0.05, N_KEYPOINTS).astype(np.float32),
    }
    return w


def load_keras_weights(src) -> dict:
    """The Keras-convention tensors (keys: mars.py) from a dict, an `.npz` or a Keras `.h5` / `.hdf5` path -- what
    MarsCNN.from_keras_weights / MarsCNN.load take."""
    if isinstance(src, dict):
        return src
    path = str(src)
    if path.lower().endswith((".h5", ".hdf5")):
        from .h5weights import load_keras_h5
        return load_keras_h5(path)
    z = np.load(path)
    return {k: z[k] for k in z.files}


# the arrays of fold_keras_weights' result, in the order _lib.MmwPostureModel.of takes their device pointers
FOLDED_KEYS = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "dense1_w", "dense1_b", "dense2_w", "dense2_b")


def fold_keras_weights(w: dict) -> dict:
    """The fp32 tensors the HIP kernels take, from Keras-convention weights: both BatchNormalizations folded into the Dense layer
    behind them in fp64 and rounded once.  The only fold: MarsCNN.from_keras_weights copies these arrays (conv1_w .. conv2_b = k_w1 ..
    k_b2, dense1_w / dense1_b = dense1_dhwc, dense2_w / dense2_b = dense2) and permutes dense1_w for its channels-first Dense-1.
    Layouts = struct mmw_posture_model: conv kernels flat in Keras order (kd,kh,kw,in,out), dense1_w
    [hidden][flat] (K contiguous, Keras' Flatten order), dense2_w [57][hidden].  `frames` = 3 (define_CNN_3D) or 1 (define_CNN)."""
    flat = np.asarray(w["dense1_w"]).shape[0]
    f64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    a1 = f64["bn1_gamma"] / np.sqrt(f64["bn1_var"] + BN_EPS)
    c1 = f64["bn1_beta"] - a1 * f64["bn1_mean"]
    spatial = flat // 32
    w1 = f64["dense1_w"].reshape(spatial, 32, -1)            # [s, c, out]
    b1 = f64["dense1_b"] + np.einsum("c,sco->o", c1, w1)
    wk = (f64["dense1_w"].reshape(spatial, 32, -1) * a1[None, :, None]).reshape(flat, -1)  # Keras row order kept
    a2 = f64["bn2_gamma"] / np.sqrt(f64["bn2_var"] + BN_EPS)
    c2 = f64["bn2_beta"] - a2 * f64["bn2_mean"]
    w2 = f64["dense2_w"]
    f32 = lambda a: np.ascontiguousarray(a).astype(np.float32)
    return {
        "frames": frames_of(w),
        "conv1_w": f32(f64["conv1_w"].reshape(-1)), "conv1_b": f32(f64["conv1_b"]),
        "conv2_w": f32(f64["conv2_w"].reshape(-1)), "conv2_b": f32(f64["conv2_b"]),
        "dense1_w": f32(wk.T.copy()), "dense1_b": f32(b1),
        "dense2_w": f32((w2 * a2[:, None]).T.copy()), "dense2_b": f32(f64["dense2_b"] + c2 @ w2),
    }
