"""Seeded random MARS weights in Keras' tensor shapes (train.py:33-106) -- numpy only, no torch: the CPU-side tools (the
oracle's child processes of bench_e2e.oracle_reference, fixture generators) import this without paying for `import torch`."""
import numpy as np

N_KEYPOINTS = 57   # 19 joints x (x, y, z)  (preprocessing.py:377)
BN_EPS = 1e-3      # Keras' BatchNormalization default (mars.BN_EPS)


def random_keras_weights(seed: int = 0, frames: int = 3) -> dict:
    """Seeded random weights with Keras shapes (Glorot-like scales, non-trivial BN stats)."""
    rng = np.random.default_rng(seed)
    three_d = frames > 1
    k = (3, 3, 3) if three_d else (3, 3)
    flat = (frames if three_d else 1) * 64 * 32
    hidden = 512 * (3 if three_d else 1)

    def glorot(shape, fan_in, fan_out):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)

    rf = int(np.prod(k))
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


def fold_keras_weights(w: dict) -> dict:
    """The fp32 tensors the HIP kernels take, from Keras-convention weights: both BatchNormalizations folded into the Dense layer
    behind them in fp64 and rounded once -- the operations of MarsCNN.from_keras_weights in the same order, so every array equals
    the model's tensor bit for bit (conv1_w .. conv2_b = k_w1 .. k_b2, dense1_w / dense1_b = dense1_dhwc, dense2_w / dense2_b =
    dense2), without torch.  Layouts = struct mmw_posture_model: conv kernels flat in Keras order (kd,kh,kw,in,out), dense1_w
    [hidden][flat] (K contiguous, Keras' Flatten order), dense2_w [57][hidden].  `frames` = 3 (define_CNN_3D) or 1 (define_CNN)."""
    three_d = np.asarray(w["conv1_w"]).ndim == 5
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
        "frames": (flat // (64 * 32)) if three_d else 1,
        "conv1_w": f32(f64["conv1_w"].reshape(-1)), "conv1_b": f32(f64["conv1_b"]),
        "conv2_w": f32(f64["conv2_w"].reshape(-1)), "conv2_b": f32(f64["conv2_b"]),
        "dense1_w": f32(wk.T.copy()), "dense1_b": f32(b1),
        "dense2_w": f32((w2 * a2[:, None]).T.copy()), "dense2_b": f32(f64["dense2_b"] + c2 @ w2),
    }
