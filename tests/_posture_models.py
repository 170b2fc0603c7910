"""Shared by test_posture_models_exports.py (CPU) and test_gpu_posture_models.py (GPU): a numpy restatement of what
k_feat_scan_models (csrc/k_feat_models.hip) hands out -- the rows of a call model by model, every model's band on a multiple of
256 -- and the owner list of such a call from that of a uniform context.  Nothing here touches a GPU or torch."""
import numpy as np

NONE = -1   # MMW_POSTURE_NONE


def pad256(v):
    return (int(v) + 255) // 256 * 256


def grouped_offsets(counts, model_of, n_models, buffer_rows):
    """counts[S] (eligible tracks per scene), model_of[S] (model index, NONE = no model) -> (offsets[S], bases[n_models],
    totals[n_models]): offsets[s] = bases[m] + the rows of earlier scenes of the same model, bases[0] = 0,
    bases[m + 1] = bases[m] + pad256(totals[m]); a scene on NONE gets buffer_rows (at or beyond the buffer: its rows are dropped)."""
    counts, model_of = np.asarray(counts, dtype=np.int64), np.asarray(model_of, dtype=np.int64)
    assert counts.shape == model_of.shape and counts.ndim == 1
    totals = np.array([counts[model_of == m].sum() for m in range(n_models)], dtype=np.int64)
    bases = np.zeros(n_models, dtype=np.int64)
    for m in range(1, n_models):
        bases[m] = bases[m - 1] + pad256(totals[m - 1])
    offsets = np.full(len(counts), buffer_rows, dtype=np.int64)
    for m in range(n_models):
        mine = np.flatnonzero(model_of == m)
        offsets[mine] = bases[m] + np.cumsum(counts[mine]) - counts[mine]
    return offsets, bases, totals


def grouped_owners(owners, model_of, n_models):
    """The (scene, list position) rows of a uniform context's call, [n, 2] by ascending scene, in the order a context with the map
    `model_of` estimates them: model by model, within a model as they were; the scenes on NONE left out.  Returns (rows, per-model counts)."""
    owners = np.asarray(owners, dtype=np.int32).reshape(-1, 2)
    model_of = np.asarray(model_of)
    of_row = model_of[owners[:, 0]] if len(owners) else np.zeros(0, dtype=np.int64)
    parts = [owners[of_row == m] for m in range(n_models)]
    return (np.concatenate(parts) if parts else owners[:0]), np.array([len(p) for p in parts], dtype=np.int32)
