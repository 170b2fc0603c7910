"""Per-scene posture models (include/mmw.h: mmw_posture_attach_models) without a GPU: the numpy restatement of the
model-by-model scan and its properties, the five entries in the header, the library and _lib, what they do with a NULL context, and
the compiler's report on k_feat_scan_models."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._posture_models import NONE, grouped_offsets, grouped_owners, pad256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmw_posture_attach_models", "mmw_posture_set_scene_models", "mmw_posture_get_scene_models", "mmw_posture_group_rows",
           "mmw_posture_owners")


def _check_properties(counts, model_of, n_models, buffer_rows):
    off, bases, totals = grouped_offsets(counts, model_of, n_models, buffer_rows)
    assert bases[0] == 0 and all(b % 256 == 0 for b in bases)
    for m in range(n_models):
        mine = np.flatnonzero(model_of == m)
        assert totals[m] == counts[mine].sum()
        if m + 1 < n_models:   # model order; an empty model shares its base with the next one
            assert bases[m + 1] == bases[m] + pad256(totals[m]) >= bases[m]
            assert (bases[m + 1] == bases[m]) == (totals[m] == 0)
        # inside a model the scenes ascend and are contiguous: every scene starts where the one before it ended
        at = bases[m]
        for s in mine:
            assert off[s] == at
            at += counts[s]
        assert at == bases[m] + totals[m]
    assert (off[model_of == NONE] >= buffer_rows).all()
    # no two rows of the call share a place, and every row lies inside the buffer when the buffer is sized as the attachment sizes it
    rows = np.concatenate([np.arange(off[s], off[s] + counts[s]) for s in np.flatnonzero(model_of != NONE)] or [np.zeros(0, np.int64)])
    assert len(np.unique(rows)) == len(rows) == totals.sum()
    if len(rows) and totals.sum() <= buffer_rows - 256 * n_models:
        assert rows.max() < buffer_rows
    return off, bases, totals


@pytest.mark.parametrize("seed", range(12))
def test_grouped_offsets_properties_on_random_maps(seed):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(1, 3000))
    n_models = int(rng.integers(1, 9))
    counts = rng.integers(0, 5, size=S) * (rng.random(S) < 0.6)
    model_of = rng.integers(-1, n_models, size=S)
    if seed % 3 == 0 and n_models > 1:
        model_of[model_of == n_models // 2] = NONE   # a model without scenes
    if seed % 4 == 1 and n_models > 1:
        counts[model_of == n_models - 1] = 0         # a model with scenes but no rows
    buffer_rows = pad256(counts[model_of != NONE].sum()) + 256 * n_models
    _check_properties(counts, model_of, n_models, buffer_rows)


@pytest.mark.parametrize("total", [0, 1, 255, 256, 257])
def test_grouped_offsets_at_the_band_edges(total):
    """Model 0 gets exactly `total` rows over one-row scenes, model 1 follows it, model 2 has scenes without rows, model 3 none."""
    S = 600
    counts = np.zeros(S, dtype=np.int64)
    model_of = np.full(S, NONE, dtype=np.int64)
    zero = np.arange(0, S, 2)[:total]
    counts[zero], model_of[zero] = 1, 0
    one = np.arange(1, S, 2)[:3]
    counts[one], model_of[one] = 2, 1
    model_of[[S - 1, S - 3]] = 2
    off, bases, totals = _check_properties(counts, model_of, 4, pad256(total + 6) + 4 * 256)
    assert list(totals) == [total, 6, 0, 0]
    assert list(bases) == [0, pad256(total), pad256(total) + 256, pad256(total) + 256]
    assert off[S - 1] == off[S - 3] == bases[2] and off[S - 2] == pad256(total + 6) + 4 * 256


def test_grouped_owners_reorders_a_uniform_owner_list_model_by_model():
    owners = np.array([(0, 0), (0, 1), (1, 0), (3, 0), (3, 2), (4, 1)], dtype=np.int32)
    rows, per = grouped_owners(owners, np.array([1, NONE, 0, 0, 1]), 3)
    assert rows.tolist() == [[3, 0], [3, 2], [0, 0], [0, 1], [4, 1]] and per.tolist() == [2, 3, 0]


def test_header_library_and_lib_carry_the_five_entries_and_two_macros():
    from mmwave_msc_amd import _lib
    from tests import _abi
    protos = _abi.header_prototypes()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, f"{name}: not declared in include/mmw.h"
        assert name in _lib.sig and hasattr(lib, name), name
    assert _abi.header_defines()["MMW_POSTURE_MODELS_MAX"] == 8 == _lib.POSTURE_MODELS_MAX
    assert _abi.header_defines()["MMW_POSTURE_NONE"] == -1 == _lib.POSTURE_NONE == NONE


def test_null_context_is_refused_and_the_outputs_are_left_alone():
    from mmwave_msc_amd import _lib
    L = _lib.load()
    model = _lib.MmwPostureModel()
    out = np.full(8, 77, dtype=np.int32)
    n = C.c_int32(77)
    assert L.mmw_posture_attach_models(None, C.byref(model), 1, 1, None, 64) == _lib.E_ARG
    assert L.mmw_posture_set_scene_models(None, None, 0, None) == _lib.E_ARG
    assert L.mmw_posture_get_scene_models(None, out.ctypes.data) == _lib.E_ARG
    assert L.mmw_posture_group_rows(None, out.ctypes.data, C.byref(n)) == _lib.E_ARG
    assert L.mmw_posture_owners(None, out.ctypes.data, 4, C.byref(n)) == _lib.E_ARG
    assert (out == 77).all() and n.value == 77
    assert b"mmw_posture_owners" in L.mmw_last_error(None)


def test_the_scan_kernel_compiles_clean_with_two_64_bit_arrays_of_lds():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_feat_models",))["k_feat_models"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    assert len(names) == 1 and "k_feat_scan_models" in names[0], names
    assert_clean(rows)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    assert lds == [16384], lds   # two 64-bit arrays of 1024
    body = kernel_body(asm, names[0], ".Lfunc_end")
    assert "scratch_" not in body and "atomic" not in body
    # integers only: no floating-point instruction of any width
    assert not re.search(r"\bv_(add|mul|fma|mac|cvt)_f(16|32|64)", body)
    src = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", "mmw_kernels.hpp")).read()
    assert src.count("launch_feat_scan_models(") == 1, "the launcher is declared once"
