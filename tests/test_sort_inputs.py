"""The key frames of tests/_sort_inputs.py tell a wrong sort network from the right one -- shown here in numpy alone, without a
GPU.  The model of the network is written from the (SZ, STRIDE) list of mmwave_msc_amd/csrc/mmw_sort.hpp and shares no code with
the kernel; tests/test_gpu_format_frames.py holds the kernel itself to format_frames_ref on the same frames.

What the model says of the network: on keys that are not NaN it IS np.argsort(kind="stable"), ties, -0.0 and +-inf included; every
one of its 21 steps is needed for these frames; turning the direction of a step of the LAST merge, breaking ties by the larger
row, or comparing the keys as fp32 changes bytes.  (Turning a step of an EARLIER merge changes nothing: the last merge sorts any
bitonic input, and the model confirms those 15 mutants equivalent -- they are not required to be caught.)  On a NaN key the bare
network is no permutation at all: `<` and `==` are false on both sides of a pair, both lanes keep the same element.  That is why
mmw_format_frames, whose rows are the caller's, sorts through sort_rows_store_nan_last; k_features cannot meet a NaN key
(mmw_sort.hpp says why) and runs the bare network."""
import numpy as np
import pytest

from tests import _sort_inputs as si
from tests._golden import assert_feat_equal, assert_feat_identical, canon_feat

FINITE, NAN = si.finite_frames(), si.nan_frames()


def _changed(**rule):
    """The finite frames whose output bytes the wrong rule changes."""
    return [kf.tag for kf in FINITE if not np.array_equal(si.gathered(kf, si.network(si.keys64(kf), **rule)), si.gathered(kf, si.reference_order(kf)))]


def test_steps_are_the_21_of_the_header():
    assert len(si.STEPS) == 21 and si.STEPS[0] == (2, 1) and si.STEPS[1:3] == ((4, 2), (4, 1)) and si.STEPS[-6:] == tuple((64, s) for s in (32, 16, 8, 4, 2, 1))
    assert si.LAST_MERGE == tuple(range(15, 21))
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "mmwave_msc_amd", "csrc", "mmw_sort.hpp")).read()
    body = hdr[hdr.index("void bitonic_sort64"):]
    merges = [f"bitonic_merge<{sz}, {sz // 2}>(lane, key, src);" for sz in (2, 4, 8, 16, 32, 64)]
    assert [body.index(m) for m in merges] == sorted(body.index(m) for m in merges)
    assert "bitonic_merge<SZ, STRIDE / 2>" in hdr


def test_the_frames_are_the_families_asked_for():
    tags = [kf.tag for kf in FINITE]
    assert len(set(tags)) == len(tags) and 35 <= len(FINITE) + len(NAN) <= 100
    for name in si.ALPHABETS:
        assert {kf.m for kf in FINITE if kf.tag.startswith(name + " ")} == set(si.SIZES)
    assert {kf.count for kf in FINITE} >= {-1, 0, 65, 1000}
    tie_with_pad = [kf for kf in FINITE if 0 < kf.m < 64 and np.any(kf.keys == 0)]
    assert len(tie_with_pad) >= 8                                   # real rows that tie with the pad rows
    assert any(np.any(np.signbit(kf.keys) & (kf.keys == 0)) and np.any(~np.signbit(kf.keys) & (kf.keys == 0)) for kf in FINITE)
    assert any(np.isposinf(kf.keys).any() and np.isneginf(kf.keys).any() for kf in FINITE)
    assert not any(np.isnan(kf.keys).any() for kf in FINITE) and all(np.isnan(kf.keys).any() for kf in NAN)
    assert any(np.isnan(kf.keys).all() for kf in NAN) and sum(int(np.isnan(kf.keys).sum() == 1) for kf in NAN) >= 1
    assert any(np.isnan(kf.keys).any() and np.isposinf(kf.keys).any() for kf in NAN)
    for kf in FINITE + NAN:                                         # a swap inside a tie group changes bytes: the payload names the row
        r = si.rows5(kf)[: kf.m]
        assert len({row[1:].tobytes() for row in r}) == kf.m
        for rf in ((0.0 if kf.zero_ref else si.REF[0], si.REF[1]),):
            with np.errstate(invalid="ignore"):
                back = si.rows_of(kf, rf)[: kf.m, 0] - rf[0]
            assert back.tobytes() == kf.keys.tobytes(), kf.tag      # x - ref_x is the key, to the sign of a zero


@pytest.mark.parametrize("ring", [3, 1])
def test_packed_items_hold_every_frame_and_leave_idle_waves(ring):
    p = si.pack("all", ring)
    B = len(p.frames)
    assert (B * ring) % 4 != 0 and p.counts.shape == (B, ring)
    held = [kf.tag for item in p.src for kf in item if kf is not None]
    assert set(held) == {kf.tag for kf in FINITE + NAN}
    assert np.any(p.ref[:, 0] != 0) and np.all(p.ref[:, 1] != 0)
    groups = [sorted({min(max(int(c), 0), 64) for c in p.counts.reshape(-1)[i: i + 4]}) for i in range(0, B * ring, 4)]
    assert sum(len(g) >= 3 for g in groups) >= 4                    # workgroups whose four frames differ in m
    want = si.format_frames_ref(p.frames, p.counts, p.ref, si.MU, si.STD, ring)
    assert want.shape == (B, ring, 64, 5) and want.dtype == np.float32
    assert not np.any(want == 100.0) and not np.any(np.abs(want[..., 1]) > 64)          # no junk row past a count shows
    for b, item in enumerate(p.src):
        for k, kf in enumerate(item):
            if kf is None:
                assert p.counts[b, k] == -1 and not want[b, k].any()
            else:
                assert np.array_equal(want[b, k].view(np.uint32), si.gathered(kf, si.reference_order(kf))), kf.tag


def test_reference_is_the_stable_sort_with_nan_last():
    for kf in FINITE + NAN:
        order = si.reference_order(kf)
        assert sorted(order.tolist()) == list(range(64))
        k = si.keys64(kf)[order]
        nn = int(np.isnan(k).sum())
        assert np.all(np.isnan(k[64 - nn:])) and np.all(np.diff(k[: 64 - nn][~np.isinf(k[: 64 - nn])]) >= 0)
        for v in set(k[: 64 - nn].tolist()) | ({np.nan} if nn else set()):
            rows = order[np.isnan(k)] if v != v else order[k == v]
            assert np.all(np.diff(rows) > 0), (kf.tag, v)           # ties, and the NaN rows, in row order
    kf = next(kf for kf in NAN if kf.tag.startswith("NaN beside +inf"))
    k = si.keys64(kf)[si.reference_order(kf)]
    assert np.isposinf(k[64 - 5: 64 - 2]).all() and np.isnan(k[64 - 2:]).all()


def test_model_of_the_network_is_the_reference_on_every_finite_frame():
    for kf in FINITE:
        assert np.array_equal(si.network(si.keys64(kf)), si.reference_order(kf)), kf.tag
        assert np.array_equal(si.network_nan_last(si.keys64(kf)), si.reference_order(kf)), kf.tag
    assert any(np.array_equal(si.reference_order(kf), np.arange(64)) and kf.m == 64 for kf in FINITE)   # the identity is asked for


@pytest.mark.parametrize("step", range(21))
def test_every_dropped_step_changes_a_frame(step):
    changed = _changed(drop=step)
    print(f"step {step} {si.STEPS[step]} dropped: {len(changed)} of {len(FINITE)} frames change")
    assert changed


@pytest.mark.parametrize("step", si.LAST_MERGE)
def test_a_reversed_step_of_the_last_merge_changes_a_frame(step):
    changed = _changed(reverse=(step,))
    print(f"step {step} {si.STEPS[step]} reversed: {len(changed)} of {len(FINITE)} frames change")
    assert changed


def test_reversed_steps_of_the_earlier_merges_are_equivalent_and_not_asked_for():
    rng = np.random.default_rng(3)
    for step in range(15):
        assert not _changed(reverse=(step,))
        for _ in range(20):
            k = rng.integers(-3, 4, size=64) / 4.0
            assert np.array_equal(si.network(k, reverse=(step,)), np.argsort(k, kind="stable"))


def test_ties_by_the_larger_row_and_fp32_keys_change_frames():
    larger, f32 = _changed(tie_larger=True), _changed(key32=True)
    print(f"ties by the larger row: {len(larger)} of {len(FINITE)} frames change; fp32 keys: {f32}")
    tied = []                                                        # a key shared by two rows of which one at least is real
    for kf in FINITE:
        k = si.keys64(kf)
        if any(np.sum(k == v) > 1 and np.any(k[: kf.m] == v) for v in set(k.tolist())):
            tied.append(kf.tag)
    assert larger == tied and len(tied) >= 34, (larger, tied)
    assert sorted(f32) == ["adjacent doubles m=32", "adjacent doubles m=64"]


def test_bare_network_is_no_permutation_on_nan_keys_and_the_nan_last_form_is_the_reference():
    for kf in NAN:
        bare = si.network(si.keys64(kf))
        lost = 64 - len(set(bare.tolist()))
        print(f"{kf.tag}: the bare network loses {lost} rows")
        if kf.m > 1:
            assert lost >= 1, kf.tag                                # rows lost, others written twice: the network must not see NaN
        assert np.array_equal(si.network_nan_last(si.keys64(kf)), si.reference_order(kf)), kf.tag
        assert np.array_equal(si.gathered(kf, si.network_nan_last(si.keys64(kf))), si.gathered(kf, si.reference_order(kf)))
    rng = np.random.default_rng(4)
    for _ in range(200):
        k = rng.integers(-3, 4, size=64) / 4.0
        k[rng.integers(0, 64)] = np.nan
        assert len(set(si.network(k).tolist())) < 64
        assert np.array_equal(si.network_nan_last(k), np.argsort(k, kind="stable"))


def test_nan_last_form_is_sensitive_to_the_same_wrong_rules():
    for kf in NAN:
        if 1 < int(np.isnan(kf.keys).sum()):
            assert not np.array_equal(si.gathered(kf, si.network_nan_last(si.keys64(kf), tie_larger=True)), si.gathered(kf, si.reference_order(kf))), kf.tag


# ------------------------------------------------------------------------------------------- the shared feature comparison
def _frame():
    f = np.zeros((64, 5), np.float32)
    f[:, 0] = np.repeat(np.arange(16) / 8.0 - 1, 4)
    f[:, 1] = np.arange(64) + 1
    return f


def test_assert_feat_equal_accepts_a_swap_inside_a_tie_group_only():
    want = _frame()
    tie = want.copy()
    tie[[4, 6]] = tie[[6, 4]]                                        # two rows of equal x
    assert_feat_equal(tie, want)
    with pytest.raises(AssertionError):
        assert_feat_identical(tie, want)
    unsorted = want.copy()
    unsorted[[3, 4]] = unsorted[[4, 3]]                              # two rows of different x: the same rows, not sorted
    assert np.array_equal(unsorted[np.lexsort(unsorted.T[::-1])], want)
    with pytest.raises(AssertionError):
        assert_feat_equal(unsorted, want)
    with pytest.raises(AssertionError):
        assert_feat_equal(want, unsorted)
    with pytest.raises(AssertionError):
        canon_feat(unsorted)
    other = want.copy()
    other[5, 3] = 1.0
    with pytest.raises(AssertionError):
        assert_feat_equal(other, want)


def test_feature_comparisons_on_nan_and_signed_zero():
    want = _frame()
    want[60:, 0] = np.nan                                            # NaN x at the end: sorted
    assert_feat_equal(want.copy(), want)
    assert_feat_identical(want.copy(), want)
    swapped = want.copy()
    swapped[[61, 62]] = swapped[[62, 61]]
    assert_feat_equal(swapped, want)                                 # the NaN rows are one tie group
    early = want.copy()
    early[[0, 63]] = early[[63, 0]]                                  # a NaN before a number
    with pytest.raises(AssertionError):
        assert_feat_equal(early, want)
    zero = _frame()
    zero[:, 0] = 0
    neg = zero.copy()
    neg[7, 0] = -0.0
    assert np.array_equal(neg, zero)
    assert_feat_equal(neg, zero)
    with pytest.raises(AssertionError):
        assert_feat_identical(neg, zero)                             # a -0.0 in the wrong row is seen
