"""The crafted inputs of test_gpu_sort_ranges.py are what their names say (numpy alone, no GPU): the key range that decides which sort
m2s_sort.hip takes, who survives the frustum test, what becomes of the special values in the reference formula, and that every set has
ties for the sort's stability to show on.  Conditions on the inputs, not measurements: they hold exactly.

What a size can hold: one record has a range of 0 whatever the set is called; two records hold both ends of the range but no tie;
from three records on every set has both.  All listed sizes but 1 and 2 are therefore checked for everything."""
import numpy as np
import pytest

import camera
import sort_cases as sc

VIEW = sc.depth_view()
SECOND = sc.second_view()


def keys_of(name, n, view=VIEW):
    return sc.want_keys(sc.records_with_keys(sc.key_bits(name, n), seed=n), view)


def has_distant_tie(keys, pos=None) -> bool:
    """two equal keys at input positions (pos[i], default i) that are not neighbours"""
    order = np.argsort(keys, kind="stable")
    k = keys[order]
    if pos is not None:
        order = np.asarray(pos)[order]
    first = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))      # start of every run of equal keys
    last = np.concatenate([first[1:], [k.shape[0]]]) - 1
    return bool(np.any(order[last] - order[first] > 1))                   # (stable: positions ascend inside a run)


def test_records_carry_the_bits_an_index_and_distinct_words():
    bits = sc.key_bits("mixed_sign", 1025)
    rec = sc.records_with_keys(bits, seed=7)
    w = rec.view(np.uint32)
    assert rec.dtype == np.float32 and rec.shape == (1025, 24)
    assert np.array_equal(w[:, 0], bits) and not w[:, 1:3].any()
    assert np.array_equal(w[:, sc.INDEX_WORD], np.arange(1025))
    other = np.delete(w, [0, 1, 2, sc.INDEX_WORD], axis=1)
    assert other.shape[1] == 20 and np.unique(other).size == other.size
    assert not np.array_equal(other, np.delete(sc.records_with_keys(bits, seed=8).view(np.uint32), [0, 1, 2, sc.INDEX_WORD], axis=1))


def test_down_and_up_visits_every_size_large_small_large():
    order = sc.down_and_up(sc.SIZES)
    assert sorted(order) == sorted(sc.SIZES) and order[0] == max(sc.SIZES) and min(sc.SIZES) not in (order[0], order[-1])
    low = order.index(min(sc.SIZES))
    assert order[:low + 1] == sorted(order[:low + 1], reverse=True) and order[low:] == sorted(order[low:])
    assert order[-1] > 1000


@pytest.mark.parametrize("name", sc.RANGE_SETS)
def test_range_sets_have_their_named_range(name):
    r, smallest = sc.RANGE_SETS[name]
    for n in sc.SIZES:
        bits = sc.key_bits(name, n)
        keys = keys_of(name, n)
        assert np.array_equal(keys, bits), (name, n)                       # 1 * x + 0 leaves every one of these patterns alone
        assert int(keys.min()) == smallest, (name, n)
        assert int(keys.max()) - int(keys.min()) == (r if n > 1 else 0), (name, n)


@pytest.mark.parametrize("name", [k for k in sc.RANGE_SETS if k.endswith("_hi")])
def test_the_second_view_keeps_the_range_of_the_large_minimum_sets(name):
    r, smallest = sc.RANGE_SETS[name]
    for n in sc.SIZES:
        keys = keys_of(name, n, SECOND)
        assert int(keys.min()) == smallest + 0x00800000 and int(keys.max()) - int(keys.min()) == (r if n > 1 else 0), (name, n)


def test_the_24_25_bit_switch_lies_between_the_two_named_sets():
    """m2s_sort.hip sorts key - min over `bits` bits while (bits + 7) / 8 < 4: 0xFFFFFF is the last such range, 0x1000000 the first
    that takes all 32 bits."""
    assert 0xFFFFFF in sc.RANGES and 0x1000000 in sc.RANGES
    assert (0xFFFFFF).bit_length() == 24 and (0x1000000).bit_length() == 25


def test_special_sets_keep_their_character_in_both_views():
    for view in (VIEW, SECOND):
        for n in sc.SIZES[2:]:
            k = keys_of("mixed_sign", n, view)
            assert (k >> 31).any() and not (k >> 31).all()                  # in front of and behind the camera
            assert sc.INF_POS in k and sc.INF_NEG in k and 0 in k and 0x80000000 not in k      # (-0 has become +0)
            assert int(k.max()) - int(k.min()) > 0xFFFFFF
            d = keys_of("denormals", n, view)
            assert np.all(((d >> 23) & 0xFF) <= 1) and np.all((d & 0x7FFFFFFF) != 0) and (d >> 31).any() and not (d >> 31).all()
            q = keys_of("quiet_nans", n, view)
            finite = ((q >> 23) & 0xFF) != 0xFF
            assert finite.sum() > n // 2 and (q[finite] >> 31).any() and not (q[finite] >> 31).all()
            assert all(v in q for v in (sc.QNAN_POS, sc.QNAN_NEG, sc.INF_POS, sc.INF_NEG))
    k = keys_of("mixed_sign", 63)
    assert 0x7F7FFFFF in k and 0xFF7FFFFF in k and 0x00000001 in k and 0x80000001 in k and 0x00800000 in k and 0x80800000 in k
    assert np.all(((keys_of("denormals", 40_000) >> 23) & 0xFF) == 0)


def test_the_quiet_nans_keep_their_bits_through_the_reference_formula():
    for view in (VIEW, SECOND):
        for n in sc.SIZES:
            bits = sc.key_bits("quiet_nans", n)
            keys = keys_of("quiet_nans", n, view)
            nan = ((bits >> 23) & 0xFF == 0xFF) & ((bits & 0x7FFFFF) != 0)
            assert nan.any() and set(bits[nan].tolist()) <= {sc.QNAN_POS, sc.QNAN_NEG}
            assert np.array_equal(keys[nan], bits[nan]), n
    assert {sc.QNAN_POS, sc.QNAN_NEG} <= set(sc.key_bits("quiet_nans", 2).tolist())


@pytest.mark.parametrize("name", sc.KEY_SETS)
def test_every_key_set_has_equal_keys_at_distant_positions(name):
    for n in sc.SIZES:
        if n >= 3:
            assert has_distant_tie(keys_of(name, n)), (name, n)
            assert has_distant_tie(keys_of(name, n, SECOND)), (name, n)


# ---- the cull sets ----------------------------------------------------------------------------------------------------------------------
def cull_camera():
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), camera.perspective(45.0, 1.0, 0.01, 100.0)


@pytest.mark.parametrize("name", sc.CULL_SETS)
def test_cull_sets_survivors_culled_and_range(name):
    r, smallest, layout = sc.CULL_SETS[name]
    model, view, proj = cull_camera()
    for n in sc.CULL_SIZES:
        rec = sc.cull_records(name, n)
        alive = sc.cull_survivors(name, n)
        inside, z = sc.frustum_test(rec, model, view, proj)
        assert np.array_equal(inside, alive), (name, n)                   # every survivor passes the guard-band test, every culled record fails it
        assert np.array_equal(z, rec[:, 2].view(np.uint32))                # identity model and view: the key is z itself
        assert np.array_equal(rec.view(np.uint32)[:, 20], np.arange(n, dtype=np.float32).view(np.uint32))
        m = int(alive.sum())
        assert m == {"one": 1, "none": n, "all": 0}.get(layout, m)
        if layout == "thirds":
            assert m == n - (n + 1) // 3
            for w in range(0, n, 64):                                      # both kinds in every wave that holds three records or more
                assert n - w < 3 or (alive[w:w + 64].any() and not alive[w:w + 64].all()), (name, n, w)
        if layout == "waves":
            assert not alive[:64].any() and (n <= 64 or alive[64:128].all())
        if m:
            k = z[alive]
            assert int(k.min()) == smallest and int(k.max()) - int(k.min()) == (r if m > 1 else 0), (name, n)
            assert np.all((z >= smallest) & (z <= smallest + r))           # the culled records' z lies among the survivors'
        # ties: among the survivors once there are three of them; the culled records all share one key (the marker, then `behind`)
        if m >= 3:
            assert has_distant_tie(z[alive], np.flatnonzero(alive)), (name, n)
        elif n >= 3:
            assert n - m >= 2


def test_the_cull_ranges_sit_on_both_sides_of_the_24_bit_edge():
    """cull mode sorts over the bits of range + 1 (`behind`, the culled records' key)"""
    assert (sc.CULL_SETS["cull_range_fffffe"][0] + 1).bit_length() == 24 and (sc.CULL_SETS["cull_range_ffffff"][0] + 1).bit_length() == 25
    assert np.array([sc.Z_NEAR, sc.Z_FAR], np.uint32).view(np.float32).tolist() == [np.float32(-0.02), np.float32(-90.0)]
    assert np.array([sc.Z_FIRST], np.uint32).view(np.float32)[0] == -1.0
    assert (sc.CULL_SETS["cull_wide"][0] + 1).bit_length() > 25
