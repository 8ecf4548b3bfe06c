"""CPU tier: the checker of tests/extents.py checks -- every kind of mistake it exists for is planted in host words and must be
reported, with the right place; a clean buffer passes.  Pure numpy, no GPU."""
import numpy as np
import pytest

import extents as X

BEFORE, COLS, N, AFTER = 40, 3, 100, X.GUARD
EXTENT = COLS * N


def _buffer(seed=5):
    """(what a kernel that is right leaves, the poison uploaded before it): canonical values in the extent, poison around it"""
    pz = X.poison(BEFORE + EXTENT + AFTER, seed)
    got = pz.copy()
    got[BEFORE: BEFORE + EXTENT] = np.arange(EXTENT, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF) % np.uint64(X.P)
    return got, pz


def test_poison_is_never_canonical_and_depends_on_position_and_seed():
    a = X.poison(1 << 16, 7)
    assert a.dtype == np.uint64 and (a > np.uint64(X.P)).all()
    assert np.unique(a).size > 65000  # (2^32 - 2 values: hardly a repeat in 2^16 draws)
    assert (X.poison(100, 7) == a[:100]).all()  # a word depends on its position and the seed, not on the length
    assert (X.poison(1 << 16, 8) != a).mean() > 0.99
    # the two ends of the range: P + 1 and 2^64 - 1 are the smallest and the largest word the formula can give
    assert X.P + 1 + (2**32 - 3) == 2**64 - 1


def test_clean_buffer_passes_and_returns_the_extent():
    got, pz = _buffer()
    ext = X.check_words(got, pz, BEFORE, EXTENT, "all", (COLS, N))
    assert ext.size == EXTENT and (ext == got[BEFORE: BEFORE + EXTENT]).all()
    mask = np.zeros(EXTENT, dtype=bool)
    mask[:N] = True  # a header that promises the first column only: the rest must still be poison
    got[BEFORE + N: BEFORE + EXTENT] = pz[BEFORE + N: BEFORE + EXTENT]
    X.check_words(got, pz, BEFORE, EXTENT, mask)
    X.check_words(pz.copy(), pz, BEFORE, EXTENT, None)  # an extent that is not judged


def test_stray_store_behind_the_extent_is_named_with_column_and_row():
    got, pz = _buffer()
    got[BEFORE + EXTENT + 3] = 17  # a kernel that ran to row N + 3 of the last column
    got[BEFORE + EXTENT + 9] = 0
    with pytest.raises(AssertionError) as e:
        X.check_words(got, pz, BEFORE, EXTENT, "all", (COLS, N))
    msg = str(e.value)
    assert "stray stores BEHIND the extent" in msg and "2 words" in msg and "first at offset +3" in msg and "last at +9" in msg
    assert "(column %d, row %d)" % (COLS - 1, N + 3) in msg and "(column %d, row %d)" % (COLS - 1, N + 9) in msg


def test_stray_store_in_the_last_guard_word_is_seen():
    got, pz = _buffer()
    got[-1] = 1
    with pytest.raises(AssertionError, match=r"1 words, first at offset \+%d" % (AFTER - 1)):
        X.check_words(got, pz, BEFORE, EXTENT)


def test_stray_store_before_the_extent_is_reported():
    got, pz = _buffer()
    got[BEFORE - 1] = 12345
    got[0] = 5
    with pytest.raises(AssertionError) as e:
        X.check_words(got, pz, BEFORE, EXTENT)
    msg = str(e.value)
    assert "stray stores BEFORE the extent" in msg and "2 words" in msg and "first at offset -%d" % BEFORE in msg and "last at -1" in msg


def test_poison_left_inside_the_extent_is_reported():
    got, pz = _buffer()
    got[BEFORE + 2 * N + 7] = pz[BEFORE + 2 * N + 7]  # one cell the kernel never stored
    with pytest.raises(AssertionError) as e:
        X.check_words(got, pz, BEFORE, EXTENT)
    assert "never stored" in str(e.value) and "1 words" in str(e.value) and "first at offset -%d" % (EXTENT - (2 * N + 7)) in str(e.value)
    # also where only a part is promised, inside that part
    mask = np.zeros(EXTENT, dtype=bool)
    mask[2 * N:] = True
    got[BEFORE: BEFORE + 2 * N] = pz[BEFORE: BEFORE + 2 * N]
    with pytest.raises(AssertionError, match="never stored"):
        X.check_words(got, pz, BEFORE, EXTENT, mask)


def test_store_into_a_part_the_header_leaves_alone_is_reported():
    got, pz = _buffer()
    mask = np.zeros(EXTENT, dtype=bool)
    mask[:N] = True
    got[BEFORE + N: BEFORE + EXTENT] = pz[BEFORE + N: BEFORE + EXTENT]
    got[BEFORE + N + 1] = 3
    with pytest.raises(AssertionError, match="the header leaves alone"):
        X.check_words(got, pz, BEFORE, EXTENT, mask)


def test_poison_moved_by_one_position_is_reported():
    """a copy that overshoots out of another poisoned region stores words that are not canonical: only their position gives them away"""
    got, pz = _buffer()
    end = BEFORE + EXTENT
    got[end: end + 64] = pz[end + 1: end + 65]
    with pytest.raises(AssertionError) as e:
        X.check_words(got, pz, BEFORE, EXTENT)
    assert "poison moved" in str(e.value) and "first at offset +0" in str(e.value)
    got, pz = _buffer()
    got[1:BEFORE] = pz[: BEFORE - 1]
    with pytest.raises(AssertionError, match="BEFORE the extent"):
        X.check_words(got, pz, BEFORE, EXTENT)


class _Held:
    """what assert_preserved reads of a Guarded buffer, on the host"""

    def __init__(self, words, off, extent):
        self.words, self.off, self.extent, self.name = words, off, extent, "input"

    def download(self):
        return self.words.copy()


def test_assert_preserved_sees_the_input_and_both_sides_of_it():
    got, _ = _buffer()
    g = _Held(got, BEFORE, EXTENT)
    snap = X.snapshot(g)
    X.assert_preserved(g, snap)
    for at, what in ((BEFORE + 5, "const input was changed"), (BEFORE + EXTENT, "BEHIND a const input"), (BEFORE - 1, "BEFORE a const input")):
        g.words = got.copy()
        g.words[at] ^= np.uint64(1)
        with pytest.raises(AssertionError, match=what):
            X.assert_preserved(g, snap)
