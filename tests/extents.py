"""Poisoned buffers and guard zones: does a kernel store every word of its documented extent, and nothing outside it?

Poison and guards see STORES, never loads: a kernel that reads outside its input is invisible here.
A guard sees a store past either end of the whole buffer region; for a column-major output that is the LAST column's overshoot only.
Overshoot of an earlier column lands inside the extent, in the next column: only a comparison of the WHOLE extent with a reference sees it.

Every documented device output of the library is canonical (< P), every poison word is not and depends on its position, so
  - a word < P inside a guard is a stray store,
  - a word >= P inside an extent is a store that never happened,
  - a block of poison copied from elsewhere no longer matches its position.
This module holds no tests and is no conftest: tests/test_extents.py proves the checker checks, tests/test_gpu_extents.py uses it.
"""
import numpy as np

P = 2**64 - 2**32 + 1
# two times the largest per-block footprint of the kernels: SCAN_TILE (csrc/vx_lookup.hip), PP_TILE (csrc/vx_plonk.hip) and the NTT
# tile (csrc/vx_ntt.hip: "each pass stages a [R rows x T columns] tile (R*T = 4096 elements)") are each 4096 elements
GUARD = 2 * 4096


def _mix(x):
    """SplitMix64's finaliser on a uint64 array (wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def poison(n, seed):
    """n words, all non-canonical: P + 1 + h(seed, i) mod (2^32 - 2) for i < n, so every word is in (P, 2^64)."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        h = _mix(i * np.uint64(0x9E3779B97F4A7C15) + _mix(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15)))
    return np.uint64(P + 1) + h % np.uint64(2**32 - 2)


def _where(bad, rel0, shape):
    """count, first and last offset of the bad words, and the (column, row) a run past the last row of a [cols][n] extent would mean"""
    at = np.nonzero(bad)[0]
    first, last = int(at[0]) + rel0, int(at[-1]) + rel0
    msg = "%d words, first at offset %+d, last at %+d" % (at.size, first, last)
    if shape is not None and first >= 0:
        cols, n = shape
        msg += "; past the last row that is (column %d, row %d) .. (column %d, row %d)" % (cols - 1, n + first, cols - 1, n + last)
    return msg


def check_words(got, want_poison, before, extent, written="all", shape=None, name="buffer"):
    """The checker itself, on host words: `got` is the whole buffer after the kernel, `want_poison` what was uploaded before it.
    written: "all" (the whole extent is stored), a boolean mask over the extent (those words are stored, the others are NOT touched)
    or None (the extent is not judged: an in-place input).  Offsets in a message are relative to the extent's END for the guard
    behind it and to its START (negative) for the guard before it.  Returns the extent."""
    got = np.asarray(got, dtype=np.uint64)
    assert got.size == want_poison.size, "%s: %d words downloaded, %d allocated" % (name, got.size, want_poison.size)
    end = before + extent
    bad = got[end:] != want_poison[end:]
    if bad.any():
        kind = "stray stores" if (got[end:][bad] < np.uint64(P)).all() else "words changed (poison moved?)"
        raise AssertionError("%s: %s BEHIND the extent: %s" % (name, kind, _where(bad, 0, shape)))
    bad = got[:before] != want_poison[:before]
    if bad.any():
        kind = "stray stores" if (got[:before][bad] < np.uint64(P)).all() else "words changed (poison moved?)"
        raise AssertionError("%s: %s BEFORE the extent: %s" % (name, kind, _where(bad, -before, None)))
    ext = got[before:end]
    if written is None:
        return ext
    mask = np.ones(extent, dtype=bool) if isinstance(written, str) and written == "all" else np.asarray(written, dtype=bool).reshape(-1)
    assert mask.size == extent, "%s: a mask of %d words for an extent of %d" % (name, mask.size, extent)
    bad = mask & (ext >= np.uint64(P))
    if bad.any():
        raise AssertionError("%s: words of the extent never stored (still not canonical): %s" % (name, _where(bad, -extent, None)))
    bad = ~mask & (ext != want_poison[before:end])
    if bad.any():
        raise AssertionError("%s: words of the extent stored that the header leaves alone: %s" % (name, _where(bad, -extent, None)))
    return ext


def as_words(values):
    """an array as contiguous uint64 words; bytes (a header buffer) are padded with zeros to whole words, as Context.from_host does"""
    a = np.ascontiguousarray(values)
    if a.dtype == np.uint64:
        return a.reshape(-1)
    if a.dtype != np.uint8:
        return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    raw = np.zeros((a.size + 7) // 8 * 8, dtype=np.uint8)
    raw[: a.size] = a.reshape(-1)
    return raw.view(np.uint64)


class Guarded:
    """One vx_buf of before + extent + after words, poison over all of it.  `.buf` goes to the library, `.off` is where the extent
    starts (pass it where the API has an offset argument; before = 0 everywhere else)."""

    def __init__(self, ctx, extent_words, before=0, after=GUARD, seed=1, shape=None, name="buffer"):
        self.extent, self.off, self.after, self.shape, self.name = int(extent_words), int(before), int(after), shape, name
        self.poison = poison(self.off + self.extent + self.after, seed)
        self.buf = ctx.alloc(self.poison.size).upload(self.poison)
        self.last = None  # the whole buffer as check() last saw it: the snapshot of an output that is the next call's input

    @classmethod
    def holding(cls, ctx, values, before=0, after=GUARD, seed=2, name="input"):
        """an INPUT: `values` (words, or bytes padded with zeros to whole words) in the extent, poison around it"""
        v = as_words(values)
        g = cls(ctx, v.size, before, after, seed, name=name)
        if v.size:
            g.buf.upload(v, off=g.off)
        return g

    def download(self):
        return self.buf.download()

    def check(self, written="all", shape=None):
        self.last = self.download()
        return check_words(self.last, self.poison, self.off, self.extent, written, shape or self.shape, self.name)

    def free(self):
        self.buf.free()


def snapshot(g):
    """every word of a Guarded input, guards included, before the call that must preserve it"""
    return g.download()


def assert_preserved(g, snap):
    """the input the header declares const / preserved is the same words, and nothing was stored around it"""
    now = g.download()
    end = g.off + g.extent
    bad = now[g.off:end] != snap[g.off:end]
    assert not bad.any(), "%s: a const input was changed: %s" % (g.name, _where(bad, -g.extent, None))
    bad = now[end:] != snap[end:]
    assert not bad.any(), "%s: stores BEHIND a const input: %s" % (g.name, _where(bad, 0, None))
    bad = now[:g.off] != snap[:g.off]
    assert not bad.any(), "%s: stores BEFORE a const input: %s" % (g.name, _where(bad, -g.off, None))
