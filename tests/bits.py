"""Bit-level comparison of float32 arrays for the range-end tests (not a test module). np.array_equal cannot see the sign of a zero
and never accepts a NaN; same_bits compares the bit patterns after mapping every NaN to one canonical NaN, so NaN positions must
match exactly, -0 != +0, and a NaN's sign and payload are not compared (x86 and the GPU may differ there; the spec fixes neither)."""
import numpy as np

_QNAN = np.uint32(0x7FC00000)


def canon(a):
    """The uint32 bit patterns of a float32 array, every NaN mapped to 0x7FC00000."""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = _QNAN
    return b


def diff_bits(got, want):
    """Boolean array: where the two differ in the sense of same_bits (shapes must agree)."""
    return canon(got) != canon(want)


def same_bits(got, want, what=""):
    """Asserts got == want bit for bit (see the module docstring); prints the count and, on failure, the first four differing
    elements as (index, got, want, got bits, want bits)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = canon(got), canon(want)
    diff = g != w
    print(f"{what}: {int(np.count_nonzero(diff))} of {want.size} elements differ")
    at = np.argwhere(diff)[:4]
    assert not diff.any(), (what, int(np.count_nonzero(diff)),
                            [(i.tolist(), float(got[tuple(i)]), float(want[tuple(i)]), hex(int(g[tuple(i)])), hex(int(w[tuple(i)]))) for i in at])
